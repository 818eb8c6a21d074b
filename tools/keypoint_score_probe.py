"""What keypoint repeatability against depth and pose costs on the device (include/oetr_keypoint_score.h,
csrc/keypoint_score.hip), in one run.

Cells: 64 maps of 640 x 640 with 2048 keypoints per picture (the sets of tests/keypoint_score_oracle.py: true points
seen in every picture, random ones, duplicated and special rows), 16 pairs per image (1024 pairs) and 4 pairs per image
(256 pairs).  Per cell
  scored          one ``oetr_keypoint_repeatability`` call through ``score_keypoints`` on device tensors (the
                  concatenated form, parameter blocks given), with ``nearest`` and ``dist_sq`` stored,
  counters_only   the same with ``nearest=False``,
and the two yardsticks, taken in the same run:
  (a) numpy       the float64 restatement ``tests/keypoint_score_oracle.py::score`` on the host, per pair,
  (b) torch       what a user would write on the device: float64 ``((p[:, None] - q[None]) ** 2).sum(-1).min(1)`` per
                  pair and direction, looped over the pairs - on points that were projected BEFORE the clock starts
                  (the projection is not charged to it) and with no nearest index and no counters.  It materialises
                  67 MB per pair and direction; it is measured over the first TORCH_PAIRS pairs of the cell and scaled
                  linearly to the cell's pairs (a loop over pairs has no work across pairs), both figures recorded.
A few pairs are first checked bit for bit against the restatement.  Device variants are captured into a HIP graph of
CALLS back-to-back calls (the host's enqueue cost is not part of the number) and replayed between device events; the
variants alternate over ROUNDS after a warm-up replay; medians.

    python tools/keypoint_score_probe.py [--out profiles/keypoint_score_probe.json] [--dry-run]
                                         [--maps N --size S --keypoints K]

``--dry-run`` does everything up to the first device call - input generation, the host restatement, argument handling,
the JSON skeleton (printed, not written) - and needs no GPU.  ``--maps`` / ``--size`` / ``--keypoints`` shrink the
workload for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as met / MISSED, not gated): the call takes less device time than (b) over the
same pairs.  ESTIMATE, unmeasured when it was written down: about 9 float64 VALU issues per distance, hence on the
order of 2 ms for 1024 pairs; the record holds what the call takes and the issues per distance that implies
(time x CUs x 4 SIMDs x 16 float64 lanes per clock x the 2.4 GHz maximum clock / distances: an upper bound, the clock
under load is lower)."""
import argparse
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402
import keypoint_score_oracle as kso  # noqa: E402
import match_score_oracle as mso  # noqa: E402

CALLS, ROUNDS = 10, 9
CELLS = (('16 pairs per image', 16), ('4 pairs per image', 4))
THR = (1.0, 2.0, 3.0, 5.0)
HOST_PAIRS = 4                      # pairs the numpy restatement is timed on (and the device results checked against)
TORCH_PAIRS = 16                    # pairs the torch yardstick is timed on
ESTIMATE = {'f64_valu_issues_per_distance': 9, 'ms_for_1024_pairs': 2.0}
MAX_CLOCK_HZ = 2.4e9                # the part's maximum engine clock: the issue count it implies is an UPPER bound


def host_yardstick(views, kps, pairs, blocks):
    """The restatement on HOST_PAIRS pairs (spread over the list): results and milliseconds per pair."""
    picked = list(range(0, len(pairs), max(1, len(pairs) // HOST_PAIRS)))[:HOST_PAIRS]
    results, ms = {}, []
    for p in picked:
        i, j = pairs[p]
        t0 = time.perf_counter()
        results[p] = kso.score(views[i]['depth'], views[j]['depth'], blocks[p], kps[i], kps[j], THR)
        ms.append((time.perf_counter() - t0) * 1e3)
    return results, ms


def projected_points(views, kps, pairs, blocks, dev):
    """For the torch yardstick: per pair and direction (projected kept points, target keypoints), float64 on the device."""
    jobs = []
    for p, (i, j) in enumerate(pairs):
        for src, dst, reverse in ((i, j, False), (j, i, True)):
            d, pu, pv = kso.project(views[src]['depth'], blocks[p], kps[src], reverse)
            h, w = views[dst]['depth'].shape
            with np.errstate(all='ignore'):
                kept = (d != 0.0) & (pu < w) & (pv < h)
            q = kps[dst].astype(np.float64)
            jobs.append((torch.from_numpy(np.stack([pu[kept], pv[kept]], 1)).to(dev),
                         torch.from_numpy(q[np.isfinite(q).all(1)]).to(dev)))
    return jobs


def cell(dev, ds, views, kps, name, per_image, dry_run):
    n, K = len(views), len(kps[0])
    pairs = [(i, (i + 1 + k) % n) for i in range(n) for k in range(per_image)]
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in pairs])
    P = len(pairs)
    want, host_ms = host_yardstick(views, kps, pairs, blocks)
    distances = 2 * P * K * K
    rec = {'cell': f'{views[0]["depth"].shape[0]}x{views[0]["depth"].shape[1]} x{n}, {K} keypoints per picture, {name}',
           'maps': n, 'pairs': P, 'keypoints_per_picture': K, 'distances': distances,
           'pairs_restated_on_the_host': sorted(want), 'numpy_ms_per_pair': stats(host_ms),
           'numpy_distances_per_s': 2 * K * K / (statistics.median(host_ms) * 1e-3)}
    if dry_run:
        return rec
    from imagematching_oetr_amd import score_keypoints
    index = torch.tensor(pairs, dtype=torch.int32, device=dev)
    params = torch.from_numpy(blocks).to(dev)
    cat = torch.from_numpy(np.concatenate(kps)).to(dev)
    offsets = torch.arange(n + 1, dtype=torch.int32, device=dev) * K
    call = lambda **kw: score_keypoints(ds, index, (cat, offsets, K), THR, params=params, **kw)
    out = call()
    torch.cuda.synchronize()
    counts = out['counts'].cpu().numpy()
    for p, (a, b) in want.items():                                    # bit for bit against the restatement
        for s, w in enumerate((a, b)):
            assert counts[p, s].tolist() == w['counts'].tolist(), (p, s, counts[p, s], w['counts'])
            assert np.array_equal(out['nearest'][p, s].cpu().numpy(), w['nearest']), (p, s)
            assert mso.equal_bits(out['dist_sq'][p, s].cpu().numpy(), w['dist_sq']), (p, s)
    rec['counters_sum'] = counts.sum((0, 1)).tolist()
    rec['kept_share'] = float(counts[:, :, 1].sum() / counts[:, :, 0].sum())
    bare = call(nearest=False)
    assert torch.equal(bare['counts'], out['counts'])
    n_torch = min(TORCH_PAIRS, P)
    jobs = projected_points(views, kps, pairs[:n_torch], blocks, dev)
    keep = [None] * len(jobs)                                         # the minima stay referenced, as a user's would

    def torch_loop():
        for k, (p, q) in enumerate(jobs):
            keep[k] = ((p[:, None] - q[None]) ** 2).sum(-1).min(1).values

    torch_loop()
    for p in (p for p in want if p < n_torch):                        # the yardstick computes the same minima
        for s, w in enumerate(want[p]):
            ours = out['dist_sq'][p, s].cpu().numpy()[w['kept']]
            assert mso.rel_diff(keep[2 * p + s].cpu().numpy(), ours) < 1e-9, (p, s)
    graphs = {'scored': graph_of(lambda: call(out=out), CALLS), 'counters_only': graph_of(lambda: call(nearest=False, out=bare), CALLS),
              'torch': graph_of(torch_loop, CALLS)}
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / CALLS)
    for k in us:
        rec[k + '_us'] = stats(us[k])
    rec['torch_pairs_measured'] = n_torch
    rec['torch_us_per_pair'] = rec['torch_us']['median'] / n_torch
    rec['torch_us_scaled_to_the_cell'] = rec['torch_us_per_pair'] * P
    rec['scored_us_per_pair'] = rec['scored_us']['median'] / P
    rec['speedup_over_torch'] = rec['torch_us_scaled_to_the_cell'] / rec['scored_us']['median']
    rec['counters_only_over_scored'] = rec['counters_only_us']['median'] / rec['scored_us']['median']
    rec['distances_per_s'] = distances / (rec['scored_us']['median'] * 1e-6)
    rec['speedup_over_numpy'] = rec['distances_per_s'] / rec['numpy_distances_per_s']
    rec['f64_lane_issues_per_s'] = torch.cuda.get_device_properties(dev).multi_processor_count * 4 * 16 * MAX_CLOCK_HZ
    rec['implied_f64_valu_issues_per_distance'] = rec['scored_us']['median'] * 1e-6 * rec['f64_lane_issues_per_s'] / distances
    rec['faster_than_torch'] = 'met' if rec['scored_us']['median'] < rec['torch_us_scaled_to_the_cell'] else 'MISSED'
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'keypoint_score_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--keypoints', type=int, default=2048)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('keypoint_score_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/keypoint_score_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__, 'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/keypoint_score_probe.py', 'imagematching_oetr_amd/csrc/keypoint_score.hip',
                                             'tests/keypoint_score_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'thresholds': list(THR), 'estimate_before_measuring': ESTIMATE,
           'cells': []}
    views = mso.make_scene(((args.size, args.size),) * args.maps, seed=640, behind=None)
    kps = kso.make_keypoints(views, (args.keypoints,) * args.maps, seed=2048)
    dev = ds = None
    if not args.dry_run:
        from imagematching_oetr_amd import DepthSet
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
        rec['compute_units'], rec['max_clock_mhz_assumed'] = torch.cuda.get_device_properties(dev).multi_processor_count, MAX_CLOCK_HZ / 1e6
        ds = DepthSet(dev)
        for v in views:
            ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose'])
    for name, per_image in CELLS:
        c = cell(dev, ds, views, kps, name, min(per_image, args.maps - 1), args.dry_run)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    if args.dry_run:
        print(json.dumps(rec, indent=1))
        print('dry run: stopped before the first device call; nothing written')
        return
    first = rec['cells'][0]
    rec['expectations'] = {
        'faster_than_torch_in_every_cell': 'met' if all(c['faster_than_torch'] == 'met' for c in rec['cells']) else 'MISSED',
        'estimate_ms_for_1024_pairs': ESTIMATE['ms_for_1024_pairs'],
        'measured_ms_first_cell': first['scored_us']['median'] / 1e3,
        'measured_pairs_first_cell': first['pairs'],
        'estimate_issues_per_distance': ESTIMATE['f64_valu_issues_per_distance'],
        'implied_issues_per_distance_first_cell': first['implied_f64_valu_issues_per_distance']}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
