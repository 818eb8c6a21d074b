"""What scoring matches against depth and pose costs on the device (include/oetr_match_score.h, csrc/match_score.hip),
in one run.

Cells: 64 maps of 640 x 640 with 16 pairs per image (1024 pairs) and with 4 pairs per image (256 pairs), 2048 matches
per pair, made by warping true points of map 1 (noise and outliers as in the tests' lists).  Per cell
  scored        one ``oetr_match_score`` call through ``score_matches`` on device tensors (parameter blocks given),
  flags_only    the same with ``values=False`` (no value arrays stored),
and the two yardsticks, taken in the same run:
  (a) numpy     the float64 restatement ``tests/match_score_oracle.py::score`` on the host, per pair,
  (b) copy      a ``Tensor.copy_`` that moves the call's ALGORITHMIC bytes - per match 16 B of keypoints, 32 B of
                values, 1 B of flags and 8 B of depth; the copy reads half of that many bytes and writes the other half.
A few lists are first checked bit for bit against the restatement.  Device variants are captured into a HIP graph of
CALLS back-to-back calls (the host's enqueue cost is not part of the number) and replayed between device events; the
variants alternate over ROUNDS after a warm-up replay; medians.

    python tools/match_score_probe.py [--out profiles/match_score_probe.json] [--dry-run] [--maps N --size S --matches M]

``--dry-run`` does everything up to the first device call - input generation, the host restatement, argument handling,
the JSON skeleton (printed, not written) - and needs no GPU.  ``--maps`` / ``--size`` / ``--matches`` shrink the
workload for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as met / missed, not gated): with values the call takes at most 3x the copy
(1x for the bytes, up to 2x for about 150 float64 operations and twelve float64 divisions per match, which the copy
does not have), and it is faster without the values than with them."""
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
import match_score_oracle as mso  # noqa: E402

CALLS, ROUNDS = 10, 9
CELLS = (('16 pairs per image', 16), ('4 pairs per image', 4))
THR = dict(epi_thr=5e-4, sym_thr=1e-4, px_thr=3.0)
BYTES_PER_MATCH = {'keypoints': 16, 'values': 32, 'flags': 1, 'depth': 8}
HOST_PAIRS = 4                      # pairs the numpy restatement is timed on (and the device results checked against)


def make_inputs(views, per_image, n_matches):
    """-> (pairs, blocks float64 [P,20], k1, k2 float32 [P * n_matches, 2]) of one cell, on the host."""
    n = len(views)
    pairs = [(i, (i + 1 + k) % n) for i in range(n) for k in range(per_image)]
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in pairs])
    lists = [mso.make_matches(views, i, j, n_matches, seed=7000 + p) for p, (i, j) in enumerate(pairs)]
    k1 = np.concatenate([a for a, _ in lists]).astype(np.float32)
    k2 = np.concatenate([b for _, b in lists]).astype(np.float32)
    return pairs, blocks, k1, k2


def host_yardstick(views, pairs, blocks, k1, k2, n_matches):
    """The restatement on the first HOST_PAIRS pairs (spread over the list): results and milliseconds per pair."""
    picked = list(range(0, len(pairs), max(1, len(pairs) // HOST_PAIRS)))[:HOST_PAIRS]
    results, ms = {}, []
    for p in picked:
        i, j = pairs[p]
        rows = slice(p * n_matches, (p + 1) * n_matches)
        t0 = time.perf_counter()
        results[p] = mso.score(views[i]['depth'], views[j]['depth'], blocks[p], k1[rows], k2[rows], **THR)
        ms.append((time.perf_counter() - t0) * 1e3)
    return results, ms


def cell(dev, ds, views, name, per_image, n_matches, dry_run):
    pairs, blocks, k1, k2 = make_inputs(views, per_image, n_matches)
    P, M = len(pairs), len(k1)
    want, host_ms = host_yardstick(views, pairs, blocks, k1, k2, n_matches)
    moved = {k: v * M for k, v in BYTES_PER_MATCH.items()}
    rec = {'cell': f'{views[0]["depth"].shape[0]}x{views[0]["depth"].shape[1]} x{len(views)}, {name}', 'maps': len(views),
           'pairs': P, 'matches_per_pair': n_matches, 'matches': M, 'algorithmic_bytes': moved,
           'algorithmic_bytes_total': sum(moved.values()), 'pairs_restated_on_the_host': sorted(want),
           'numpy_ms_per_pair': stats(host_ms), 'numpy_matches_per_s': n_matches / (statistics.median(host_ms) * 1e-3)}
    if dry_run:
        return rec
    from imagematching_oetr_amd import score_matches
    index = torch.tensor(pairs, dtype=torch.int32, device=dev)
    params = torch.from_numpy(blocks).to(dev)
    d1, d2 = torch.from_numpy(k1).to(dev), torch.from_numpy(k2).to(dev)
    offsets = torch.arange(P + 1, dtype=torch.int32, device=dev) * n_matches
    call = lambda **kw: score_matches(ds, index, d1, d2, offsets=offsets, params=params, **THR, **kw)
    out = call()
    torch.cuda.synchronize()
    flags, counts = out['flags'].cpu().numpy(), out['counts'].cpu().numpy()
    for p, w in want.items():                                         # bit for bit against the restatement
        rows = slice(p * n_matches, (p + 1) * n_matches)
        assert np.array_equal(flags[rows], w['flags']) and counts[p].tolist() == w['counts'].tolist(), p
        for k in mso.VALUES:
            assert mso.equal_bits(out[k][rows].cpu().numpy(), w[k]), (p, k)
    rec['counters_sum'] = counts.sum(0).tolist()
    bare = call(values=False)
    assert torch.equal(bare['flags'], out['flags']) and torch.equal(bare['counts'], out['counts'])
    total = rec['algorithmic_bytes_total']
    src, dst = (torch.empty(total // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    src.zero_()
    graphs = {'scored': graph_of(lambda: call(out=out), CALLS), 'flags_only': graph_of(lambda: call(values=False, out=bare), CALLS),
              'copy': graph_of(lambda: dst.copy_(src), CALLS)}
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / CALLS)
    for k in us:
        rec[k + '_us'] = stats(us[k])
    rec['spread_us'] = max(rec[k + '_us']['max'] - rec[k + '_us']['min'] for k in us)
    rec['matches_per_s'] = M / (rec['scored_us']['median'] * 1e-6)
    rec['matches_per_s_flags_only'] = M / (rec['flags_only_us']['median'] * 1e-6)
    rec['ratio_to_copy'] = rec['scored_us']['median'] / rec['copy_us']['median']
    rec['flags_only_over_scored'] = rec['flags_only_us']['median'] / rec['scored_us']['median']
    rec['speedup_over_numpy'] = rec['matches_per_s'] / rec['numpy_matches_per_s']
    rec['within_3x_of_copy'] = rec['ratio_to_copy'] <= 3.0
    rec['faster_without_values'] = rec['flags_only_us']['median'] < rec['scored_us']['median']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'match_score_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--matches', type=int, default=2048)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('match_score_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/match_score_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__, 'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/match_score_probe.py', 'imagematching_oetr_amd/csrc/match_score.hip',
                                             'tests/match_score_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'thresholds': THR, 'bytes_per_match': BYTES_PER_MATCH, 'cells': []}
    views = mso.make_scene(((args.size, args.size),) * args.maps, seed=640, behind=None)
    dev = ds = None
    if not args.dry_run:
        from imagematching_oetr_amd import DepthSet
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
        ds = DepthSet(dev)
        for v in views:
            ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose'])
    for name, per_image in CELLS:
        c = cell(dev, ds, views, name, min(per_image, args.maps - 1), args.matches, args.dry_run)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    if args.dry_run:
        print(json.dumps(rec, indent=1))
        print('dry run: stopped before the first device call; nothing written')
        return
    rec['expectations'] = {'within_3x_of_copy_in_every_cell': all(c['within_3x_of_copy'] for c in rec['cells']),
                           'faster_without_values_in_every_cell': all(c['faster_without_values'] for c in rec['cells'])}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
