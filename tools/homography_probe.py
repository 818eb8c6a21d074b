"""What scoring matches and computing overlap boxes against a homography costs on the device
(include/oetr_homography.h, csrc/homography.hip), in one run.

Match-scoring cells: 1024 and 256 pairs x 2048 matches, lists made as the tests make them.  Per cell
  scored        one ``oetr_homography_match_score`` call through ``score_matches_homography`` on device tensors,
  counts_only   the same with ``values=False`` (``dist_sq`` not stored),
and the two yardsticks, taken in the same run:
  (a) copy      a ``Tensor.copy_`` that moves the call's ALGORITHMIC bytes with values - per match 16 B of keypoints read
                and 8 B of ``dist_sq`` written; the copy reads half of that many bytes and writes the other half,
  (b) torch     a float64 restatement in torch on the device (the same elementwise operations, one kernel each, and the
                per-pair counters by a comparison and a segment sum).
Boxes cells: 8 and 32 pairs of 640 x 640 and 8 pairs of 1024 x 1024, 'perspective' homographies.  Per cell
  boxes         one ``oetr_homography_boxes`` call through ``overlap_boxes_from_homography``,
and the yardsticks
  (a) covis     THIS tree's ``oetr_covis_boxes`` without masks at the same shape, on plane scenes (it reads two depth
                maps and does more per pixel),
  (b) torch     a float64 restatement in torch on the device, pair by pair.
A few lists and every pair are first checked bit for bit against ``tests/homography_oracle.py``.  Device variants are
captured into a HIP graph of CALLS back-to-back calls (the host's enqueue cost is not part of the number) and replayed
between device events; the variants alternate over ROUNDS after a warm-up replay; medians.

    python tools/homography_probe.py [--out profiles/homography_probe.json] [--dry-run] [--matches M] [--shrink K]

``--dry-run`` does everything up to the first device call - input generation, the host restatement, the JSON skeleton
(printed, not written) - and needs no GPU.  ``--matches`` / ``--shrink`` (divides pair counts and picture sides) shrink
the workload for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as met / missed, not gated): match scoring with values takes at most 3x the copy
(a); both entries take less device time than their torch restatement (b); the boxes are not slower than
``oetr_covis_boxes`` at equal shape."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402
import covis_oracle as cvo  # noqa: E402
import homography_oracle as ho  # noqa: E402
import match_score_oracle as mso  # noqa: E402

CALLS, ROUNDS = 10, 9
SCORE_CELLS = (1024, 256)                               # pairs, x --matches
BOX_CELLS = ((8, 640), (32, 640), (8, 1024))            # (pairs, side)
BYTES_PER_MATCH = {'keypoints_read': 16, 'dist_sq_written': 8}
CHECKED = 4                                             # lists checked bit for bit against the restatement
SIZES = ((480, 640), (480, 640))


def measure(graphs):
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / CALLS)
    return {k + '_us': stats(v) for k, v in us.items()}


def torch_score(params, k1, k2, pair_of_row, thr_sq, n_pairs):
    """The restatement in torch, float64 on the device: elementwise operations in the specification's order."""
    h = params[pair_of_row]
    x, y, x2, y2 = (k.to(torch.float64) for k in (k1[:, 0], k1[:, 1], k2[:, 0], k2[:, 1]))
    a0 = (h[:, 0] * x + h[:, 1] * y) + h[:, 2]
    a1 = (h[:, 3] * x + h[:, 4] * y) + h[:, 5]
    a2 = (h[:, 6] * x + h[:, 7] * y) + h[:, 8]
    pu, pv = a0 / a2, a1 / a2
    d = (x2 - pu) * (x2 - pu) + (y2 - pv) * (y2 - pv)
    hits = (d[:, None] <= thr_sq[None, :]).to(torch.int32)
    counts = torch.zeros(n_pairs, thr_sq.numel(), dtype=torch.int32, device=d.device).index_add_(0, pair_of_row, hits)
    return d, counts


def score_cell(dev, n_pairs, n_matches, dry_run):
    kinds = ('similarity', 'perspective', 'zoom_out', 'shift')
    drawn = {p: ho.checked_homography(kinds[p % 4], SIZES, 300 + p)[0] for p in range(min(n_pairs, 64))}
    Hs = [drawn[p % len(drawn)] for p in range(n_pairs)]
    base = [ho.make_matches(Hs[p], SIZES, n_matches, seed=7000 + p) for p in range(min(n_pairs, 64))]
    k1 = np.concatenate([base[p % len(base)][0] for p in range(n_pairs)])
    k2 = np.concatenate([base[p % len(base)][1] for p in range(n_pairs)])
    M = len(k1)
    picked = list(range(0, n_pairs, max(1, n_pairs // CHECKED)))[:CHECKED]
    rows = lambda p: slice(p * n_matches, (p + 1) * n_matches)
    want = {p: ho.score(Hs[p], k1[rows(p)], k2[rows(p)]) for p in picked}
    moved = {k: v * M for k, v in BYTES_PER_MATCH.items()}
    rec = {'cell': f'{n_pairs} pairs x {n_matches} matches', 'pairs': n_pairs, 'matches': M, 'algorithmic_bytes': moved,
           'algorithmic_bytes_total': sum(moved.values()), 'lists_checked': picked}
    if dry_run:
        return rec
    from imagematching_oetr_amd import homography_params, score_matches_homography
    params = homography_params(np.stack(Hs), SIZES[0], SIZES[1], device=dev)
    d1, d2 = torch.from_numpy(k1).to(dev), torch.from_numpy(k2).to(dev)
    offsets = torch.arange(n_pairs + 1, dtype=torch.int32, device=dev) * n_matches
    call = lambda **kw: score_matches_homography(params, d1, d2, offsets=offsets, **kw)
    out = call()
    bare = call(values=False)
    torch.cuda.synchronize()
    counts = out['counts'].cpu().numpy()
    for p, w in want.items():                                         # bit for bit against the restatement
        assert counts[p].tolist() == w['counts'].tolist(), p
        assert mso.equal_bits(out['dist_sq'][rows(p)].cpu().numpy(), w['dist_sq']), p
    assert torch.equal(bare['counts'], out['counts'])
    pair_of_row = torch.arange(n_pairs, device=dev).repeat_interleave(n_matches)
    thr_sq = torch.tensor([float(t) * float(t) for t in ho.THRESHOLDS], dtype=torch.float64, device=dev)
    td, tc = torch_score(params, d1, d2, pair_of_row, thr_sq, n_pairs)
    rec['torch_restatement_equal_bits'] = bool(mso.equal_bits(td.cpu().numpy(), out['dist_sq'].cpu().numpy())
                                               and torch.equal(tc, out['counts'][:, 1:]))
    rec['counters_sum'] = counts.sum(0).tolist()
    total = rec['algorithmic_bytes_total']
    src, dst = (torch.zeros(total // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    rec.update(measure({'scored': graph_of(lambda: call(out=out), CALLS),
                        'counts_only': graph_of(lambda: call(values=False, out=bare), CALLS),
                        'copy': graph_of(lambda: dst.copy_(src), CALLS),
                        'torch': graph_of(lambda: torch_score(params, d1, d2, pair_of_row, thr_sq, n_pairs), CALLS)}))
    med = lambda k: rec[k + '_us']['median']
    rec['matches_per_s'] = M / (med('scored') * 1e-6)
    rec['ratio_to_copy'] = med('scored') / med('copy')
    rec['ratio_to_torch'] = med('scored') / med('torch')
    rec['counts_only_over_scored'] = med('counts_only') / med('scored')
    rec['within_3x_of_copy'] = rec['ratio_to_copy'] <= 3.0
    rec['less_time_than_torch'] = med('scored') < med('torch')
    return rec


def torch_boxes(params, sizes):
    """The boxes' restatement in torch, float64 on the device, pair by pair; ``sizes``: the pictures' (H, W), host."""
    out = []
    (H1, W1), (H2, W2) = sizes
    for P in params:
        v, u = torch.meshgrid(torch.arange(int(H1), device=params.device, dtype=torch.float64),
                              torch.arange(int(W1), device=params.device, dtype=torch.float64), indexing='ij')
        a0 = (P[0] * u + P[1] * v) + P[2]
        a1 = (P[3] * u + P[4] * v) + P[5]
        a2 = (P[6] * u + P[7] * v) + P[8]
        i, j = torch.round(a0 / a2), torch.round(a1 / a2)
        kept = (a2 > 0) & (i >= 0) & (i < W2) & (j >= 0) & (j < H2)
        big = 1e9
        lo = lambda t: torch.where(kept, t, torch.full_like(t, big)).min()
        hi = lambda t: torch.where(kept, t, torch.full_like(t, -big)).max()
        out.append(torch.stack([lo(u), lo(v), hi(u), hi(v), lo(i), lo(j), hi(i), hi(j), kept.sum().to(torch.float64)]))
    return torch.stack(out)


def box_cell(dev, n_pairs, side, dry_run):
    sizes = ((side, side), (side, side))
    drawn = [ho.checked_homography('perspective', sizes, 500 + p) for p in range(n_pairs)]
    rec = {'cell': f'{n_pairs} pairs of {side} x {side}', 'pairs': n_pairs, 'side': side, 'pixels': n_pairs * side * side,
           'counts': [r['count'] for _, r in drawn]}
    if dry_run:
        return rec
    from imagematching_oetr_amd import covis, homography_params, overlap_boxes_from_homography
    params = homography_params(np.stack([h for h, _ in drawn]), sizes[0], sizes[1], device=dev)
    call = lambda **kw: overlap_boxes_from_homography(params, max_size1=sizes[0], **kw)
    out = call()
    torch.cuda.synchronize()
    for p, (_, r) in enumerate(drawn):                                # every pair against the restatement
        assert int(out['overlap_count'][p]) == r['count'], p
        assert out['overlap_box1'][p].tolist() == r['box1'].tolist() and out['overlap_box2'][p].tolist() == r['box2'].tolist(), p
    tb = torch_boxes(params, sizes).cpu().numpy()
    rec['torch_restatement_equal'] = bool(all(
        tb[p, 8] == r['count'] and tb[p, :4].tolist() == r['box1'].tolist() and tb[p, 4:8].tolist() == r['box2'].tolist()
        for p, (_, r) in enumerate(drawn)))
    # yardstick (a): oetr_covis_boxes, no masks, the same number of maps of the same shape
    scenes = [cvo.make_scene('plane', side, side, 900 + p % 4) for p in range(min(n_pairs, 4))]
    t = lambda key, dt: torch.from_numpy(np.stack([scenes[p % len(scenes)][key] for p in range(n_pairs)])).to(dev, dt)
    cparams = covis.covis_params(*(t(k + s, torch.float64) for s in ('1', '2') for k in ('intrinsics', 'pose', 'bbox', 'ratio')))
    depth1, depth2 = t('depth1', torch.float32).contiguous(), t('depth2', torch.float32).contiguous()
    cout = covis.covis_boxes(depth1, depth2, cparams.contiguous())
    rec['covis_counts'] = cout['overlap_count'].cpu().tolist()
    rec.update(measure({'boxes': graph_of(lambda: call(out=out), CALLS),
                        'covis': graph_of(lambda: covis.covis_boxes(depth1, depth2, cparams, out=cout), CALLS),
                        'torch': graph_of(lambda: torch_boxes(params, sizes), 1)}))
    rec['torch_us'] = {k: v * CALLS for k, v in rec['torch_us'].items()}        # its graph holds ONE call
    med = lambda k: rec[k + '_us']['median']
    rec['pixels_per_s'] = rec['pixels'] / (med('boxes') * 1e-6)
    rec['ratio_to_covis'] = med('boxes') / med('covis')
    rec['ratio_to_torch'] = med('boxes') / med('torch')
    rec['not_slower_than_covis'] = med('boxes') <= med('covis')
    rec['less_time_than_torch'] = med('boxes') < med('torch')
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'homography_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--matches', type=int, default=2048)
    ap.add_argument('--shrink', type=int, default=1)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('homography_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/homography_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__, 'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/homography_probe.py', 'imagematching_oetr_amd/csrc/homography.hip',
                                             'imagematching_oetr_amd/csrc/covis.hip', 'tests/homography_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'thresholds': list(ho.THRESHOLDS), 'bytes_per_match': BYTES_PER_MATCH,
           'shrink': args.shrink, 'score_cells': [], 'box_cells': []}
    dev = None
    if not args.dry_run:
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
    for n_pairs in SCORE_CELLS:
        c = score_cell(dev, max(1, n_pairs // args.shrink), args.matches, args.dry_run)
        rec['score_cells'].append(c)
        print(json.dumps(c), flush=True)
    for n_pairs, side in BOX_CELLS:
        c = box_cell(dev, max(1, n_pairs // args.shrink), max(8, side // args.shrink), args.dry_run)
        rec['box_cells'].append(c)
        print(json.dumps(c), flush=True)
    if args.dry_run:
        print(json.dumps(rec, indent=1))
        print('dry run: stopped before the first device call; nothing written')
        return
    verdict = lambda ok: 'MET' if ok else 'MISSED'
    rec['expectations'] = {
        'match scoring within 3x of (a) with values': verdict(all(c['within_3x_of_copy'] for c in rec['score_cells'])),
        'match scoring: less device time than (b)': verdict(all(c['less_time_than_torch'] for c in rec['score_cells'])),
        'boxes: less device time than (b)': verdict(all(c['less_time_than_torch'] for c in rec['box_cells'])),
        'boxes not slower than oetr_covis_boxes at equal shape': verdict(all(c['not_slower_than_covis'] for c in rec['box_cells']))}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
