"""What estimating homographies from match lists costs on the device (include/oetr_homography_ransac.h,
csrc/homography_ransac.hip), in one run.

Cells: 1024 and 256 pairs x 2048 rows, ``n_hyp`` 256, half of the rows outliers, 0.5 px noise (16 distinct scenes of
``tests/homography_ransac_oracle.py``, repeated over the pairs; every pair draws its own samples), ``refit_iters`` 0
and 2.  Per cell
  full_r0 / full_r2  one ``oetr_homography_ransac`` call through ``estimate_homographies`` on device tensors; their
                difference is the cost of the two refit rounds,
  models        the ``models=`` route (``refit_iters`` 0) on the 256 models the full call left in its workspace (no
                sampling, no solving): full_r0 - models is the solver's share,
  models_512    the same with each pair's models twice (two scoring tiles per pair): models_512 - models is what ONE MORE
                scoring tile per pair costs.  That MARGINAL tile is cheaper than the first one - with one tile per pair
                the scoring kernel runs at four waves per SIMD (one at 256 pairs) and does not fill the float64 pipe -
                so `models` is not split further here: per-kernel times come from a kernel trace (``--kernels``),
and the yardsticks, taken in the same run:
  (a) numpy     the specification (``homography_ransac_oracle.estimate``) on the host, wall time per pair,
  (b) torch     the SCORING stage restated in torch float64 on the device - per pair a broadcast over [models, rows],
                the same elementwise operations, equal counts - timed over 16 pairs and scaled to the cell,
  (c) pose      ``oetr_pose_ransac`` through its ``models=`` route with 256 and with 512 finite models on the same
                lists, compared with ``k_hr_score`` on two bases: the marginal tile (pose_512 - pose_256 against
                models_512 - models), and the whole one-tile route (pose_256 = ``k_pr_score`` + ``k_pr_pose`` against
                models = ``k_hr_score`` + ``k_hr_finish``).
Four pairs per cell are first checked bit for bit against the specification.  Device variants are captured into a HIP
graph of CALLS back-to-back calls (the host's enqueue cost is not part of the number) and replayed between device
events; the variants alternate over ROUNDS after a warm-up replay; medians.

    python tools/homography_ransac_probe.py [--out profiles/homography_ransac_probe.json] [--dry-run] [--rows M] [--shrink K]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/homography_ransac_probe.py --kernels

``--kernels`` only issues the cells' calls (12 each: ``refit_iters`` 0 and 2, then the pose entry's ``models=`` route
with 256 models), without graphs and without writing anything: the workload of a kernel trace, in a run of its own.

``--dry-run`` does everything up to the first device call - input generation, the host specification on the checked
pairs, the JSON skeleton (printed, not written) - and needs no GPU.  ``--rows`` / ``--shrink`` (divides the pair
counts) shrink the workload for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as MET / MISSED, not gated): (1) the whole call, with the refit, takes less
device time than the torch restatement of its scoring stage alone (b); (2) a tile of ``k_hr_score`` takes no more device
time per (model, row) than a tile of ``k_pr_score`` (c), within the larger of 3 % and the spread between rounds."""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402
import homography_ransac_oracle as hro  # noqa: E402
import match_score_oracle as mso  # noqa: E402
import pose_ransac_oracle as pro  # noqa: E402

CALLS, ROUNDS = 10, 9
CELLS = (1024, 256)                                     # pairs, x --rows
N_HYP, SEED, PX_THR = 256, 5, 3.0
SCENES = 16
CHECKED = 4                                             # pairs checked bit for bit against the specification
TORCH_PAIRS = 16
VALU_PER_MODEL_ROW = 23                                 # the estimate's float64 issues per (model, row): 12 mul, 9 add, 2 cmp
POSE_VALU_PER_MODEL_ROW = 33                            # k_pr_score's, counted from its ISA


def measure(graphs):
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, (g, calls) in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / calls)
    return {k + '_us': stats(v) for k, v in us.items()}


def torch_score(params, k1, k2, models, n_rows, px_thr):
    """The scoring stage in torch, float64 on the device: per pair a broadcast over [models, rows]."""
    counts = []
    for p in range(models.shape[0]):
        P = params[p]
        a, b = k1[p * n_rows:(p + 1) * n_rows].to(torch.float64), k2[p * n_rows:(p + 1) * n_rows].to(torch.float64)
        s1, s2 = (P[9] + P[10]) / 2.0, (P[11] + P[12]) / 2.0
        x1, y1 = ((a[:, 0] - (P[9] - 1.0) / 2.0) / s1)[None], ((a[:, 1] - (P[10] - 1.0) / 2.0) / s1)[None]
        x2, y2 = ((b[:, 0] - (P[11] - 1.0) / 2.0) / s2)[None], ((b[:, 1] - (P[12] - 1.0) / 2.0) / s2)[None]
        thr_n = px_thr / s2
        h = [models[p, :, k][:, None] for k in range(9)]
        a0 = (h[0] * x1 + h[1] * y1) + h[2]
        a1 = (h[3] * x1 + h[4] * y1) + h[5]
        a2 = (h[6] * x1 + h[7] * y1) + h[8]
        dx, dy = x2 * a2 - a0, y2 * a2 - a1
        n = ((a2 > 0.0) & (dx * dx + dy * dy < (thr_n * thr_n) * (a2 * a2))).sum(1, dtype=torch.int32)
        counts.append(torch.where(torch.isfinite(models[p]).all(1), n, torch.full_like(n, -1)))
    return torch.stack(counts)


def spread(rec, key):
    s = rec[key + '_us']
    return (s['max'] - s['min']) / s['median']


def cell(dev, n_pairs, n_rows, dry_run):
    scenes = [hro.make_scene(n_rows, seed=4000 + s, noise=0.5, outliers=0.5)[:3] for s in range(min(SCENES, n_pairs))]
    blocks = np.stack([scenes[p % len(scenes)][0] for p in range(n_pairs)])
    k1 = np.concatenate([scenes[p % len(scenes)][1] for p in range(n_pairs)])
    k2 = np.concatenate([scenes[p % len(scenes)][2] for p in range(n_pairs)])
    picked = list(range(0, n_pairs, max(1, n_pairs // CHECKED)))[:CHECKED]
    want, host_ms = {}, []
    for p in picked:
        t = time.perf_counter()
        want[p] = hro.estimate(*scenes[p % len(scenes)], N_HYP, SEED, PX_THR, 2, p)
        host_ms.append((time.perf_counter() - t) * 1e3)
    rec = {'cell': f'{n_pairs} pairs x {n_rows} rows', 'pairs': n_pairs, 'rows': n_pairs * n_rows, 'n_hyp': N_HYP,
           'pairs_checked': picked, 'numpy_ms_per_pair': stats(host_ms),
           'finite_models_of_checked': [int(want[p]['counts'][1]) for p in picked],
           'counts_of_checked': [[int(c) for c in want[p]['counts']] for p in picked],
           'corner_error_px_of_checked': [hro.mean_corner_error(want[p]) for p in picked]}
    if dry_run:
        return rec
    from imagematching_oetr_amd import estimate_homographies, estimate_poses
    from imagematching_oetr_amd.homography_ransac import workspace_views
    params = torch.from_numpy(blocks).to(dev)
    d1, d2 = torch.from_numpy(k1).to(dev), torch.from_numpy(k2).to(dev)
    offsets = torch.arange(n_pairs + 1, dtype=torch.int32, device=dev) * n_rows
    call = lambda r, **kw: estimate_homographies(params, d1, d2, offsets=offsets, n_hyp=N_HYP, seed=SEED, px_thr=PX_THR,
                                                 refit_iters=r, **kw)
    out2, out0 = call(2), call(0)
    torch.cuda.synchronize()
    models, model_counts = workspace_views(out2)
    for p, w in want.items():                                         # bit for bit against the specification
        assert mso.equal_bits(models[p].cpu().numpy(), w['models']), p
        assert np.array_equal(model_counts[p].cpu().numpy(), w['model_counts']), p
        for k in ('model', 'H', 'corner_sq'):
            assert mso.equal_bits(out2[k][p].cpu().numpy(), w[k]), (p, k)
        assert out2['counts'][p].cpu().tolist() == w['counts'].tolist(), p
        assert np.array_equal(out2['inliers'][p * n_rows:(p + 1) * n_rows].cpu().numpy(), w['inliers']), p
    counts = out2['counts'].cpu().numpy()
    finite = int(counts[:, 1].sum())
    rec['finite_models'], rec['finite_share'] = finite, finite / (n_pairs * N_HYP)
    rec['refit_rounds_accepted'] = int(counts[:, 5].sum())
    rec['inliers_gained_by_refit'] = int((counts[:, 4] - counts[:, 3]).sum())
    from imagematching_oetr_amd import homography_errors
    e0, e2 = homography_errors(out0), homography_errors(out2)
    rec['mean_corner_error_px'] = {'refit_0': float(e0.mean()), 'refit_2': float(e2.mean())}
    kept = models.clone()
    twice = torch.cat([kept, kept], 1).contiguous()
    routed = estimate_homographies(params, d1, d2, offsets=offsets, models=kept, px_thr=PX_THR, refit_iters=0)
    routed2 = estimate_homographies(params, d1, d2, offsets=offsets, models=twice, px_thr=PX_THR, refit_iters=0)
    torch.cuda.synchronize()
    for k in ('model', 'H', 'corner_sq', 'counts', 'inliers'):
        assert torch.equal(routed[k].view(torch.uint8), out0[k].view(torch.uint8)), k
    n_torch = min(TORCH_PAIRS, n_pairs)
    tc = torch_score(params, d1, d2, kept[:n_torch], n_rows, PX_THR)
    rec['torch_restatement_equal'] = bool(torch.equal(tc, model_counts[:n_torch]))
    # (c) the pose entry on the same lists: any camera blocks, finite models
    pose_blocks = torch.from_numpy(np.stack([pro.make_scene(8, seed=s)[0] for s in range(len(scenes))])).to(dev)
    pose_params = pose_blocks[torch.arange(n_pairs, device=dev) % len(scenes)].contiguous()
    g = torch.Generator(device='cpu').manual_seed(1)
    F256 = torch.randn(n_pairs, 256, 9, generator=g, dtype=torch.float64).to(dev)
    F512 = torch.cat([F256, F256], 1).contiguous()
    pose = lambda F, **kw: estimate_poses(pose_params, d1, d2, offsets=offsets, models=F, px_thr=1.0, **kw)
    p256, p512 = pose(F256), pose(F512)
    rec.update(measure({
        'full_r2': (graph_of(lambda: call(2, out=out2), CALLS), CALLS),
        'full_r0': (graph_of(lambda: call(0, out=out0), CALLS), CALLS),
        'models': (graph_of(lambda: estimate_homographies(params, d1, d2, offsets=offsets, models=kept, px_thr=PX_THR,
                                                          refit_iters=0, out=routed), CALLS), CALLS),
        'models_512': (graph_of(lambda: estimate_homographies(params, d1, d2, offsets=offsets, models=twice,
                                                              px_thr=PX_THR, refit_iters=0, out=routed2), CALLS), CALLS),
        'pose_256': (graph_of(lambda: pose(F256, out=p256), CALLS), CALLS),
        'pose_512': (graph_of(lambda: pose(F512, out=p512), CALLS), CALLS),
        'torch_16_pairs': (graph_of(lambda: torch_score(params, d1, d2, kept[:n_torch], n_rows, PX_THR), 1), 1)}))
    med = lambda k: rec[k + '_us']['median']
    rec['torch_scaled_us'] = med('torch_16_pairs') * n_pairs / n_torch
    tile_us, pose_tile_us = med('models_512') - med('models'), med('pose_512') - med('pose_256')
    rec['split_us'] = {'solve': med('full_r0') - med('models'), 'one_tile_and_finish': med('models'),
                       'marginal_tile': tile_us, 'refit_2_rounds': med('full_r2') - med('full_r0')}
    cells = n_pairs * 256 * n_rows
    rec['marginal_tile_ps_per_model_row'] = {'k_hr_score': tile_us * 1e6 / cells, 'k_pr_score': pose_tile_us * 1e6 / cells}
    rec['marginal_tile_us'] = {'k_hr_score': tile_us, 'k_pr_score': pose_tile_us}
    rec['one_tile_route_us'] = {'k_hr_score + k_hr_finish': med('models'), 'k_pr_score + k_pr_pose': med('pose_256')}
    margin = max(0.03, *(spread(rec, k) for k in ('models', 'models_512', 'pose_256', 'pose_512')))
    rec['same_run_margin'] = margin
    rec['no_more_time_per_model_row_than_k_pr_score'] = bool(tile_us <= pose_tile_us * (1.0 + margin)
                                                             and med('models') <= med('pose_256') * (1.0 + margin))
    rec['numpy_scaled_ms'] = rec['numpy_ms_per_pair']['median'] * n_pairs
    rec['ratio_to_torch'] = med('full_r2') / rec['torch_scaled_us']
    rec['ratio_to_numpy'] = med('full_r2') * 1e-3 / rec['numpy_scaled_ms']
    rec['less_time_than_torch'] = bool(med('full_r2') < rec['torch_scaled_us'])
    rec['estimate'] = {'valu_issues_per_model_row': VALU_PER_MODEL_ROW, 'k_pr_score_valu_issues': POSE_VALU_PER_MODEL_ROW,
                       'lane_ops_all_models': VALU_PER_MODEL_ROW * cells,
                       'marginal_tile_lane_ops_per_s': VALU_PER_MODEL_ROW * cells / (tile_us * 1e-6),
                       'one_tile_and_finish_lane_ops_per_s': VALU_PER_MODEL_ROW * cells / (med('models') * 1e-6)}
    rec['pairs_per_s'] = n_pairs / (med('full_r2') * 1e-6)
    return rec


def kernels(n_rows, shrink):
    """The workload of a kernel trace: every cell's calls, 12 each, nothing timed here and nothing written."""
    from imagematching_oetr_amd import estimate_homographies, estimate_poses
    dev = torch.device('cuda', 0)
    scenes = [hro.make_scene(n_rows, seed=4000 + s, noise=0.5, outliers=0.5)[:3] for s in range(SCENES)]
    poses = torch.from_numpy(np.stack([pro.make_scene(8, seed=s)[0] for s in range(SCENES)])).to(dev)
    for n_pairs in (max(1, c // shrink) for c in CELLS):
        at = [p % SCENES for p in range(n_pairs)]
        params = torch.from_numpy(np.stack([scenes[i][0] for i in at])).to(dev)
        d1 = torch.from_numpy(np.concatenate([scenes[i][1] for i in at])).to(dev)
        d2 = torch.from_numpy(np.concatenate([scenes[i][2] for i in at])).to(dev)
        offsets = torch.arange(n_pairs + 1, dtype=torch.int32, device=dev) * n_rows
        for refit in (0, 2):
            out = None
            for _ in range(12):
                out = estimate_homographies(params, d1, d2, offsets=offsets, n_hyp=N_HYP, seed=SEED, px_thr=PX_THR,
                                            refit_iters=refit, out=out)
            torch.cuda.synchronize()
        F = torch.randn(n_pairs, 256, 9, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
        pose_params = poses[torch.as_tensor(at, device=dev)].contiguous()
        out = None
        for _ in range(12):
            out = estimate_poses(pose_params, d1, d2, offsets=offsets, models=F, px_thr=1.0, out=out)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'homography_ransac_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--rows', type=int, default=2048)
    ap.add_argument('--shrink', type=int, default=1)
    ap.add_argument('--kernels', action='store_true')
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.rows, args.shrink)
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('homography_ransac_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/homography_ransac_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__,
           'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/homography_ransac_probe.py',
                                             'imagematching_oetr_amd/csrc/homography_ransac.hip',
                                             'imagematching_oetr_amd/csrc/homography_ransac_math.h',
                                             'tests/homography_ransac_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'n_hyp': N_HYP, 'seed': SEED, 'px_thr': PX_THR, 'shrink': args.shrink,
           'cells': []}
    dev = None
    if not args.dry_run:
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
    for n_pairs in CELLS:
        c = cell(dev, max(1, n_pairs // args.shrink), args.rows, args.dry_run)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    if args.dry_run:
        print(json.dumps(rec, indent=1))
        print('dry run: stopped before the first device call; nothing written')
        return
    rec['expectations'] = {
        'less device time than the torch restatement of the scoring stage (b)':
            'MET' if all(c['less_time_than_torch'] for c in rec['cells']) else 'MISSED',
        'k_hr_score takes no more device time per (model, row) than k_pr_score (c)':
            'MET' if all(c['no_more_time_per_model_row_than_k_pr_score'] for c in rec['cells']) else 'MISSED'}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
