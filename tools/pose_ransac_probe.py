"""What estimating relative poses from match lists costs on the device (include/oetr_pose_ransac.h,
csrc/pose_ransac.hip), in one run.

Cells: 1024 and 256 pairs x 2048 rows, ``n_hyp`` 256 (768 models per pair), half of the rows outliers, 0.5 px noise
(16 distinct scenes of ``tests/pose_ransac_oracle.py``, repeated over the pairs; every pair draws its own samples).
Per cell
  full          one ``oetr_pose_ransac`` call through ``estimate_poses`` on device tensors,
  models        the same through the ``models=`` route on the models the full call left in its workspace (no sampling,
                no solving): full - models is the solver's share,
  one_model     the ``models=`` route with ONE model per pair: the pose kernel and ONE scoring tile per pair (a tile of
                256 models takes the same time whether one or all of its models are live), so a tile costs
                (models - one_model) / (tiles - 1), the scoring stage `tiles` times that, and the pose kernel the rest
                of one_model,
and the two yardsticks, taken in the same run:
  (a) numpy     the specification (``pose_ransac_oracle.estimate``) on the host, wall time per pair, over the checked pairs,
  (b) torch     the SCORING stage restated in torch float64 on the device - per pair a broadcast over [models, rows] on
                the models of the call's workspace, the same elementwise operations - timed over 16 pairs and scaled to
                the cell.
Four pairs per cell are first checked bit for bit against the specification.  Device variants are captured into a HIP
graph of CALLS back-to-back calls (the host's enqueue cost is not part of the number) and replayed between device
events; the variants alternate over ROUNDS after a warm-up replay; medians.

    python tools/pose_ransac_probe.py [--out profiles/pose_ransac_probe.json] [--dry-run] [--rows M] [--shrink K]

``--dry-run`` does everything up to the first device call - input generation, the host specification on the checked
pairs, the JSON skeleton (printed, not written) - and needs no GPU.  ``--rows`` / ``--shrink`` (divides the pair
counts) shrink the workload for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as met / missed, not gated): the whole call takes less device time than the
torch restatement of its scoring stage alone (b)."""
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
import match_score_oracle as mso  # noqa: E402
import pose_ransac_oracle as pro  # noqa: E402

CALLS, ROUNDS = 10, 9
CELLS = (1024, 256)                                     # pairs, x --rows
N_HYP, SEED, PX_THR = 256, 5, 1.0
SCENES = 16
CHECKED = 4                                             # pairs checked bit for bit against the specification
TORCH_PAIRS = 16
VALU_PER_MODEL_ROW = 36                                 # the estimate's float64 issues per (model, row)


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
        x1, y1 = ((a[:, 0] - P[2]) / P[0])[None], ((a[:, 1] - P[3]) / P[1])[None]
        x2, y2 = ((b[:, 0] - P[6]) / P[4])[None], ((b[:, 1] - P[7]) / P[5])[None]
        thr_n = px_thr / ((P[0] + P[5]) / 2.0)
        F = [models[p, :, k][:, None] for k in range(9)]
        a0 = (F[0] * x1 + F[1] * y1) + F[2]
        a1 = (F[3] * x1 + F[4] * y1) + F[5]
        a2 = (F[6] * x1 + F[7] * y1) + F[8]
        b0 = (F[0] * x2 + F[3] * y2) + F[6]
        b1 = (F[1] * x2 + F[4] * y2) + F[7]
        s = (x2 * a0 + y2 * a1) + a2
        n = (s * s < (thr_n * thr_n) * ((a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1))).sum(1, dtype=torch.int32)
        counts.append(torch.where(torch.isfinite(models[p]).all(1), n, torch.full_like(n, -1)))
    return torch.stack(counts)


def cell(dev, n_pairs, n_rows, dry_run):
    scenes = [pro.make_scene(n_rows, seed=4000 + s, noise=0.5, outliers=0.5)[:3] for s in range(min(SCENES, n_pairs))]
    blocks = np.stack([scenes[p % len(scenes)][0] for p in range(n_pairs)])
    k1 = np.concatenate([scenes[p % len(scenes)][1] for p in range(n_pairs)])
    k2 = np.concatenate([scenes[p % len(scenes)][2] for p in range(n_pairs)])
    picked = list(range(0, n_pairs, max(1, n_pairs // CHECKED)))[:CHECKED]
    want, host_ms = {}, []
    for p in picked:
        t = time.perf_counter()
        want[p] = pro.estimate(*scenes[p % len(scenes)], N_HYP, SEED, PX_THR, p)
        host_ms.append((time.perf_counter() - t) * 1e3)
    n_models = 3 * N_HYP
    rec = {'cell': f'{n_pairs} pairs x {n_rows} rows', 'pairs': n_pairs, 'rows': n_pairs * n_rows, 'n_hyp': N_HYP,
           'models_per_pair': n_models, 'pairs_checked': picked, 'numpy_ms_per_pair': stats(host_ms),
           'finite_models_of_checked': [int(want[p]['counts'][1]) for p in picked],
           'pose_error_deg_of_checked': [pro.error_of(want[p]) for p in picked]}
    if dry_run:
        return rec
    from imagematching_oetr_amd import estimate_poses
    from imagematching_oetr_amd.pose_ransac import workspace_views
    params = torch.from_numpy(blocks).to(dev)
    d1, d2 = torch.from_numpy(k1).to(dev), torch.from_numpy(k2).to(dev)
    offsets = torch.arange(n_pairs + 1, dtype=torch.int32, device=dev) * n_rows
    call = lambda **kw: estimate_poses(params, d1, d2, offsets=offsets, n_hyp=N_HYP, seed=SEED, px_thr=PX_THR, **kw)
    out = call()
    torch.cuda.synchronize()
    models, model_counts = workspace_views(out)
    for p, w in want.items():                                         # bit for bit against the specification
        assert mso.equal_bits(models[p].cpu().numpy(), w['models']), p
        assert np.array_equal(model_counts[p].cpu().numpy(), w['model_counts']), p
        for k in ('model', 'pose', 'cosines'):
            assert mso.equal_bits(out[k][p].cpu().numpy(), w[k]), (p, k)
        assert out['counts'][p].cpu().tolist() == w['counts'].tolist(), p
        assert np.array_equal(out['inliers'][p * n_rows:(p + 1) * n_rows].cpu().numpy(), w['inliers']), p
    counts = out['counts'].cpu().numpy()
    finite = int(counts[:, 1].sum())
    rec['finite_models'] = finite
    rec['finite_share'] = finite / (n_pairs * n_models)
    kept = models.clone()
    routed = estimate_poses(params, d1, d2, offsets=offsets, models=kept, px_thr=PX_THR)
    one = estimate_poses(params, d1, d2, offsets=offsets, models=kept[:, :1].contiguous(), px_thr=PX_THR)
    first = kept[:, :1].contiguous()
    torch.cuda.synchronize()
    for k in ('model', 'pose', 'cosines', 'counts', 'inliers'):
        assert torch.equal(routed[k].view(torch.uint8), out[k].view(torch.uint8)), k
    n_torch = min(TORCH_PAIRS, n_pairs)
    tc = torch_score(params, d1, d2, kept[:n_torch], n_rows, PX_THR)
    rec['torch_restatement_equal'] = bool(torch.equal(tc, model_counts[:n_torch]))
    rec.update(measure({
        'full': (graph_of(lambda: call(out=out), CALLS), CALLS),
        'models': (graph_of(lambda: estimate_poses(params, d1, d2, offsets=offsets, models=kept, px_thr=PX_THR, out=routed), CALLS), CALLS),
        'one_model': (graph_of(lambda: estimate_poses(params, d1, d2, offsets=offsets, models=first, px_thr=PX_THR, out=one), CALLS), CALLS),
        'torch_16_pairs': (graph_of(lambda: torch_score(params, d1, d2, kept[:n_torch], n_rows, PX_THR), 1), 1)}))
    med = lambda k: rec[k + '_us']['median']
    rec['torch_scaled_us'] = med('torch_16_pairs') * n_pairs / n_torch
    tiles = (n_models + 255) // 256
    tile_us = (med('models') - med('one_model')) / (tiles - 1)
    rec['split_us'] = {'solve': med('full') - med('models'), 'score': tiles * tile_us, 'pose': med('one_model') - tile_us,
                       'score_tiles_per_pair': tiles}
    rec['numpy_scaled_ms'] = rec['numpy_ms_per_pair']['median'] * n_pairs
    rec['ratio_to_torch'] = med('full') / rec['torch_scaled_us']
    rec['ratio_to_numpy'] = med('full') * 1e-3 / rec['numpy_scaled_ms']
    rec['less_time_than_torch'] = med('full') < rec['torch_scaled_us']
    # the estimate made beforehand: 36 float64 issues per (model, row) over the FINITE models
    lane_ops = VALU_PER_MODEL_ROW * finite * n_rows
    rec['estimate'] = {'lane_ops_finite_models': lane_ops, 'lane_ops_all_models': VALU_PER_MODEL_ROW * n_pairs * n_models * n_rows,
                       'score_lane_ops_per_s': VALU_PER_MODEL_ROW * n_pairs * n_models * n_rows / (rec['split_us']['score'] * 1e-6)}
    rec['pairs_per_s'] = n_pairs / (med('full') * 1e-6)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'pose_ransac_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--rows', type=int, default=2048)
    ap.add_argument('--shrink', type=int, default=1)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('pose_ransac_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/pose_ransac_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__, 'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/pose_ransac_probe.py', 'imagematching_oetr_amd/csrc/pose_ransac.hip',
                                             'imagematching_oetr_amd/csrc/pose_ransac_math.h', 'tests/pose_ransac_oracle.py')},
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
    rec['expectations'] = {'less device time than the torch restatement of the scoring stage (b)':
                           'MET' if all(c['less_time_than_torch'] for c in rec['cells']) else 'MISSED'}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
