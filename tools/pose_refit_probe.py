"""What refitting relative poses on their inliers costs on the device (include/oetr_pose_refit.h, csrc/pose_refit.hip),
in one run.

Two cells: 1024 and 256 pairs of 2048 rows (0.5 px noise, half the rows outliers; 16 distinct scenes of
``tests/pose_ransac_oracle.py``, repeated over the pairs), ``model_in`` from ``estimate_poses`` at ``n_hyp`` 256 and
``px_thr`` 1.  Four pairs of each cell are checked BIT FOR BIT against the specification (``pose_refit_oracle.refit``
of the device's ``model_in``) before anything is timed.  Timed, each as a HIP graph of 10 back-to-back calls, 9 rounds
alternating between the graphs, medians:

  refit_0 / 1 / 2 / 4   one ``oetr_pose_refit`` call through ``refine_poses`` on device tensors; their differences are
                        what the rounds cost,
  one_model, models_768 ``estimate_poses``' ``models=`` route with one model and with all 768 of a pair: a scoring tile
                        costs (models_768 - one_model) / 2, k_pr_pose's share of ``oetr_pose_ransac`` is one_model
                        minus a tile (the split of tools/pose_ransac_probe.py) - yardstick (a),
  torch_16_pairs        (b) ONE round restated in torch float64 on the device for 16 pairs - the mask, ``einsum`` for
                        ``M``, a batched ``torch.linalg.solve``, the rescoring - scaled to the cell's pairs; timed
                        EAGERLY between device events (the batched solver cannot be captured into a graph),
  hr_r0 / hr_r2         (c) ``estimate_homographies``' ``models=`` route on planar scenes of the same sizes at
                        ``refit_iters`` 0 and 2: their difference is k_hr_finish's refit cost.

Recorded as well: the cell's ``match_pose_auc`` at ``refit_iters`` 0 and 4 and the inliers gained.

    python tools/pose_refit_probe.py [--out profiles/pose_refit_probe.json] [--dry-run] [--rows M] [--shrink K]

``--dry-run`` does everything up to the first device call - input generation, the specification and the torch
restatement (on the CPU) on one scene, the JSON skeleton (printed, not written) - and needs no GPU.  ``--rows`` /
``--shrink`` (divides the pair counts) shrink the workload for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as MET / MISSED, not gated): (a) ``refit_iters`` 0 takes no more device time
than k_pr_pose's share of ``oetr_pose_ransac``, beyond the larger of 3 % and the spread between rounds; (b) one round
takes less device time than its torch restatement; (c) two rounds cost about 1.5 x k_hr_finish's two (44
sums against 28, the same elimination, 33 against 23 VALU issues per scored row) - recorded as a ratio."""
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
import homography_ransac_oracle as hro  # noqa: E402
import match_score_oracle as mso  # noqa: E402
import pose_ransac_oracle as pro  # noqa: E402
import pose_refit_oracle as pfo  # noqa: E402

CALLS, ROUNDS = 10, 9
CELLS = (1024, 256)                                     # pairs, x --rows
N_HYP, SEED, PX_THR = 256, 5, 1.0
SCENES = 16
CHECKED = 4                                             # pairs checked bit for bit against the specification
TORCH_PAIRS = 16
EXPECTED_RATIO_TO_HR = 1.5                              # DESIGN 9.3m, written before the first measurement


def measure(graphs):
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, (g, calls) in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / calls)
    return {k + '_us': stats(v) for k, v in us.items()}


def spread(rec, key):
    s = rec[key + '_us']
    return (s['max'] - s['min']) / s['median']


def torch_round(params, k1, k2, models, n_rows, px_thr):
    """ONE refit round in torch, float64, for every pair of ``models`` [p,9] at once -> (candidates [p,9], their inlier
    counts, the inlier counts of ``models``).  Not the specified operation order: a restatement of the work."""
    n = models.shape[0]
    P = params[:n]
    a = k1[:n * n_rows].to(torch.float64).reshape(n, n_rows, 2)
    b = k2[:n * n_rows].to(torch.float64).reshape(n, n_rows, 2)
    x1, y1 = (a[..., 0] - P[:, 2:3]) / P[:, 0:1], (a[..., 1] - P[:, 3:4]) / P[:, 1:2]
    x2, y2 = (b[..., 0] - P[:, 6:7]) / P[:, 4:5], (b[..., 1] - P[:, 7:8]) / P[:, 5:6]
    thr_n = px_thr / ((P[:, 0:1] + P[:, 5:6]) / 2.0)

    def inliers(F):
        f = [F[:, k:k + 1] for k in range(9)]
        a0, a1, a2 = (f[0] * x1 + f[1] * y1) + f[2], (f[3] * x1 + f[4] * y1) + f[5], (f[6] * x1 + f[7] * y1) + f[8]
        b0, b1 = (f[0] * x2 + f[3] * y2) + f[6], (f[1] * x2 + f[4] * y2) + f[7]
        s = (x2 * a0 + y2 * a1) + a2
        return s * s < (thr_n * thr_n) * ((a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1))

    mask = inliers(models)
    w = torch.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, torch.ones_like(x1)], 2)
    wm = w * mask[..., None].to(torch.float64)
    M = torch.einsum('prm,prn->pmn', wm, w)
    held = models.abs().argmax(1)
    keep = torch.arange(9, device=models.device)[None, :].expand(n, 9)
    keep = keep[keep != held[:, None]].reshape(n, 8)
    A = M.gather(1, keep[:, :, None].expand(n, 8, 9)).gather(2, keep[:, None, :].expand(n, 8, 8))
    rhs = -M.gather(1, keep[:, :, None].expand(n, 8, 9)).gather(2, held[:, None, None].expand(n, 8, 1))
    sol = torch.linalg.solve_ex(A, rhs, check_errors=False)[0][..., 0]
    cand = torch.ones(n, 9, dtype=torch.float64, device=models.device).scatter(1, keep, sol)
    cand = cand / cand.pow(2).sum(1, keepdim=True).sqrt()
    return cand, inliers(cand).sum(1, dtype=torch.int32), mask.sum(1, dtype=torch.int32)


def scene_inputs(n_pairs, n_rows):
    scenes = [pro.make_scene(n_rows, seed=6000 + s, noise=0.5, outliers=0.5)[:3] for s in range(min(SCENES, n_pairs))]
    at = [p % len(scenes) for p in range(n_pairs)]
    return (scenes, np.stack([scenes[i][0] for i in at]), np.concatenate([scenes[i][1] for i in at]),
            np.concatenate([scenes[i][2] for i in at]))


def close_up_to_sign(a, b):
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


def cell(dev, n_pairs, n_rows, dry_run):
    scenes, blocks, k1, k2 = scene_inputs(n_pairs, n_rows)
    picked = list(range(0, n_pairs, max(1, n_pairs // CHECKED)))[:CHECKED]
    rec = {'cell': f'{n_pairs} pairs x {n_rows} rows', 'pairs': n_pairs, 'rows': n_pairs * n_rows, 'n_hyp': N_HYP,
           'pairs_checked': picked}
    if dry_run:                                                       # the host side on one scene
        P, a, b = scenes[0]
        M = pro.estimate(P, a, b, 16, SEED, PX_THR, 0)['model']
        want = pfo.refit(P, a, b, M, PX_THR, 1)
        cand, c, c0 = torch_round(torch.from_numpy(P[None]), torch.from_numpy(a), torch.from_numpy(b),
                                  torch.from_numpy(M[None]), n_rows, PX_THR)
        rec['dry_run_counts'] = [int(v) for v in want['counts']]
        if want['candidates']:
            rec['torch_restatement_distance'] = close_up_to_sign(cand[0].numpy(), want['candidates'][0])
            rec['torch_restatement_counts'] = [int(c0[0]), int(c[0]), int(want['counts'][1]), want['candidate_counts'][0]]
        return rec
    from imagematching_oetr_amd import (estimate_homographies, estimate_poses, match_pose_auc, refine_poses)
    from imagematching_oetr_amd.pose_ransac import workspace_views
    params = torch.from_numpy(blocks).to(dev)
    d1, d2 = torch.from_numpy(k1).to(dev), torch.from_numpy(k2).to(dev)
    offsets = torch.arange(n_pairs + 1, dtype=torch.int32, device=dev) * n_rows
    est = estimate_poses(params, d1, d2, offsets=offsets, n_hyp=N_HYP, seed=SEED, px_thr=PX_THR)
    model_in = est['model'].clone()
    call = lambda r, **kw: refine_poses(params, d1, d2, model_in, offsets=offsets, px_thr=PX_THR, refit_iters=r, **kw)
    outs = {r: call(r) for r in (0, 1, 2, 4)}
    torch.cuda.synchronize()
    host_models = model_in.cpu().numpy()
    for p in picked:                                                  # bit for bit against the specification
        P, a, b = scenes[p % len(scenes)]
        for r in (0, 4):
            w = pfo.refit(P, a, b, host_models[p], PX_THR, r)
            for k in ('model', 'pose', 'cosines'):
                assert mso.equal_bits(outs[r][k][p].cpu().numpy(), w[k]), (p, r, k)
            assert outs[r]['counts'][p].cpu().tolist() == w['counts'].tolist(), (p, r)
            assert np.array_equal(outs[r]['inliers'][p * n_rows:(p + 1) * n_rows].cpu().numpy(), w['inliers']), (p, r)
    for k in ('model', 'pose', 'cosines', 'inliers'):                 # no round: estimate_poses' own tail
        assert torch.equal(outs[0][k].view(torch.uint8), est[k].view(torch.uint8)), k
    c4 = outs[4]['counts'].cpu().numpy()
    rec['rounds_accepted'] = int(c4[:, 2].clip(0).sum())
    rec['inliers_gained_by_4_rounds'] = int((c4[:, 3] - c4[:, 1]).sum())
    rec['inliers_of_model_in'] = int(c4[:, 1].sum())
    rec['match_pose_auc'] = {f'refit_{r}': match_pose_auc(outs[r])['auc'] for r in (0, 1, 2, 4)}
    rec['mean_pose_error_deg'] = {f'refit_{r}': float(np.mean(match_pose_auc(outs[r])['pose_error'])) for r in (0, 4)}
    # (a) k_pr_pose's share of oetr_pose_ransac
    models, _ = workspace_views(est)
    kept = models.clone()
    first = kept[:, :1].contiguous()
    one = estimate_poses(params, d1, d2, offsets=offsets, models=first, px_thr=PX_THR)
    routed = estimate_poses(params, d1, d2, offsets=offsets, models=kept, px_thr=PX_THR)
    # (b) one round in torch
    n_torch = min(TORCH_PAIRS, n_pairs)
    cand, cc, c0 = torch_round(params, d1, d2, model_in[:n_torch], n_rows, PX_THR)
    torch.cuda.synchronize()
    rec['torch_restatement_counts_equal'] = bool(torch.equal(c0, outs[1]['counts'][:n_torch, 1]))
    # torch's batched solver cannot be captured into a graph (it allocates and synchronises): the restatement is timed
    # eagerly between device events, so its figure includes whatever of the host's enqueue the device has to wait for
    rec['torch_timing'] = 'eager, between device events'

    class Eager:
        replay = staticmethod(lambda: torch_round(params, d1, d2, model_in[:n_torch], n_rows, PX_THR))
    torch_graph = Eager
    # (c) k_hr_finish's refit on planar scenes of the same sizes
    hscenes = [hro.make_scene(n_rows, seed=4000 + s, noise=0.5, outliers=0.5)[:3] for s in range(len(scenes))]
    at = [p % len(hscenes) for p in range(n_pairs)]
    hparams = torch.from_numpy(np.stack([hscenes[i][0] for i in at])).to(dev)
    h1 = torch.from_numpy(np.concatenate([hscenes[i][1] for i in at])).to(dev)
    h2 = torch.from_numpy(np.concatenate([hscenes[i][2] for i in at])).to(dev)
    hest = estimate_homographies(hparams, h1, h2, offsets=offsets, n_hyp=N_HYP, seed=SEED, px_thr=3.0, refit_iters=0)
    from imagematching_oetr_amd.homography_ransac import workspace_views as hr_views
    hkept = hr_views(hest)[0].clone()
    hcall = lambda r, **kw: estimate_homographies(hparams, h1, h2, offsets=offsets, models=hkept, px_thr=3.0,
                                                  refit_iters=r, **kw)
    hout = {r: hcall(r) for r in (0, 2)}
    graphs = {f'refit_{r}': (graph_of(lambda r=r: call(r, out=outs[r]), CALLS), CALLS) for r in (0, 1, 2, 4)}
    graphs.update({
        'one_model': (graph_of(lambda: estimate_poses(params, d1, d2, offsets=offsets, models=first, px_thr=PX_THR,
                                                      out=one), CALLS), CALLS),
        'models_768': (graph_of(lambda: estimate_poses(params, d1, d2, offsets=offsets, models=kept, px_thr=PX_THR,
                                                       out=routed), CALLS), CALLS),
        'hr_r0': (graph_of(lambda: hcall(0, out=hout[0]), CALLS), CALLS),
        'hr_r2': (graph_of(lambda: hcall(2, out=hout[2]), CALLS), CALLS),
        'torch_16_pairs': (torch_graph, 1)})
    rec.update(measure(graphs))
    med = lambda k: rec[k + '_us']['median']
    tiles = (kept.shape[1] + 255) // 256
    tile_us = (med('models_768') - med('one_model')) / (tiles - 1)
    pose_share = med('one_model') - tile_us
    rec['k_pr_pose_share_us'], rec['k_pr_score_tile_us'] = pose_share, tile_us
    margin = max(0.03, *(spread(rec, k) for k in ('refit_0', 'one_model', 'models_768')))
    rec['same_run_margin'] = margin
    rec['refit_0_no_more_than_k_pr_pose'] = bool(med('refit_0') <= pose_share * (1.0 + margin))
    rec['round_us'] = {'first': med('refit_1') - med('refit_0'), 'two': med('refit_2') - med('refit_0'),
                       'four': med('refit_4') - med('refit_0')}
    rec['torch_scaled_us'] = med('torch_16_pairs') * n_pairs / n_torch
    rec['one_round_less_than_torch'] = bool(rec['round_us']['first'] < rec['torch_scaled_us'])
    rec['k_hr_finish_two_rounds_us'] = med('hr_r2') - med('hr_r0')
    rec['ratio_to_k_hr_finish'] = rec['round_us']['two'] / rec['k_hr_finish_two_rounds_us']
    rec['expected_ratio_to_k_hr_finish'] = EXPECTED_RATIO_TO_HR
    rec['pairs_per_s_4_rounds'] = n_pairs / (med('refit_4') * 1e-6)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'pose_refit_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--rows', type=int, default=2048)
    ap.add_argument('--shrink', type=int, default=1)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('pose_refit_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/pose_refit_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__,
           'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/pose_refit_probe.py', 'imagematching_oetr_amd/csrc/pose_refit.hip',
                                             'imagematching_oetr_amd/csrc/pose_refit_math.h',
                                             'tests/pose_refit_oracle.py')},
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
        'refit_iters 0 takes no more device time than k_pr_pose\'s share of oetr_pose_ransac (a)':
            'MET' if all(c['refit_0_no_more_than_k_pr_pose'] for c in rec['cells']) else 'MISSED',
        'one round takes less device time than its torch restatement (b)':
            'MET' if all(c['one_round_less_than_torch'] for c in rec['cells']) else 'MISSED',
        'two rounds cost about 1.5 x k_hr_finish\'s two (c): within 1.2 .. 1.8':
            'MET' if all(1.2 <= c['ratio_to_k_hr_finish'] <= 1.8 for c in rec['cells']) else 'MISSED'}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
