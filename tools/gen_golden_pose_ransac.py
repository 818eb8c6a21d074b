#!/usr/bin/env python
"""Write tests/pose_ransac_expected.json: the pinned call and the recorded scenes of the relative-pose specification
(tests/pose_ransac_oracle.py).

The inputs are a RECIPE of ``tests/pose_ransac_oracle.py`` (seeds, lengths, noise, outlier shares, the drawing used) -
they are regenerated from it, bit for bit (pinned by the hashes of the parameter blocks and the keypoints) - and the
recorded results are those of the float64 program in that module: per pinned ``n_hyp`` and list the five counters and
models, per-model counts, the selected model, pose, cosines and inliers by hash, and the margins.  The script draws
every pinned list again until no decision of it can be flipped by a last bit (every ``s * s`` at least 1e-6 relative
from its threshold product under every finite model, every cheirality depth at least 1e-9 from 0; the best two models
differ in count or tie exactly and resolve by number, by construction of the selection) and records the drawing and the
smallest margins.  The solver's own comparisons carry no margin.  It measures and records the solver's residuals on noise-free samples, draws the noise-free scenes until the pose error is below
0.01 degrees and the noisy ones until the selected model has at least the inliers of the true essential matrix (at
most 20 drawings each; the drawings and the errors are recorded; no scene is excluded).

Where the reference snapshot exists (``oracle/_ref/``, placed by ``build()`` and kept out of git) the script also loads
the REFERENCE's ``compute_pose_error`` and ``pose_auc`` and asserts that ``pose_errors`` equals the former on the
fixture's poses (the largest absolute difference is recorded and asserted at 8 x float64's rounding of an angle in
degrees near the clip) and ``pose_auc`` the latter on the fixture's errors (equality expected), and sets
``reference_checked``.  No estimator of the reference is run: it needs OpenCV, and no parity with it is claimed.

Usage:  python tools/gen_golden_pose_ransac.py [--out tests/pose_ransac_expected.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
REF = REPO / 'oracle' / '_ref'
sys.dont_write_bytecode = True
sys.path.insert(0, str(REPO / 'tests'))

import covis_oracle as cvo  # noqa: E402
import match_score_oracle as mso  # noqa: E402
import pose_ransac_oracle as pro  # noqa: E402

# |d arccos| near the clip: a cosine within one rounding (1.1e-16) of 1 moves the angle by sqrt(2 * 1.1e-16) rad =
# 8.5e-7 degrees; the reference forms the same cosine through np.dot / np.trace in another order.  8 x that.
REFERENCE_BOUND_DEG = 8 * 8.5e-7


def reference_errors(ref, blocks, results):
    """The reference's compute_pose_error on the poses of ``results`` -> (err_R, err_t), inf without a pose."""
    _, evaluation = ref
    err_R, err_t = [], []
    for P, res in zip(blocks, results):
        if res['counts'][2] < 0 or not np.isfinite(res['pose']).all():
            err_R.append(np.inf), err_t.append(np.inf)
            continue
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = P[8:17].reshape(3, 3), P[17:20]
        et, eR = evaluation.compute_pose_error(T, res['pose'][:9].reshape(3, 3), res['pose'][9:])
        err_R.append(float(eR)), err_t.append(float(et))
    return np.array(err_R), np.array(err_t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'pose_ransac_expected.json'))
    args = ap.parse_args()
    have_reference = (REF / 'dloc' / 'evaluate' / 'utils' / 'evaluation.py').is_file()
    ref = mso.load_reference(REF) if have_reference else None

    blocks, lists, draws = pro.pinned_call()
    by_hyp, margins, all_results = {}, dict(threshold=np.inf, depth=np.inf), []
    for n in pro.PINNED_HYPOTHESES:
        results = pro.estimate_lists(blocks, lists, n, pro.PINNED_SEED)
        for res in results:
            assert pro.margins_hold(res)
            g = res['margins']
            if g:
                margins = dict(threshold=min(margins['threshold'], g['threshold']), depth=min(margins['depth'], g['depth']))
        by_hyp[str(n)] = [pro.list_record(r) for r in results]
        all_results.append(results)

    solver = [pro.solver_check(i) for i in range(pro.SOLVER_SCENES)]
    noise_free = []
    for i in range(pro.NOISE_FREE_SCENES):
        for d in range(pro.MAX_DRAWS):
            res = pro.estimate(*pro.noise_free_scene(i, d), 256, 0, 1.0, i)
            if pro.error_of(res) < pro.NOISE_FREE_BOUND_DEG:
                break
        assert pro.error_of(res) < pro.NOISE_FREE_BOUND_DEG, i
        noise_free.append(dict(draw=d, pose_error_deg=pro.error_of(res), counts=[int(c) for c in res['counts']]))
    noisy = []
    for i, share in pro.NOISY_SCENES:
        for d in range(pro.MAX_DRAWS):
            res, true_inliers = pro.noisy_result(i, share, d)
            if res['counts'][3] >= true_inliers:
                break
        assert res['counts'][3] >= true_inliers, (i, share)      # none is excluded after the cap
        noisy.append(dict(scene=i, outliers=share, draw=d, pose_error_deg=pro.error_of(res),
                          counts=[int(c) for c in res['counts']], true_inliers=true_inliers))

    observed = auc_equal = None
    if ref is not None:
        observed = 0.0
        for results in all_results:
            ours = pro.pose_errors(np.stack([r['cosines'] for r in results]), np.stack([r['counts'] for r in results]))
            theirs = reference_errors(ref, blocks, results)
            for a, b in zip(ours[:2], theirs):
                assert np.array_equal(np.isinf(a), np.isinf(b))
                fin = np.isfinite(a)
                observed = max(observed, float(np.abs(a[fin] - b[fin]).max()))
            if not hasattr(np, 'trapz'):                           # the reference calls np.trapz, gone from numpy 2
                np.trapz = np.trapezoid
            auc_ref = ref[0].pose_auc(ours[2], [5, 10, 20])
            auc_equal = [float(a) for a in auc_ref] == [float(a) for a in pro.pose_auc(ours[2], [5, 10, 20])]
            assert np.abs(np.array(auc_ref) - np.array(pro.pose_auc(ours[2], [5, 10, 20]))).max() <= 8 * 2.2e-16
        assert observed <= REFERENCE_BOUND_DEG, observed

    last = all_results[-1]
    errors = pro.pose_errors(np.stack([r['cosines'] for r in last]), np.stack([r['counts'] for r in last]))[2]
    out = dict(
        specification='tests/pose_ransac_oracle.py: the project\'s own statement; no parity with OpenCV is claimed',
        pinned=dict(seed=pro.PINNED_SEED, recipe=[list(r) for r in pro.PINNED], draws=draws,
                    blocks_sha256=cvo.sha(blocks),
                    kpts_sha256=[cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists],
                    n_hyp=by_hyp, margins=margins,
                    pose_error_deg_n257=[None if np.isinf(e) else float(e) for e in errors],
                    auc_n257=[float(a) for a in pro.pose_auc(errors)]),
        solver=dict(scenes=pro.SOLVER_SCENES, hypotheses=pro.SOLVER_HYPOTHESES,
                    residual=max(s[0] for s in solver), det=max(s[1] for s in solver),
                    nearest_root=max(s[2] for s in solver)),
        noise_free=noise_free, noisy_recipe=pro.NOISY, noisy=noisy,
        degenerate=dict(collinear_counts=[int(c) for c in pro.estimate(*pro.degenerate_lists()['collinear'], 16)['counts']]),
        reference_checked=bool(have_reference),
        reference_max_abs_diff_deg=observed, reference_auc_equal=auc_equal)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print('pinned draws', draws, 'margins', margins, 'solver', out['solver'])
    print('noise-free', [(s['draw'], '%.1e' % s['pose_error_deg']) for s in noise_free])
    print('noisy', [(s['draw'], s['counts'][3], s['true_inliers'], '%.2f' % s['pose_error_deg']) for s in noisy])
    print(('reference checked: max |error - compute_pose_error| = %.2e deg, AUC equal: %s' % (observed, auc_equal))
          if have_reference else 'specification only')


if __name__ == '__main__':
    main()
