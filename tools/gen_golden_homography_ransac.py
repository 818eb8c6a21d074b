#!/usr/bin/env python
"""Write tests/homography_ransac_expected.json: the pinned call and the recorded scenes of the homography
specification (tests/homography_ransac_oracle.py).

The inputs are a RECIPE of ``tests/homography_ransac_oracle.py`` (seeds, lengths, noise, outlier shares, the drawing
used) - they are regenerated from it, bit for bit (pinned by the hashes of the parameter blocks and the keypoints) - and
the recorded results are those of the float64 program in that module: per pinned ``n_hyp``, ``refit_iters`` and list
the six counters and the models, per-model counts, the selected and the delivered model, ``H``, ``corner_sq`` and
inliers by hash, and the margins.  The script draws every pinned list again until no decision of it can be flipped by a
last bit - every inlier comparison of every finite model and of every refit candidate at least 1e-6 relative from its
threshold product, every ``a2`` of a row that passes the distance test at least 1e-6 relative from 0; the acceptance
comparisons are between integers that rest on those - and records the drawing and the smallest margins.  The solver's
and the elimination's own comparisons carry no margin: they rest on equal bits, which the GPU tests assert on the
models.

It also measures and records: the residual of the minimal models on their own samples (noise-free); the mean corner
error after the refit on noise-free scenes with 50 % outliers at ``px_thr`` 0.01; and twelve noisy scenes, drawn until
the delivered model has at least the inliers of ``H_gt`` scored by the same function (at most 20 drawings each; the
drawing and the corner errors before and after the refit are recorded; no scene is excluded).

No estimator of the reference is run: it needs skimage or OpenCV, and no parity with them is claimed.

Usage:  python tools/gen_golden_homography_ransac.py [--out tests/homography_ransac_expected.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.dont_write_bytecode = True
sys.path.insert(0, str(REPO / 'tests'))

import covis_oracle as cvo  # noqa: E402
import homography_ransac_oracle as hro  # noqa: E402


def compact(obj, depth=0, width=420):
    """JSON with every value that fits in ``width`` characters on one line: one line per recorded list keeps the 240
    records of the pinned call readable and the file small."""
    flat = json.dumps(obj)
    if not isinstance(obj, (dict, list)) or len(flat) <= width:
        return flat
    pad = ' ' * (depth + 1)
    if isinstance(obj, dict):
        body = [f'{pad}{json.dumps(k)}: {compact(v, depth + 1, width)}' for k, v in obj.items()]
        return '{\n' + ',\n'.join(body) + '\n' + ' ' * depth + '}'
    return '[\n' + ',\n'.join(pad + compact(v, depth + 1, width) for v in obj) + '\n' + ' ' * depth + ']'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'homography_ransac_expected.json'))
    args = ap.parse_args()

    blocks, lists, draws = hro.pinned_call()
    records, margins = {}, dict(threshold=np.inf, positive=np.inf)
    for n in hro.PINNED_HYPOTHESES:
        records[str(n)] = {}
        for r in hro.PINNED_REFITS:
            results = hro.estimate_lists(blocks, lists, n, hro.PINNED_SEED, hro.PINNED_THR, r)
            for res in results:
                assert hro.margins_hold(res)
                g = res['margins']
                if g:
                    margins = dict(threshold=min(margins['threshold'], g['threshold']),
                                   positive=min(margins['positive'], g['positive']))
            records[str(n)][str(r)] = [hro.list_record(res) for res in results]
    last = hro.estimate_lists(blocks, lists, hro.PINNED_HYPOTHESES[-1], hro.PINNED_SEED, hro.PINNED_THR, 2)
    errors = hro.homography_errors(np.stack([r['corner_sq'] for r in last]), np.stack([r['counts'] for r in last]))

    minimal = max(hro.minimal_check(i) for i in range(hro.MINIMAL_SCENES))
    noise_free = []
    for i in range(hro.NOISE_FREE_SCENES):
        res = hro.noise_free_result(i)
        noise_free.append(dict(corner_error_px=hro.mean_corner_error(res), counts=[int(c) for c in res['counts']]))
    noisy = []
    for i, share in hro.NOISY_SCENES:
        for d in range(hro.MAX_DRAWS):
            res, true_inliers = hro.noisy_result(i, share, d)
            if res['counts'][4] >= true_inliers:
                break
        assert res['counts'][4] >= true_inliers, (i, share)      # none is excluded after the cap
        before, _ = hro.noisy_result(i, share, d, refit_iters=0)
        noisy.append(dict(scene=i, outliers=share, draw=d, counts=[int(c) for c in res['counts']],
                          true_inliers=true_inliers, corner_error_px_minimal=hro.mean_corner_error(before),
                          corner_error_px=hro.mean_corner_error(res)))
    degenerate = {k: [int(c) for c in hro.estimate(P, k1, k2, 16, 0, hro.PINNED_THR, 2, 0)['counts']]
                  for k, (P, k1, k2) in hro.degenerate_lists().items()}
    refit = {}
    for k, (P, k1, k2, M, thr) in hro.refit_cases().items():
        res = hro.estimate(P, k1, k2, px_thr=thr, models=M)
        refit[k] = dict(counts=[int(c) for c in res['counts']], acceptances=res['margins']['acceptances'])

    out = dict(
        specification='tests/homography_ransac_oracle.py: the project\'s own statement; no parity with skimage or '
                      'OpenCV is claimed',
        pinned=dict(seed=hro.PINNED_SEED, px_thr=hro.PINNED_THR, recipe=[list(r) for r in hro.PINNED], draws=draws,
                    blocks_sha256=cvo.sha(blocks),
                    kpts_sha256=[cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists],
                    n_hyp=records, margins=margins,
                    corner_error_px_n600_r2=[None if np.isinf(e) else float(e) for e in errors],
                    auc_n600_r2=[float(a) for a in hro.homography_auc(errors)]),
        minimal=dict(scenes=hro.MINIMAL_SCENES, hypotheses=hro.MINIMAL_HYPOTHESES, residual=minimal),
        noise_free_recipe=hro.NOISE_FREE, noise_free=noise_free,
        noise_free_corner_error_px=max(s['corner_error_px'] for s in noise_free),
        noisy_recipe=hro.NOISY, noisy=noisy, degenerate=degenerate, refit=refit)
    text = compact(out)
    assert json.loads(text) == out
    Path(args.out).write_text(text + '\n')
    print('pinned draws', draws, 'margins', margins, 'minimal residual', minimal)
    print('noise-free', ['%.1e' % s['corner_error_px'] for s in noise_free])
    print('noisy', [(s['draw'], s['counts'][3], s['counts'][4], s['true_inliers'],
                     '%.2f -> %.2f' % (s['corner_error_px_minimal'], s['corner_error_px'])) for s in noisy])
    print('degenerate', degenerate, 'refit', refit)


if __name__ == '__main__':
    main()
