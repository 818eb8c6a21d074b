#!/usr/bin/env python
"""Write tests/pose_refit_expected.json: the pinned call and the recorded scenes of the pose-refit specification
(tests/pose_refit_oracle.py).

The inputs are a RECIPE of ``tests/pose_refit_oracle.py`` (seeds, lengths, noise, outlier shares, the drawing used) -
they are regenerated from it, bit for bit (pinned by the hashes of the parameter blocks, the keypoints and the two
sets of ``model_in``) - and the recorded results are those of the float64 program in that module: per source of
``model_in`` (``pose_ransac_oracle.estimate`` at ``n_hyp`` 85, the true essential matrix), per ``refit_iters`` and
list the five counters, every round's candidate count, and the model, pose, cosines, inliers and candidates by hash,
and the margins.  The script draws every pinned list again until no decision of it can be flipped by a last bit (every
``s * s`` of ``model_in`` and of every candidate at least 1e-6 relative from its threshold product, every cheirality
depth at least 1e-9 from 0) and records the drawing and the smallest margins.  The elimination's own comparisons and
the choice of the held entry carry no margin: they rest on equal bits, which the tests assert on the candidates.

It also records, without gating anything: the noise-free scenes (pose error before and after the refit; the largest
error after it is the value the CPU test asserts 8 x of), the twelve noisy scenes at ``px_thr`` 1 (per ``refit_iters``
the counts, the true essential matrix's count under the same test and the pose error) and the refusals and edges.

Usage:  python tools/gen_golden_pose_refit.py [--out tests/pose_refit_expected.json]
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
import pose_ransac_oracle as pro  # noqa: E402
import pose_refit_oracle as pfo  # noqa: E402


def errors_of(results):
    e = pro.pose_errors(np.stack([r['cosines'] for r in results]), np.stack([r['counts'] for r in results]))[2]
    return [None if np.isinf(v) else float(v) for v in e], [float(a) for a in pro.pose_auc(e)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'pose_refit_expected.json'))
    args = ap.parse_args()

    blocks, lists, models, draws = pfo.pinned_call()
    records, margins, summaries = {}, dict(threshold=np.inf, depth=np.inf), {}
    for source in pfo.PINNED_SOURCES:
        records[source], summaries[source] = {}, {}
        for r in pfo.PINNED_REFITS:
            results = pfo.refit_lists(blocks, lists, models[source], 1.0, r)
            for res in results:
                assert pfo.margins_hold(res)
                for k in margins:
                    margins[k] = min(margins[k], res['margins'].get(k, np.inf))
            records[source][str(r)] = [pfo.list_record(res) for res in results]
            err, auc = errors_of(results)
            summaries[source][str(r)] = dict(pose_error_deg=err, auc=auc)

    noise_free = []
    for i in range(pfo.NOISE_FREE['scenes']):
        est, res = pfo.noise_free_result(i)
        noise_free.append(dict(counts_estimate=[int(c) for c in est['counts']], counts=[int(c) for c in res['counts']],
                               pose_error_deg_minimal=pro.error_of(est), pose_error_deg=pfo.error_of(res)))
    noisy = []
    for i, share in pro.NOISY_SCENES:
        est, by_iters, true_inliers = pfo.noisy_results(i, share)
        noisy.append(dict(scene=i, outliers=share, true_inliers=true_inliers, pose_error_deg_minimal=pro.error_of(est),
                          rounds={str(r): dict(counts=[int(c) for c in res['counts']],
                                               candidate_counts=[int(c) for c in res['candidate_counts']],
                                               pose_error_deg=pfo.error_of(res)) for r, res in by_iters.items()}))
    edges = {}
    for name, (P, k1, k2, M, thr) in pfo.edge_cases().items():
        res = pfo.refit(P, k1, k2, M, thr, pfo.DEFAULT_REFIT)
        edges[name] = dict(counts=[int(c) for c in res['counts']],
                           candidate_counts=[int(c) for c in res['candidate_counts']])

    out = dict(
        specification='tests/pose_refit_oracle.py: the project\'s own statement; no parity with OpenCV is claimed',
        pinned=dict(seed=pfo.PINNED_SEED, n_hyp=pfo.PINNED_HYPOTHESES, recipe=[list(r) for r in pfo.PINNED], draws=draws,
                    refit_iters=list(pfo.PINNED_REFITS), blocks_sha256=cvo.sha(blocks),
                    kpts_sha256=[cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists],
                    models_sha256={s: cvo.sha(np.nan_to_num(models[s], nan=-7.0)) for s in pfo.PINNED_SOURCES},
                    records=records, summaries=summaries, margins=margins),
        noise_free_recipe=pfo.NOISE_FREE, noise_free=noise_free,
        noise_free_pose_error_deg=max(s['pose_error_deg'] for s in noise_free),
        noisy_recipe=pfo.NOISY, noisy=noisy, edges=edges)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print('pinned draws', draws, 'margins', margins)
    for s in pfo.PINNED_SOURCES:
        print(s, 'accepted/gained at 4 rounds', [(r['counts'][2], r['counts'][3] - r['counts'][1])
                                                  for r in records[s]['4']], 'auc', summaries[s]['0']['auc'],
              '->', summaries[s]['4']['auc'])
    print('noise-free', [('%.1e' % s['pose_error_deg_minimal'], '%.1e' % s['pose_error_deg']) for s in noise_free])
    for s in noisy:
        print('noisy', s['scene'], s['outliers'], 'true', s['true_inliers'], '%.2f' % s['pose_error_deg_minimal'],
              [(r, v['counts'][1], v['counts'][3], '%.2f' % v['pose_error_deg']) for r, v in s['rounds'].items()])
    print('edges', edges)


if __name__ == '__main__':
    main()
