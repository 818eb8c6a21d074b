#!/usr/bin/env python
"""Write tests/keypoint_score_expected.json: the pinned keypoint sets of the keypoint-repeatability specification
(tests/keypoint_score_oracle.py).

The sets are a RECIPE (the scene of tests/match_score_oracle.py, keypoint counts per view, seeds) - the inputs are
regenerated from it, bit for bit (pinned by the hashes of the depth maps, the parameter blocks and the keypoints) - and
the recorded results are those of the float64 restatement: per pair and direction the ``2 + T`` counters, and ``nearest``
and ``dist_sq`` by hash.  A set is re-drawn until the condition holds that makes the counters comparable across
implementations that differ in the last bit: every ``dist_sq`` is at least 1e-6 (relative) away from every ``th * th``,
and every depth-look-up coordinate is exactly on a ``.5`` tie or at least 1e-3 away from one; the seeds that were used
and the smallest margins are recorded.  No row is excluded.

Where the reference snapshot exists (``oracle/_ref/``, placed by ``build()`` and kept out of git) the script also runs
the REFERENCE's ``get_projected_kp`` / ``unnormalize_keypoints`` / ``get_repeatability`` on the same sets (the target
keypoints with a non-finite coordinate removed: the specification's departure) and asserts that the kept rows and every
counter are identical; the largest relative difference of the minima is recorded (the reference goes through BLAS and
``cdist``: no bit equality is claimed) - over the pairs ``i != j``; the minima of a SELF pair are rounding residues (0, or
some 1e-29), of which the largest absolute difference of the distances in pixels is recorded instead - and
``reference_checked`` says that this happened.  Without the snapshot the file
is written from the restatement alone and says so.

Usage:  python tools/gen_golden_keypoint_score.py [--out tests/keypoint_score_expected.json]
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
import keypoint_score_oracle as kso  # noqa: E402
import match_score_oracle as mso  # noqa: E402

SEED = 0
FIRST_KEYPOINT_SEED = 100
REFERENCE_BOUND = 1e-9           # relative, pairs i != j
REFERENCE_SELF_BOUND_PX = 1e-9   # pixels, self pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'keypoint_score_expected.json'))
    args = ap.parse_args()
    have_reference = (REF / 'dloc' / 'evaluate' / 'utils' / 'evaluation.py').is_file()
    ref = mso.load_reference(REF) if have_reference else None
    views = mso.make_scene(mso.SIZES, SEED)
    sets, thr_margin, tie_margin, observed, observed_px = [], np.inf, np.inf, 0.0, 0.0
    for s, counts in enumerate(kso.COUNTS):
        kps, seed, results, (thr, tie) = kso.draw_set(views, counts, FIRST_KEYPOINT_SEED + s)
        thr_margin, tie_margin = min(thr_margin, thr), min(tie_margin, tie)
        if ref is not None:
            rel, px = kso.reference_diffs(ref, views, kps, results)
            observed, observed_px = max(observed, rel), max(observed_px, px)
        sets.append(dict(counts=list(counts), seed=seed, kpts_sha256=[cvo.sha(k) for k in kps],
                         pairs=[kso.pair_record(r) for r in results]))
    assert thr_margin >= kso.MIN_THRESHOLD_MARGIN and tie_margin >= kso.MIN_TIE_MARGIN, (thr_margin, tie_margin)
    assert observed <= REFERENCE_BOUND and observed_px <= REFERENCE_SELF_BOUND_PX, (observed, observed_px)
    out = dict(
        sizes=[list(s) for s in mso.SIZES], seed=SEED, pairs=[list(p) for p in kso.PAIRS], thresholds=list(kso.THRESHOLDS),
        depth_sha256=[cvo.sha(v['depth']) for v in views],
        params_sha256=[cvo.sha(mso.pair_block(views, i, j)) for i, j in kso.PAIRS],
        sets=sets, threshold_margin=thr_margin, tie_margin=tie_margin,
        reference_checked=bool(have_reference), reference_max_rel_diff=observed if have_reference else None,
        reference_self_max_abs_diff_px=observed_px if have_reference else None)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print('sets', len(sets), 'pairs', len(kso.PAIRS), 'seeds', [s['seed'] for s in sets],
          'threshold margin %.2e tie margin %.2e' % (thr_margin, tie_margin),
          ('reference checked, max rel diff %.3e, self pairs %.3e px' % (observed, observed_px)) if have_reference else 'restatement only')


if __name__ == '__main__':
    main()
