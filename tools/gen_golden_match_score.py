#!/usr/bin/env python
"""Write tests/match_score_expected.json: the pinned match lists of the match-scoring specification
(tests/match_score_oracle.py).

The lists are a RECIPE (sizes, seed, pair list, lengths) of ``tests/match_score_oracle.py`` - the inputs are regenerated
from it, bit for bit (pinned by the hashes of the depth maps, the parameter blocks and the keypoints) - and the recorded
results are those of the float64 restatement in that module: per list the five counters, and the flags and the four
per-match arrays by hash.  The script asserts the condition that makes counters and flags comparable across
implementations that differ in the last bit: every thresholded quantity is at least 1e-6 (relative) away from its
threshold, and every depth-test coordinate is exactly on a ``.5`` tie or at least 1e-3 away from one; the smallest
margins are recorded.

Where the reference snapshot exists (``oracle/_ref/``, placed by ``build()`` and kept out of git) the script also runs
the REFERENCE's ``compute_epipolar_error``, ``get_episym`` and ``get_projected_kp`` + ``get_truesym`` on every list and
asserts that (a) every flag and every counter is identical and (b) the per-match values agree to 1e-9 relative; the
largest observed relative difference is recorded (the reference multiplies through BLAS: no bit equality is claimed), and
``reference_checked`` says that this happened.  Without the snapshot the file is written from the restatement alone and
says so.

Usage:  python tools/gen_golden_match_score.py [--out tests/match_score_expected.json]
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

SEED = 0
REFERENCE_BOUND = 1e-9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'match_score_expected.json'))
    args = ap.parse_args()
    have_reference = (REF / 'dloc' / 'evaluate' / 'utils' / 'evaluation.py').is_file()
    ref = mso.load_reference(REF) if have_reference else None
    views = mso.make_scene(mso.SIZES, SEED)
    lists = mso.make_lists(views, seed=SEED)
    results = mso.score_lists(views, mso.PAIRS, lists, **mso.THRESHOLDS)
    thr_margin = tie_margin = np.inf
    observed = dict.fromkeys(mso.VALUES, 0.0)
    for p, ((i, j), (k1, k2), res) in enumerate(zip(mso.PAIRS, lists, results)):
        a, b = mso.margins(res, k1, k2, **mso.THRESHOLDS)
        thr_margin, tie_margin = min(thr_margin, a), min(tie_margin, b)
        if ref is not None:
            theirs = mso.reference_scores(ref, views[i]['depth'], views[j]['depth'], mso.pair_block(views, i, j), k1, k2,
                                          **mso.THRESHOLDS)
            assert np.array_equal(theirs['flags'], res['flags']), (p, 'flags')
            assert np.array_equal(theirs['counts'], res['counts']), (p, theirs['counts'], res['counts'])
            n = int(res['counts'][0])
            assert theirs['precision'] == (res['counts'][1] / n if n else 0), (p, 'precision')
            for k in mso.VALUES:
                observed[k] = max(observed[k], mso.rel_diff(theirs[k], res[k]))
    assert thr_margin >= mso.MIN_THRESHOLD_MARGIN and tie_margin >= mso.MIN_TIE_MARGIN, (thr_margin, tie_margin)
    assert all(v <= REFERENCE_BOUND for v in observed.values()), observed
    out = dict(
        sizes=[list(s) for s in mso.SIZES], seed=SEED, pairs=[list(p) for p in mso.PAIRS], lengths=list(mso.LENGTHS),
        thresholds=mso.THRESHOLDS,
        depth_sha256=[cvo.sha(v['depth']) for v in views],
        params_sha256=[cvo.sha(mso.pair_block(views, i, j)) for i, j in mso.PAIRS],
        kpts_sha256=[cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists],
        lists=[mso.list_record(r) for r in results],
        threshold_margin=thr_margin, tie_margin=tie_margin,
        reference_checked=bool(have_reference),
        reference_max_rel_diff=observed if have_reference else None)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print('lists', len(lists), 'matches', sum(mso.LENGTHS), 'counts', [r['counts'].tolist() for r in results][:4], '...',
          'threshold margin %.2e tie margin %.2e' % (thr_margin, tie_margin),
          ('reference checked, max rel diff %s' % observed) if have_reference else 'restatement only')


if __name__ == '__main__':
    main()
