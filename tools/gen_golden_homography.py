#!/usr/bin/env python
"""Write tests/homography_expected.json: the pinned match lists and overlap boxes of the homography specification
(tests/homography_oracle.py).

The inputs are a RECIPE (seed, sizes, lengths, kinds) of ``tests/homography_oracle.py`` - they are regenerated from it,
bit for bit (pinned by the hashes of the homographies and the keypoints) - and the recorded results are those of the
float64 restatement in that module: per list the ``1 + 15`` counters and ``dist_sq`` by hash, per pair of pictures the
boxes, ``valid`` and the count.  The script asserts the conditions that make counters and boxes comparable across
implementations that differ in the last bit: every finite ``dist_sq`` is at least 1e-6 (relative) away from every
``thr * thr``, and every box's decision margin (``.5`` ties of the landing coordinates, ``a2`` against 0) is at least
1e-9; the smallest margins are recorded.

Where the reference snapshot exists (``oracle/_ref/``, placed by ``build()`` and kept out of git) the script also runs
the REFERENCE's ``h_evaluate`` on every non-empty list - ``kpts0`` / ``kpts1`` float32 torch tensors and ``H`` float64,
as its loader passes them - and asserts that (a) every counter equals ``np.sum(dist <= thr)`` of the reference's
distances, (b) ``|sqrt(dist_sq) - dist| <= 1e-9`` px on every row whose projected coordinates stay below 1e4 in
magnitude (a thousand times float64 rounding at that magnitude; the reference multiplies through ``np.dot``: no bit
equality is claimed) and (c) the rows of the deliberately degenerate lists (``a2 == 0``, NaN in ``H``) are non-finite
on both sides or on neither.  The largest observed difference is recorded, and ``reference_checked`` says that this
happened.  Without the snapshot the file is written from the restatement alone and says so.  The reference has no
overlap boxes under a homography: the boxes are the project's own statement and are recorded as such.

Usage:  python tools/gen_golden_homography.py [--out tests/homography_expected.json]
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
import homography_oracle as ho  # noqa: E402
import match_score_oracle as mso  # noqa: E402

SEED = 0
REFERENCE_BOUND_PX = 1e-9
REFERENCE_MAX_COORD = 1e4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'homography_expected.json'))
    args = ap.parse_args()
    have_reference = (REF / 'dloc' / 'evaluate' / 'utils' / 'evaluation.py').is_file()
    ref = mso.load_reference(REF) if have_reference else None
    lists = ho.make_lists(SEED)
    results = [ho.score(e['H'], e['k1'], e['k2']) for e in lists]
    thr_margin, observed, compared = np.inf, 0.0, 0
    for p, (e, res) in enumerate(zip(lists, results)):
        thr_margin = min(thr_margin, ho.threshold_margin(res['dist_sq']))
        if ref is None or not len(e['k1']):
            continue
        dist = ho.reference_distances(ref, e['H'], e['k1'], e['k2'])
        with np.errstate(all='ignore'):
            theirs = [len(dist)] + [int(np.sum(dist <= thr)) for thr in ho.THRESHOLDS]
            assert theirs == res['counts'].tolist(), (p, e['kind'], theirs, res['counts'].tolist())      # (a)
            ours = np.sqrt(res['dist_sq'])
            assert np.array_equal(np.isfinite(ours), np.isfinite(dist)), (p, e['kind'], 'finite')         # (c)
            rows = np.isfinite(ours) & (np.abs(res['pu']) < REFERENCE_MAX_COORD) & (np.abs(res['pv']) < REFERENCE_MAX_COORD)
        if rows.any():
            observed = max(observed, float(np.abs(ours[rows] - dist[rows]).max()))                        # (b)
            compared += int(rows.sum())
    assert thr_margin >= mso.MIN_THRESHOLD_MARGIN, thr_margin
    assert observed <= REFERENCE_BOUND_PX, observed
    degenerate = {e['kind']: int((~np.isfinite(r['dist_sq'])).sum()) for e, r in zip(lists, results)
                  if e['kind'] in ho.DEGENERATE}
    assert degenerate == {'a2_zero': 4, 'nan_H': 64}, degenerate

    boxes = ho.make_boxes(SEED)
    box_margin = min(b['res']['margin'] for b in boxes)
    assert box_margin >= cvo.MIN_MARGIN, box_margin

    out = dict(
        seed=SEED, thresholds=list(ho.THRESHOLDS),
        list_sizes=[list(s) for s in ho.LIST_SIZES], list_kinds=list(ho.LIST_KINDS) + list(ho.DEGENERATE),
        lengths=[len(e['k1']) for e in lists],
        list_H_sha256=[cvo.sha(e['H']) for e in lists],
        kpts_sha256=[cvo.sha(np.concatenate([e['k1'], e['k2']])) for e in lists],
        lists=[ho.list_record(r) for r in results],
        threshold_margin=thr_margin,
        box_kinds=list(ho.KINDS), box_sizes=[[list(a), list(b)] for a, b in ho.BOX_SIZES],
        box_H_sha256=[cvo.sha(b['H']) for b in boxes],
        boxes=[ho.box_record(b['res']) for b in boxes],
        box_margin=box_margin,
        boxes_are='the project\'s own statement (numpy_overlap_box with the warp replaced by H): the reference has none',
        reference_checked=bool(have_reference),
        reference_rows_compared=compared if have_reference else None,
        reference_max_abs_diff_px=observed if have_reference else None)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print('lists', len(lists), 'matches', sum(out['lengths']), 'boxes', len(boxes),
          'threshold margin %.2e box margin %.2e' % (thr_margin, box_margin),
          ('reference checked on %d rows, max |sqrt(dist_sq) - dist| = %.2e px' % (compared, observed))
          if have_reference else 'restatement only')


if __name__ == '__main__':
    main()
