#!/usr/bin/env python
"""Write tests/covis_set_expected.json: the pinned depth-map sets of the set extension (include/oetr_covis_set.h).

Each set is a RECIPE (sizes, seed) of ``tests/covis_set_oracle.py`` - the inputs are regenerated from it, bit for
bit (pinned by the hashes of the depth maps and of the cameras) - and the recorded results are those of the float64
restatement in that module over ALL ordered pairs: boxes, valid, count, ``scale_diff`` and the list of pairs the
mining criterion keeps at threshold 2.  Where the reference snapshot exists (``oracle/_ref/``, placed by ``build()``
and kept out of git) this script also runs the REFERENCE's ``numpy_overlap_box`` and ``scale_diff`` on every pair of
the sets whose maps share one square size - where parity with the reference is claimed - and asserts that they give
exactly the same boxes, counts, scale differences and keep decisions.  Without the snapshot the file is written from
the restatement alone (it holds the project's own numbers either way).

Usage:  python tools/gen_golden_covis_set.py [--out tests/covis_set_expected.json]
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

import covis_set_oracle as cso  # noqa: E402

SETS = (dict(name='mixed', sizes=[list(s) for s in cso.SIZES], seed=0),
        dict(name='square', sizes=[[56, 56]] * 4, seed=5))
MIN_SCALE_DIFF = 2.0


def check_against_reference(views, results):
    numpy_overlap_box, ref_scale_diff = cso.load_reference(REF)
    for (i, j), mine in results.items():
        theirs = cso.reference_pair(numpy_overlap_box, views, i, j)
        assert np.array_equal(theirs['box1'], mine['box1']) and np.array_equal(theirs['box2'], mine['box2']), (i, j)
        assert theirs['valid'] == mine['valid'] and theirs['count'] == mine['count'], (i, j)
        with np.errstate(all='ignore'):
            sd = ref_scale_diff(theirs['box1'], theirs['box2'], views[i]['depth'], views[j]['depth'])
            ref_keep = bool(theirs['valid'] and (theirs['box1'].max() > 0 and theirs['box2'].max() > 0 and sd > MIN_SCALE_DIFF))
        assert repr(float(sd)) == repr(float(cso.scale_diff(mine['box1'], mine['box2']))), (i, j, sd)
        assert ref_keep == cso.keep(mine['box1'], mine['box2'], mine['valid'], MIN_SCALE_DIFF), (i, j)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'covis_set_expected.json'))
    args = ap.parse_args()
    have_reference = (REF / 'src' / 'datasets' / 'utils.py').is_file()
    out = []
    for recipe in SETS:
        views, results = cso.checked_set(tuple(tuple(s) for s in recipe['sizes']), recipe['seed'])
        square = len({tuple(s) for s in recipe['sizes']}) == 1 and recipe['sizes'][0][0] == recipe['sizes'][0][1]
        if square and have_reference:
            check_against_reference(views, results)
        rec = dict(recipe, min_scale_diff=MIN_SCALE_DIFF, **cso.set_record(views, results, MIN_SCALE_DIFF))
        out.append(rec)
        print(recipe['name'], 'valid', sum(rec['valid']), 'of', len(rec['valid']), 'kept', rec['kept'],
              'margin %.2e' % min(r['margin'] for r in results.values()),
              'reference checked' if square and have_reference else 'restatement only')
    Path(args.out).write_text(json.dumps({'sets': out}, indent=1) + '\n')


if __name__ == '__main__':
    main()
