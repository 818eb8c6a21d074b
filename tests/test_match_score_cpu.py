"""CPU checks of the match-scoring specification (``tests/match_score_oracle.py``): the float64
restatement reproduces the pinned lists (``tests/match_score_expected.json``), hand-checked matches and the special
rounding cases, and - where the reference snapshot exists - the reference's own ``compute_epipolar_error`` /
``get_episym`` / ``get_projected_kp`` + ``get_truesym``: every flag and counter identical, the values within 8x the
relative difference the fixture's generator recorded."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import match_score_oracle as mso  # noqa: E402
from oracle import ref_snapshot  # noqa: E402

EXPECTED = json.loads((REPO / 'tests' / 'match_score_expected.json').read_text())
needs_reference = pytest.mark.skipif(not (ref_snapshot.DEST / 'dloc' / 'evaluate' / 'utils' / 'evaluation.py').is_file(),
                                     reason='needs the reference snapshot that build() places in oracle/_ref/')


@pytest.fixture(scope='module')
def pinned():
    """(views, lists, restated results) of the fixture's recipe: computed once, shared, never modified."""
    views = mso.make_scene(tuple(tuple(s) for s in EXPECTED['sizes']), EXPECTED['seed'])
    lists = mso.make_lists(views, seed=EXPECTED['seed'])
    return views, lists, mso.score_lists(views, mso.PAIRS, lists, **EXPECTED['thresholds'])


# ------------------------------------------------------------------ the restatement and the pinned lists
def test_fixture_says_how_it_was_made():
    assert EXPECTED['reference_checked'] is True
    assert EXPECTED['threshold_margin'] >= mso.MIN_THRESHOLD_MARGIN and EXPECTED['tie_margin'] >= mso.MIN_TIE_MARGIN
    assert [tuple(p) for p in EXPECTED['pairs']] == list(mso.PAIRS) and tuple(EXPECTED['lengths']) == mso.LENGTHS
    assert set(EXPECTED['lengths']) == {0, 1, 63, 64, 65, 255, 256, 257, 600} and len(EXPECTED['pairs']) == 14
    assert EXPECTED['thresholds'] == mso.THRESHOLDS
    counts = np.array([rec['counts'] for rec in EXPECTED['lists']])
    assert (counts[:, 0] == mso.LENGTHS).all() and (counts >= 0).all()
    for col in range(1, 5):                     # every counter decides something somewhere
        assert 0 < counts[:, col].sum() < counts[:, 0].sum(), col


def test_restatement_reproduces_the_fixture(pinned):
    views, lists, results = pinned
    assert [cvo.sha(v['depth']) for v in views] == EXPECTED['depth_sha256']
    assert [cvo.sha(mso.pair_block(views, i, j)) for i, j in mso.PAIRS] == EXPECTED['params_sha256']
    assert [cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists] == EXPECTED['kpts_sha256']
    thr = tie = np.inf
    for p, (res, (k1, k2), rec) in enumerate(zip(results, lists, EXPECTED['lists'])):
        assert mso.list_record(res) == rec, p
        a, b = mso.margins(res, k1, k2, **EXPECTED['thresholds'])
        thr, tie = min(thr, a), min(tie, b)
    assert thr == EXPECTED['threshold_margin'] and tie == EXPECTED['tie_margin']


def test_restatement_on_hand_checked_matches():
    """Cameras a unit apart along x, identity rotation, f = 10: the epipolar lines are the rows.  A match on its row
    has zero error; one row off has s = dy / f, and the reference's UNSQUARED denominators make it a0 + a1 = -t0 = -1
    and b0 + b1 = +1: epi_ref = s^2 (1 / -1 + 1 / 1) = 0, while episym = s^2 (1 + 1)."""
    K = np.array([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]])
    T = np.eye(4)
    T[0, 3] = 1.0
    P = mso.param_block(K, K, T)
    depth = np.full((9, 9), 5.0, np.float32)
    depth[2, 2] = 0
    k1 = np.array([[4, 4], [4, 4], [2, 2], [4.5, 3.5], [-0.5, 8.49], [8.5, 4]], np.float32)
    k2 = np.array([[6, 4], [6, 5], [4, 2], [6.5, 3.5], [1.5, 8.49], [np.nan, 4]], np.float32)
    r = mso.score(depth, depth, P, k1, k2, 5e-4, 1e-4, 0.5)
    assert r['epi_ref'][0] == 0 and r['episym'][0] == 0 and r['reproj12_sq'][0] == 0 and r['reproj21_sq'][0] == 0
    assert r['epi_ref'][1] == 0 and r['episym'][1] == pytest.approx(2 * 0.1 ** 2, rel=1e-12)
    assert r['reproj12_sq'][1] == pytest.approx(1.0, rel=1e-12)
    assert r['flags'][0] == 31 and r['flags'][1] == 1 + 2 + 4                     # one px off: only epi_ref is fooled
    assert r['flags'][2] == 2 + 4 + 8 and np.isnan(r['reproj12_sq'][2])             # a hole under keypoint 1
    # (4.5, 3.5) reads pixel (4, 4): both halves go to the even neighbour; (-0.5, 8.49) reads (0, 8); 8.5 -> 8
    assert r['d1'].tolist() == [5, 5, 0, 5, 5, 5] and r['d2'].tolist() == [5, 5, 5, 5, 5, 0]
    assert r['flags'][5] == 1 and np.isnan(r['epi_ref'][5])                         # a NaN keypoint: no flag beyond depth 1
    assert r['counts'].tolist() == [6, 5, 4, 4, 3]
    off = mso.score(depth, depth, P, k1, k2, None, None, None)
    assert off['counts'].tolist() == [6, -1, -1, 4, -1] and (off['flags'] & 28 == 0).all()


def test_special_rows_are_what_they_claim():
    s = mso.special_points((40, 64))
    d = mso.depth_at(np.arange(40 * 64, dtype=np.float32).reshape(40, 64) + 1, s[:, 0].astype(np.float64), s[:, 1].astype(np.float64))
    inside = d != 0
    #        .5 ties (3)       -0.5  -0.51  W-.5   W-.49  inf    -inf   nan    y=inf  y=nan  y=-.5 H-.5   H-.49  tie
    assert inside.tolist() == [True, True, True, True, False, False, False, False, False, False, False, False, True, False, False, True]
    assert d[0] == 2 * 64 + 0 + 1 and d[1] == 0 * 64 + 2 + 1 and d[2] == 2 * 64 + 2 + 1       # (0.5, 1.5) -> (0, 2) ...
    odd = mso.special_points((7, 5))
    d = mso.depth_at(np.ones((7, 5), np.float32), odd[:, 0].astype(np.float64), odd[:, 1].astype(np.float64))
    assert d[5] == 1 and d[6] == 0 and d[13] == 1 and d[14] == 0      # W - 0.5 = 4.5 -> 4 inside, 4.51 -> 5 outside; H likewise


@needs_reference
def test_restatement_against_the_reference(pinned):
    views, lists, results = pinned
    before = {n: sys.modules.get(n) for n in ('cv2', 'skimage')}
    ref = mso.load_reference(ref_snapshot.DEST)
    assert {n: sys.modules.get(n) for n in before} == before               # the stand-ins are gone again
    recorded = EXPECTED['reference_max_rel_diff']
    for p, ((i, j), (k1, k2), mine) in enumerate(zip(mso.PAIRS, lists, results)):
        theirs = mso.reference_scores(ref, views[i]['depth'], views[j]['depth'], mso.pair_block(views, i, j), k1, k2,
                                      **EXPECTED['thresholds'])
        assert np.array_equal(theirs['flags'], mine['flags']), p
        assert np.array_equal(theirs['counts'], mine['counts']), (p, theirs['counts'], mine['counts'])
        n = int(mine['counts'][0])
        assert theirs['precision'] == (mine['counts'][1] / n if n else 0)
        for k in mso.VALUES:
            diff = mso.rel_diff(theirs[k], mine[k])
            print(p, k, diff)
            assert diff <= 8 * recorded[k], (p, k, diff, recorded[k])
