"""CPU checks of the keypoint-repeatability specification (``tests/keypoint_score_oracle.py``): the
float64 restatement reproduces the pinned sets (``tests/keypoint_score_expected.json``), hand-computed cases and the
kept quirks of the reference (no lower bound on the projection, negative and NaN depth counted as depth), its two
departures (an empty picture, non-finite targets), the tie rule, and - where the reference snapshot exists - the
reference's own ``get_projected_kp`` / ``unnormalize_keypoints`` / ``get_repeatability``: kept rows and every counter
identical, the minima within 8x the difference the fixture's generator recorded."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import keypoint_score_oracle as kso  # noqa: E402
import match_score_oracle as mso  # noqa: E402
from oracle import ref_snapshot  # noqa: E402

EXPECTED = json.loads((REPO / 'tests' / 'keypoint_score_expected.json').read_text())
needs_reference = pytest.mark.skipif(not (ref_snapshot.DEST / 'dloc' / 'evaluate' / 'utils' / 'evaluation.py').is_file(),
                                     reason='needs the reference snapshot that build() places in oracle/_ref/')


@pytest.fixture(scope='module')
def pinned():
    """(views, [(keypoint sets, restated results) per pinned set]) of the fixture's recipe: computed once, shared."""
    views = mso.make_scene(tuple(tuple(s) for s in EXPECTED['sizes']), EXPECTED['seed'])
    sets = []
    for rec in EXPECTED['sets']:
        kps = kso.make_keypoints(views, rec['counts'], rec['seed'])
        sets.append((kps, kso.score_pairs(views, kps, thresholds=EXPECTED['thresholds'])))
    return views, sets


def simple_pair():
    """Cameras a unit apart along x, identity rotation, f = 10, depth 5 everywhere: a keypoint of picture 1 appears
    10 * 1 / 5 = 2 px to the right in picture 2."""
    K = np.array([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]])
    T = np.eye(4)
    T[0, 3] = 1.0
    return mso.param_block(K, K, T), np.full((9, 9), 5.0, np.float32)


# ------------------------------------------------------------------ the restatement and the pinned sets
def test_fixture_says_how_it_was_made():
    assert EXPECTED['reference_checked'] is True
    assert EXPECTED['threshold_margin'] >= kso.MIN_THRESHOLD_MARGIN and EXPECTED['tie_margin'] >= kso.MIN_TIE_MARGIN
    assert [tuple(p) for p in EXPECTED['pairs']] == list(kso.PAIRS) and len(kso.PAIRS) == 16
    assert sum(i == j for i, j in kso.PAIRS) == 4 and set(kso.PAIRS) == {(i, j) for i in range(4) for j in range(4)}
    assert tuple(EXPECTED['thresholds']) == kso.THRESHOLDS == (1.0, 2.0, 3.0, 5.0)
    assert [tuple(s) for s in EXPECTED['sizes']] == [(1, 1), (7, 5), (40, 64), (56, 56)]
    assert tuple(tuple(s['counts']) for s in EXPECTED['sets']) == kso.COUNTS
    assert {n for s in EXPECTED['sets'] for n in s['counts']} == {0, 1, 63, 64, 65, 255, 256, 257, 600}
    counts = np.array([p['counts'] for s in EXPECTED['sets'] for p in s['pairs']])
    assert counts.shape == (48, 2, 6) and (counts >= 0).all()
    assert 0 < counts[:, :, 1].sum() < counts[:, :, 0].sum()                   # some rows are kept, some are not
    for col in range(2, 6):                                                   # every threshold decides something
        assert 0 < counts[:, :, col].sum() < counts[:, :, 1].sum(), col
    assert (np.diff(counts[:, :, 2:], axis=2) >= 0).all() and (counts[:, :, 5] <= counts[:, :, 1]).all()


def test_restatement_reproduces_the_fixture(pinned):
    views, sets = pinned
    assert [cvo.sha(v['depth']) for v in views] == EXPECTED['depth_sha256']
    assert [cvo.sha(mso.pair_block(views, i, j)) for i, j in kso.PAIRS] == EXPECTED['params_sha256']
    thr = tie = np.inf
    for (kps, results), rec in zip(sets, EXPECTED['sets']):
        assert [len(k) for k in kps] == rec['counts'] and all(k.dtype == np.float32 for k in kps)
        assert [cvo.sha(k) for k in kps] == rec['kpts_sha256']
        for p, (res, want) in enumerate(zip(results, rec['pairs'])):
            assert kso.pair_record(res) == want, (rec['counts'], p)
        a, b = kso.set_margins(results, kps, thresholds=EXPECTED['thresholds'])
        thr, tie = min(thr, a), min(tie, b)
        # drawn with the first seed that keeps the margins: the recorded seed is what draw_set arrives at
        assert kso.draw_set(views, rec['counts'], rec['seed'])[1] == rec['seed']
    assert thr == EXPECTED['threshold_margin'] and tie == EXPECTED['tie_margin']


def test_pinned_sets_hold_what_they_claim(pinned):
    """Duplicated rows, special rows, exact ties between two targets that resolve to the lower index, +inf minima."""
    views, sets = pinned
    tied = infinite = 0
    for kps, results in sets:
        for k, kp in enumerate(kps):
            if len(kp) >= kso.SPECIAL_FROM:
                assert np.array_equal(kp[10], kp[3]) and np.array_equal(kp[40], kp[7]) and np.array_equal(kp[41], kp[7])
                assert mso.equal_bits(kp[-16:], mso.special_points(views[k]['depth'].shape))
        for (i, j), pair in zip(kso.PAIRS, results):
            for res, dst in zip(pair, (kps[j], kps[i])):
                near = res['nearest'][res['kept']]
                assert not np.isin(near, (10, 40, 41)).any() or len(dst) < kso.SPECIAL_FROM    # the lower index won
                tied += int(np.isin(near, (3, 7)).sum()) if len(dst) >= kso.SPECIAL_FROM else 0
                assert (near < len(dst)).all() and np.isfinite(dst[near[near >= 0]]).all()     # never a non-finite one
                infinite += int(np.isinf(res['dist_sq']).sum())
                assert np.isnan(res['dist_sq'][~res['kept']]).all() and (res['nearest'][~res['kept']] == -1).all()
    assert tied > 20 and infinite > 20


def test_hand_computed_pair():
    P, depth = simple_pair()
    depth[2, 2] = 0
    kp1 = np.array([[4, 4], [2, 2], [1, 6], [8.4, 1], [0, 0]], np.float32)
    kp2 = np.array([[6, 4], [3, 9], [3, 6], [6, 5], [2, 0.5]], np.float32)
    a, b = kso.score(depth, depth, P, kp1, kp2, (1.0, 2.0))
    # 1 -> 2: (4,4) -> (6,4) exactly on kp2[0]; (2,2) is a hole; (1,6) -> (3,6) on kp2[2]; (8.4,1) -> (10.4,1) is outside
    # (pu >= W = 9); (0,0) -> (2,0), half a pixel from kp2[4]
    assert a['d'].tolist() == [5, 0, 5, 5, 5] and a['kept'].tolist() == [True, False, True, False, True]
    assert a['pu'][[0, 2, 4]].tolist() == [6, 3, 2] and a['pv'][[0, 2, 4]].tolist() == [4, 6, 0]
    assert a['nearest'].tolist() == [0, -1, 2, -1, 4] and a['dist_sq'][[0, 2, 4]].tolist() == [0, 0, 0.25]
    assert np.isnan(a['dist_sq'][[1, 3]]).all() and a['counts'].tolist() == [5, 3, 3, 3]
    # 2 -> 1: 2 px to the left.  (3,9) rounds to row 9: outside the 9 x 9 map, no depth; (6,5) -> (4,5), 1 px from (4,4):
    # not < 1, but < 2; (2,0.5) -> (0,0.5), 0.5 from (0,0)
    assert b['kept'].tolist() == [True, False, True, True, True] and b['nearest'].tolist() == [0, -1, 2, 0, 4]
    assert b['dist_sq'][[0, 2, 3, 4]].tolist() == [0, 0, 1, 0.25] and b['counts'].tolist() == [5, 4, 3, 4]
    assert kso.repeatability([a['counts'], b['counts']]).tolist() == [(3 / 3 + 3 / 4) / 2, (3 / 3 + 4 / 4) / 2]


def test_quirks_of_the_reference_are_kept():
    """No lower bound on the projection, no positive-depth test, a NaN depth counts as depth and its NaN projection
    fails both comparisons."""
    P, depth = simple_pair()
    depth[0, 1], depth[0, 2] = -5.0, np.nan
    kp1 = np.array([[0, 3], [1, 0], [2, 0]], np.float32)
    kp2 = np.array([[100, 100], [-2, 3]], np.float32)
    a, b = kso.score(depth, depth, P, kp1, kp2, (0.5, 3.0))
    # 1 -> 2 is pu = u + 10 / d.  (0,3) -> (2,3); (1,0) has the NEGATIVE depth -5 (no positive-depth test): x = -0.3,
    # X = 1.5, p0 = 2.5, p2 = -5 -> pu = 10 * (2.5 / -5) + 4 = -1: kept, there is NO lower bound; (2,0) has depth NaN
    assert a['d'][:2].tolist() == [5, -5] and np.isnan(a['d'][2])
    assert a['kept'].tolist() == [True, True, False] and a['pu'][1] == -1 and np.isnan(a['pu'][2])
    assert a['nearest'].tolist() == [1, 1, -1] and a['dist_sq'][:2].tolist() == [16, 10]
    assert a['counts'].tolist() == [3, 2, 0, 0]
    # 2 -> 1 is pu = u - 2: (-2,3) is outside its map (no depth), (100,100) likewise
    assert b['d'].tolist() == [0, 0] and b['counts'].tolist() == [2, 0, 0, 0]
    _, c = kso.score(depth, depth, P, kp1, np.array([[1, 3], [12.4, 3]], np.float32), (0.5,))
    assert c['d'].tolist() == [5, 0] and c['pu'][0] == -1 and c['kept'].tolist() == [True, False]
    # the upper bound is the TARGET map's: a 9 x 70 source, (60,3) -> (58,3), and 58 >= 9
    _, e = kso.score(depth, np.full((9, 70), 5.0, np.float32), P, kp1, np.array([[60, 3], [10, 3]], np.float32), (0.5,))
    assert e['pu'].tolist() == [58, 8] and e['kept'].tolist() == [False, True]


def test_empty_pictures_and_non_finite_targets():
    P, depth = simple_pair()
    kp1 = np.array([[4, 4], [1, 6]], np.float32)
    none = np.zeros((0, 2), np.float32)
    a, b = kso.score(depth, depth, P, kp1, none, (1.0,))
    assert a['nearest'].tolist() == [-1, -1] and np.isposinf(a['dist_sq']).all() and a['counts'].tolist() == [2, 2, 0]
    assert b['counts'].tolist() == [0, 0, 0] and b['nearest'].shape == (0,)
    assert kso.repeatability([a['counts'], b['counts']]).tolist() == [0.0]
    # non-finite targets never win - not even when they are all there is
    bad = np.array([[np.nan, 4], [6, np.inf], [-np.inf, np.nan]], np.float32)
    a, _ = kso.score(depth, depth, P, kp1, bad, (1.0,))
    assert a['nearest'].tolist() == [-1, -1] and np.isposinf(a['dist_sq']).all()
    mixed = np.concatenate([bad[:1], [[6.5, 4]], bad[1:], [[3, 6]]]).astype(np.float32)
    a, _ = kso.score(depth, depth, P, kp1, mixed, (1.0,))
    assert a['nearest'].tolist() == [1, 4] and a['dist_sq'].tolist() == [0.25, 0] and a['counts'].tolist() == [2, 2, 2]


def test_ties_resolve_to_the_lower_index():
    P, depth = simple_pair()
    kp1 = np.array([[4, 4]], np.float32)                             # lands on (6, 4)
    kp2 = np.array([[9, 9], [7, 4], [5, 4], [6, 5], [6, 3], [7, 4]], np.float32)    # four at distance 1, one twice
    a, b = kso.score(depth, depth, P, kp1, kp2, (1.0, 1.5))
    assert a['nearest'].tolist() == [1] and a['dist_sq'].tolist() == [1] and a['counts'].tolist() == [1, 1, 0, 1]
    # the other direction: duplicated SOURCE rows get the same answer
    assert b['nearest'][1] == b['nearest'][5] == 0 and b['dist_sq'][1] == b['dist_sq'][5] == 1
    near, dist = kso.nearest_neighbour(np.array([0.0]), np.array([0.0]), np.array([[3, 4], [-3, 4], [4, -3], [5, 0], [0, 5]]))
    assert near.tolist() == [0] and dist.tolist() == [25]


def test_padded_layout_and_repeatability():
    P, depth = simple_pair()
    kp1, kp2 = np.array([[4, 4], [1, 6]], np.float32), np.array([[6, 4]], np.float32)
    res = [kso.score(depth, depth, P, kp1, kp2, (1.0,))]
    counts, nearest, dist_sq = kso.padded(res, 3)
    assert counts.tolist() == [[[2, 2, 1], [1, 1, 1]]] and nearest.tolist() == [[[0, 0, -1], [0, -1, -1]]]
    assert dist_sq[0, 0, :2].tolist() == [0, 13] and np.isnan(dist_sq[0, :, 2]).all() and np.isnan(dist_sq[0, 1, 1])
    assert kso.repeatability(counts).tolist() == [[0.75]]


@needs_reference
def test_restatement_against_the_reference(pinned):
    views, sets = pinned
    ref = mso.load_reference(ref_snapshot.DEST)
    worst = worst_px = 0.0
    for kps, results in sets:                                       # asserts kept rows and counters identical
        rel, px = kso.reference_diffs(ref, views, kps, results, thresholds=EXPECTED['thresholds'])
        worst, worst_px = max(worst, rel), max(worst_px, px)
    print('max rel diff of the minima', worst, 'self pairs, px', worst_px)
    assert worst <= 8 * EXPECTED['reference_max_rel_diff'], (worst, EXPECTED['reference_max_rel_diff'])
    assert worst_px <= 8 * EXPECTED['reference_self_max_abs_diff_px'], (worst_px, EXPECTED['reference_self_max_abs_diff_px'])
