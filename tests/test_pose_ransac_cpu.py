"""The relative-pose SPECIFICATION (``tests/pose_ransac_oracle.py``) against independent facts - no
reference estimator exists on a machine without OpenCV, and no parity with it is claimed: (i) the solver's models on
noise-free samples, (ii) noise-free scenes, (iii) noisy scenes against the true essential matrix, (iv) the sampler,
(v) degenerate inputs, (vi) ``pose_auc`` by hand, (vii) the margins of the pinned lists; and the fixture
(``tests/pose_ransac_expected.json``) against the recipe it records."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import pose_ransac_oracle as pro  # noqa: E402

EXPECTED = json.loads((REPO / 'tests' / 'pose_ransac_expected.json').read_text())


@pytest.fixture(scope='module')
def pinned():
    blocks, lists, _ = pro.pinned_call(EXPECTED['pinned']['draws'])
    return blocks, lists, {n: pro.estimate_lists(blocks, lists, n, pro.PINNED_SEED) for n in pro.PINNED_HYPOTHESES}


def test_solver_models_on_true_correspondences():
    """(i) Every model of a noise-free sample: its seven ``x2^T F x1`` and ``det F`` are zero to within 8 x the
    recorded relative bounds, and one of the hypothesis's roots is the true ``[t]x R`` up to scale.  The last bound is
    reasoned, not measured: float32 pixels perturb the normalised coordinates by 3e-5 / f = 5e-8, and a minimal
    7-row sample amplifies that by its condition number, taken as at most 2e5 -> 1e-2 on matrices of unit norm (the
    largest distance met is recorded: 2.7e-4)."""
    rec = EXPECTED['solver']
    assert rec['scenes'] == pro.SOLVER_SCENES and rec['hypotheses'] == pro.SOLVER_HYPOTHESES
    checks = [pro.solver_check(i) for i in range(pro.SOLVER_SCENES)]
    print('residual %.2e (recorded %.2e), det %.2e (%.2e), nearest root %.2e (%.2e)' % (
        max(c[0] for c in checks), rec['residual'], max(c[1] for c in checks), rec['det'],
        max(c[2] for c in checks), rec['nearest_root']))
    assert max(c[0] for c in checks) <= 8 * rec['residual']
    assert max(c[1] for c in checks) <= 8 * rec['det']
    assert max(c[2] for c in checks) <= 1e-2


def test_noise_free_scenes_give_the_true_pose():
    """(ii) pose_error < 0.01 degrees (float32 pixels: ~3e-5 px); the drawing used is the recorded one."""
    assert len(EXPECTED['noise_free']) == pro.NOISE_FREE_SCENES
    for i, rec in enumerate(EXPECTED['noise_free']):
        assert 0 <= rec['draw'] < pro.MAX_DRAWS
        res = pro.estimate(*pro.noise_free_scene(i, rec['draw']), 256, 0, 1.0, i)
        err = pro.error_of(res)
        print(i, rec['draw'], err)
        assert err < pro.NOISE_FREE_BOUND_DEG and err == rec['pose_error_deg'], (i, err)
        assert res['counts'].tolist() == rec['counts'] and res['counts'][3] == 200     # every row an inlier


def test_noisy_scenes_find_at_least_the_true_models_inliers():
    """(iii) 0.5 px noise, 30 % / 60 % outliers: the selected model has at least the inliers of the true essential
    matrix under the same test, minus nothing; the errors are the recorded ones."""
    assert len(EXPECTED['noisy']) >= 12 and EXPECTED['noisy_recipe'] == pro.NOISY
    assert [(r['scene'], r['outliers']) for r in EXPECTED['noisy']] == list(pro.NOISY_SCENES)
    for rec in EXPECTED['noisy']:
        assert 0 <= rec['draw'] < pro.MAX_DRAWS
        res, true_inliers = pro.noisy_result(rec['scene'], rec['outliers'], rec['draw'])
        print(rec['scene'], rec['outliers'], rec['draw'], res['counts'].tolist(), true_inliers, pro.error_of(res))
        assert res['counts'][3] >= true_inliers == rec['true_inliers']
        assert res['counts'].tolist() == rec['counts'] and pro.error_of(res) == rec['pose_error_deg']


@pytest.mark.parametrize('length', [7, 8, 9, 64, 100000])
def test_sampler(length):
    """(iv) distinct, in range, ascending; a function of (seed, pair_id, h) alone; different for different seeds."""
    idx = pro.sample(3, 11, 300, length)
    assert idx.shape == (300, 7) and idx.min() >= 0 and idx.max() < length
    assert (np.diff(idx, axis=1) > 0).all()                                  # ascending: distinct
    if length == 7:
        assert (idx == np.arange(7)).all()
    else:
        distinct = len({tuple(r) for r in idx.tolist()})
        assert distinct == {8: 8, 9: 36}.get(length, 300)        # every 7-subset of 8 or 9 rows is reached
        assert not np.array_equal(idx, pro.sample(4, 11, 300, length))       # another seed
        assert not np.array_equal(idx, pro.sample(3, 12, 300, length))       # another pair
    assert np.array_equal(idx[:50], pro.sample(3, 11, 50, length))           # h alone, not n_hyp
    if length == 100000:                                                      # every part of the list is reached
        assert idx.min() < 2000 and idx.max() > 98000
    assert pro.sample(3, 11, 300, 6).shape == (0, 7)


def test_pair_ids_permute_with_the_pairs(pinned):
    """(iv) invariance under a permutation of the pair list when the ids travel with the pairs."""
    blocks, lists, wants = pinned
    perm = np.random.default_rng(1).permutation(len(lists))
    got = pro.estimate_lists(blocks[perm], [lists[p] for p in perm], 85, pro.PINNED_SEED, pair_ids=perm)
    for i, p in enumerate(perm):
        for k in ('models', 'model_counts', 'pose', 'cosines', 'counts', 'inliers'):
            assert pro.mso.equal_bits(got[i][k], wants[85][p][k]), (k, i, p)


def test_degenerate_inputs_give_no_model_and_no_exception():
    """(v) seven copies of one row, a list of 6, a collinear sample, NaN keypoints: no model, no exception.  The
    collinear sample that gives no model is the EXACTLY degenerate one (every point of picture 1 on ``u = cx`` of a
    camera whose normalisation is exact: the first column of the system is zero).  A stated departure: collinear rows
    in general position are rank-deficient but not exactly singular in float64, the elimination meets no zero pivot,
    and the result is arbitrary finite models and a meaningless pose - only an exactly singular sample is recognised.
    That case is pinned by its recorded counters."""
    P, k1, k2 = pro.noise_free_scene(0)
    none = [9, 0, -1, 0, 0]
    cases = pro.degenerate_lists()
    for name in ('copies', 'collinear_exact', 'nan'):
        res = pro.estimate(*cases[name], 16)
        assert res['counts'].tolist() == none, name
        assert np.isnan(res['models']).all() and np.isnan(res['model']).all() and np.isnan(res['pose']).all(), name
        assert np.isnan(res['cosines']).all() and not res['inliers'].any(), name
    x1 = pro.normalise(*cases['collinear_exact'])[0]
    assert (x1 == 0.0).all()                                                 # exactly on the line
    res = pro.estimate(*cases['collinear'], 16)
    assert res['counts'].tolist() == EXPECTED['degenerate']['collinear_counts'] == [9, 42, 6, 9, 9]
    assert np.isfinite(res['pose']).all()                                    # the departure: a pose is delivered
    res = pro.estimate(P, k1[:6], k2[:6], 16)
    assert res['counts'].tolist() == [6, 0, -1, 0, 0] and res['models'].shape == (48, 9) and np.isnan(res['cosines']).all()
    mixed = k1[:40].copy()
    mixed[::3] = np.nan                                                      # NaN rows among good ones: never inliers
    res = pro.estimate(P, mixed, k2[:40], 64)
    assert not res['inliers'][::3].any() and res['counts'][2] >= 0 and res['counts'][3] == 26
    empty = pro.estimate(P, k1[:0], k2[:0], 4)
    assert empty['counts'].tolist() == [0, 0, -1, 0, 0] and empty['inliers'].shape == (0,)
    errs = pro.pose_errors(np.stack([res['cosines'], empty['cosines']]), np.stack([res['counts'], empty['counts']]))
    assert np.isfinite(errs[2][0]) and np.isinf(errs[2][1]) and np.isinf(errs[0][1]) and np.isinf(errs[1][1])


def test_models_of_the_callers_and_the_scoring_rules():
    P, k1, k2 = pro.noise_free_scene(1)
    E = pro.true_essential(P)
    models = np.stack([np.zeros(9), np.full(9, np.nan), E, 2.0 * E, np.r_[E[:8], np.inf]])
    res = pro.estimate(P, k1, k2, models=models)
    # zero denominator fails; NaN / inf models score -1; the lowest number wins the tie of E and 2 E
    assert res['model_counts'].tolist() == [0, -1, 200, 200, -1] and res['counts'].tolist() == [200, 3, 2, 200, 200]
    assert pro.error_of(res) < 1e-3
    R, t = res['pose'][:9].reshape(3, 3), res['pose'][9:]
    assert abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(t) - 1) < 1e-12
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    R1, R2, _ = pro.decompose(E)
    assert abs(np.linalg.det(R1.reshape(3, 3)) - 1) < 1e-12 and abs(np.linalg.det(R2.reshape(3, 3)) - 1) < 1e-12


def test_pose_auc_by_hand():
    """(vi) hand-computed lists, with inf entries, nothing below a threshold, and ties."""
    # errors 1, 2: recall steps to 1/2 at 1 and to 1 at 2; up to 4: 0.5*1*0.5 + 1*0.75 + 2*1 = 3
    assert pro.pose_auc([2.0, 1.0], [4]) == [pytest.approx(3.0 / 4, abs=1e-15)]
    # one of four at 2 degrees, the rest without a pose: up to 10: 0.5*2*0.25 + 8*0.25 = 2.25
    assert pro.pose_auc([np.inf, 2.0, np.inf, np.inf], [10, 1]) == [pytest.approx(0.225, abs=1e-15), 0.0]
    assert pro.pose_auc([np.inf, np.inf], [5, 10, 20]) == [0.0, 0.0, 0.0]      # nothing below any threshold
    assert pro.pose_auc([30.0, 40.0], [5]) == [0.0]
    # ties: both at 1: recall 1/2 at 1, then 1 at 1 (a zero-width step); up to 2: 0.5*1*0.5 + 0 + 1*1 = 1.25
    assert pro.pose_auc([1.0, 1.0], [2]) == [pytest.approx(0.625, abs=1e-15)]
    assert pro.pose_auc([0.0, 0.0, 0.0], [5]) == [pytest.approx(1.0, abs=1e-15)]
    # an error exactly at the threshold is not below it
    assert pro.pose_auc([5.0], [5]) == [0.0]


def test_pinned_lists_keep_their_margins_and_equal_the_fixture(pinned):
    """(vii) margins: a bit of rounding cannot silently flip an INLIER or a CHEIRALITY decision of a pinned list, and
    the best two models differ in count or tie exactly and resolve by number.  The solver's own comparisons (the pivot
    choice, ``disc > 0``, the signs at the turning points) carry no margin: they rest on the device computing the same
    bits, which the GPU tests assert on the models themselves.  The recorded results are the recipe's."""
    blocks, lists, wants = pinned
    rec = EXPECTED['pinned']
    assert rec['recipe'] == [list(r) for r in pro.PINNED] and rec['seed'] == pro.PINNED_SEED
    assert cvo.sha(blocks) == rec['blocks_sha256']
    assert [cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists] == rec['kpts_sha256']
    assert [len(k1) for k1, _ in lists][:11] == [0, 6, 7, 8, 63, 64, 65, 255, 256, 257, 600] and len(lists) == 16
    thr = depth = np.inf
    for n in pro.PINNED_HYPOTHESES:
        for p, res in enumerate(wants[n]):
            g = res['margins']
            if g:
                assert g['threshold'] >= pro.MIN_THRESHOLD_MARGIN and g['depth'] >= pro.MIN_DEPTH_MARGIN, (n, p, g)
                tied = np.flatnonzero(res['model_counts'] == g['best'])
                assert res['counts'][2] == tied[0] and (len(tied) > 1) == (g['best'] == g['second'])   # by number
                thr, depth = min(thr, g['threshold']), min(depth, g['depth'])
            assert pro.list_record(res) == rec['n_hyp'][str(n)][p], (n, p)
    assert thr == rec['margins']['threshold'] and depth == rec['margins']['depth']
    # the tiles of 256 models: 255 and 258 models sit on both sides of one, 771 reaches the third
    assert [3 * n for n in pro.PINNED_HYPOTHESES] == [3, 255, 258, 771]
    # the reference's compute_pose_error / pose_auc were compared when the fixture was written
    if rec.get('reference_checked', EXPECTED['reference_checked']):
        assert EXPECTED['reference_auc_equal'] is True and EXPECTED['reference_max_abs_diff_deg'] < 1e-5
