"""The homography SPECIFICATION (``tests/homography_ransac_oracle.py``) against independent facts - no
reference estimator exists on a machine without skimage and OpenCV, and no parity with them is claimed: (i) the minimal
models on their own samples, (ii) noise-free scenes, (iii) noisy scenes against ``H_gt``, (iv) the sampler, (v)
degenerate lists, (vi) the summation order, (vii) the summaries and ``transfer_points``; the fixture
(``tests/homography_ransac_expected.json``) against the recipe it records; and the ONE copy of the device arithmetic
(``csrc/homography_ransac_math.h``), compiled for the host, against the specification bit for bit."""
import ctypes
import itertools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import homography_oracle as hmo  # noqa: E402
import homography_ransac_oracle as hro  # noqa: E402
import match_score_oracle as mso  # noqa: E402

EXPECTED = json.loads((REPO / 'tests' / 'homography_ransac_expected.json').read_text())
OUTPUTS = ('models', 'model_counts', 'model', 'H', 'corner_sq', 'counts', 'inliers')


@pytest.fixture(scope='module')
def pinned():
    blocks, lists, _ = hro.pinned_call(EXPECTED['pinned']['draws'])
    return blocks, lists


def test_minimal_models_map_their_samples():
    """(i) Every model of a noise-free minimal sample maps its four rows onto their partners: the residual, relative
    to the picture (normalised coordinates), within 8 x the recorded one."""
    rec = EXPECTED['minimal']
    assert rec['scenes'] == hro.MINIMAL_SCENES and rec['hypotheses'] == hro.MINIMAL_HYPOTHESES
    worst = max(hro.minimal_check(i) for i in range(hro.MINIMAL_SCENES))
    print('minimal residual %.2e (recorded %.2e)' % (worst, rec['residual']))
    assert worst <= 8 * rec['residual'] and rec['residual'] < 1e-12


def test_noise_free_scenes_after_the_refit():
    """(ii) 50 % outliers at px_thr 0.01: the mean corner error after the refit within 8 x the recorded one (float32
    pixels perturb each end by ~3e-5 px; the least-squares fit over ~150 rows averages that down)."""
    assert EXPECTED['noise_free_recipe'] == hro.NOISE_FREE and len(EXPECTED['noise_free']) == hro.NOISE_FREE_SCENES
    bound = 8 * EXPECTED['noise_free_corner_error_px']
    for i, rec in enumerate(EXPECTED['noise_free']):
        res = hro.noise_free_result(i)
        err = hro.mean_corner_error(res)
        print(i, err, res['counts'])
        assert err <= bound and err == rec['corner_error_px'] and res['counts'].tolist() == rec['counts']
        assert res['counts'][4] >= res['counts'][3]


def test_noisy_scenes_reach_the_inliers_of_the_true_homography():
    """(iii) 0.5 px noise, 30 % / 60 % outliers, n_hyp 256, px_thr 3, two refit rounds: the delivered model has at least
    the inliers of ``H_gt`` scored by the same function.  The corner errors before and after the refit are recorded,
    not gated: only ``delivered >= selected`` and finiteness are asserted."""
    assert EXPECTED['noisy_recipe'] == hro.NOISY
    assert [(r['scene'], r['outliers']) for r in EXPECTED['noisy']] == list(hro.NOISY_SCENES)     # none excluded
    for rec in EXPECTED['noisy']:
        assert 0 <= rec['draw'] < hro.MAX_DRAWS
        res, true_inliers = hro.noisy_result(rec['scene'], rec['outliers'], rec['draw'])
        before, _ = hro.noisy_result(rec['scene'], rec['outliers'], rec['draw'], refit_iters=0)
        e0, e1 = hro.mean_corner_error(before), hro.mean_corner_error(res)
        print(rec['scene'], rec['outliers'], rec['draw'], res['counts'], true_inliers, '%.3f -> %.3f px' % (e0, e1))
        assert res['counts'][4] >= true_inliers == rec['true_inliers']
        assert res['counts'][4] >= res['counts'][3] and np.isfinite(e0) and np.isfinite(e1)
        assert res['counts'].tolist() == rec['counts']
        assert (e0, e1) == (rec['corner_error_px_minimal'], rec['corner_error_px'])


def test_sampler():
    """(iv) Distinct, ascending, in range; every 4-subset of 5 and of 6 rows is reached; a function of
    (seed, pair_id, h) alone; invariant under a permutation of the pairs with their ids."""
    for length in (4, 5, 6, 64, 100000):
        idx = hro.sample(3, 11, 4096, length)
        assert idx.shape == (4096, 4) and (idx >= 0).all() and (idx < length).all()
        assert (np.diff(idx, axis=1) > 0).all()
    assert hro.sample(3, 11, 8, 3).shape == (0, 4)
    for length in (5, 6):
        seen = {tuple(r) for r in hro.sample(0, 0, 4096, length).tolist()}
        assert seen == set(itertools.combinations(range(length), 4))
    a = hro.sample(5, 9, 64, 1000)
    assert np.array_equal(a[10:20], hro.sample(5, 9, 20, 1000)[10:])         # h alone, not n_hyp
    assert not np.array_equal(a, hro.sample(6, 9, 64, 1000)) and not np.array_equal(a, hro.sample(5, 8, 64, 1000))
    P, k1, k2, _ = hro.make_scene(50, seed=4, noise=0.3, outliers=0.3)
    Q, q1, q2, _ = hro.make_scene(70, seed=5, noise=0.3, outliers=0.3)
    ab = hro.estimate_lists([P, Q], [(k1, k2), (q1, q2)], 32, 1)
    ba = hro.estimate_lists([Q, P], [(q1, q2), (k1, k2)], 32, 1, pair_ids=[1, 0])
    for k in OUTPUTS:
        assert mso.equal_bits(ab[0][k], ba[1][k]) and mso.equal_bits(ab[1][k], ba[0][k]), k


def test_degenerate_lists():
    """(v) Four copies of one row, a list of 3, NaN rows, an EXACTLY collinear list: no model and no exception.
    Collinear rows in general position are NOT recognised (no conditioning test is made): whatever finite models
    pass the orientation test are scored; the list is pinned by its counters."""
    cases = hro.degenerate_lists()
    assert EXPECTED['degenerate'].keys() == cases.keys()
    for name, (P, k1, k2) in cases.items():
        res = hro.estimate(P, k1, k2, 16, 0, hro.PINNED_THR, 2, 0)
        assert res['counts'].tolist() == EXPECTED['degenerate'][name], name
        if name != 'collinear':
            assert res['counts'].tolist() == [len(k1), 0, -1, 0, 0, 0] and np.isnan(res['models']).all(), name
            assert np.isnan(res['H']).all() and np.isnan(res['corner_sq']).all() and not res['inliers'].any()
    x1 = hro.normalise(*cases['collinear_exact'])[0]
    assert (x1 == 0.0).all()
    # sizes that are no whole numbers: not estimated, every counter -1
    P, k1, k2 = cases['collinear']
    for at, v in ((9, 640.5), (10, 0.0), (11, np.nan), (12, 8193.0)):
        bad = P.copy()
        bad[at] = v
        res = hro.estimate(bad, k1, k2, 16)
        assert res['counts'].tolist() == [-1] * 6 and np.isnan(res['H']).all() and (res['model_counts'] == -1).all()
    # no ground truth: the estimate is made, the errors are NaN
    P, k1, k2, _ = hro.make_scene(40, seed=8, gt=False)
    res = hro.estimate(P, k1, k2, 16)
    assert res['counts'][2] >= 0 and np.isfinite(res['H']).all() and np.isnan(res['corner_sq']).all()
    assert np.isinf(hro.homography_errors(res['corner_sq'][None], res['counts'][None])).all()
    # the refit's two refusals
    for name, (P, k1, k2, M, thr) in hro.refit_cases().items():
        res = hro.estimate(P, k1, k2, px_thr=thr, models=M)
        rec = EXPECTED['refit'][name]
        assert res['counts'].tolist() == rec['counts'] and res['margins']['acceptances'] == rec['acceptances'], name
        assert res['counts'][5] == 0 and mso.equal_bits(res['model'], M[0])
    assert EXPECTED['refit']['zero_pivot']['acceptances'] == [] and EXPECTED['refit']['rejected']['acceptances'] == [-1]
    x1, y1, x2, y2, _ = hro.normalise(*hro.refit_cases()['zero_pivot'][:3], 1.0)
    inl = np.array([1, 1, 1, 1, 0, 0], bool)
    assert hro.solve8(hro.normal_sums(x1, y1, x2, y2, inl), 4) is None          # an exact zero pivot


def test_summation_order_is_the_stated_one():
    """(vi) The tree sum differs from ``np.sum`` on a crafted list and equals a literal loop restatement."""
    rng = np.random.default_rng(7)
    terms = rng.standard_normal(700) * 10.0 ** rng.integers(-8, 8, 700)
    positions = np.sort(rng.choice(2000, 700, replace=False))
    got = hro.ordered_sum(terms, positions)
    # the literal restatement: 256 running sums, then the butterfly written as nested loops over explicit indices
    part = [0.0] * 256
    for t, j in zip(terms.tolist(), positions.tolist()):
        part[j % 256] = part[j % 256] + t
    v = [np.float64(x) for x in part]
    for o in (1, 2, 4, 8, 16, 32):
        v = [v[i] + v[i ^ o] for i in range(256)]
    want = (v[0] + v[64]) + (v[128] + v[192])
    assert got == want
    assert all(v[i] == v[64 * (i // 64)] for i in range(256))                  # every lane of a group ends equal
    assert got != float(np.sum(terms)) and abs(got - np.sum(terms)) <= 1e-6 * np.abs(terms).sum()
    # normal_sums is that order: one term of a list checked against ordered_sum
    P, k1, k2, _ = hro.make_scene(600, seed=9, noise=0.5, outliers=0.4)
    x1, y1, x2, y2, _ = hro.normalise(P, k1, k2)
    inl = np.random.default_rng(1).random(600) < 0.6
    S = hro.normal_sums(x1, y1, x2, y2, inl)
    pos = np.nonzero(inl)[0]
    rows = hro.row_terms(x1[pos], y1[pos], x2[pos], y2[pos])
    for k in (0, 7, 18, 27):
        assert S[k] == hro.ordered_sum(rows[k], pos), k


def test_summaries_and_transfer_points():
    """(vii) ``homography_errors`` / ``homography_auc`` by hand, with inf and ties; ``transfer_points`` forward and
    inverse against the numpy restatement."""
    import imagematching_oetr_amd as pkg
    sq = np.array([[1.0, 4.0, 9.0, 16.0], [0.0, 0.0, 0.0, 0.0], [np.nan, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0],
                   [4.0, 4.0, 4.0, 4.0], [1.0, 1.0, 1.0, np.inf]])
    counts = np.array([[9, 3, 0, 5, 6, 1], [9, 3, 1, 9, 9, 2], [9, 3, 2, 5, 5, 0], [3, 0, -1, 0, 0, 0],
                       [9, 3, 0, 5, 5, 0], [9, 1, 0, 4, 4, 0]], np.int32)
    got = pkg.homography_errors(dict(corner_sq=sq, counts=counts))
    assert got.tolist() == [2.5, 0.0, np.inf, np.inf, 2.0, np.inf]
    assert np.array_equal(got, hro.homography_errors(sq, counts))
    both = pkg.homography_errors(dict(corner_sq=torch.from_numpy(sq), counts=torch.from_numpy(counts)))
    assert np.array_equal(both, got)
    # errors 0, 2, 2.5 and three inf of 6 pairs at threshold 3: trapezoids to (0, 1/6), (2, 2/6), (2.5, 3/6), flat to 3
    by_hand = (0.0 + 2.0 * (1 / 6 + 2 / 6) / 2 + 0.5 * (2 / 6 + 3 / 6) / 2 + 0.5 * 3 / 6) / 3
    auc = pkg.homography_auc(got, thresholds=(3, 2))
    assert auc[0] == pytest.approx(by_hand, abs=1e-15) and auc == [float(a) for a in hro.homography_auc(got, (3, 2))]
    assert auc[1] == pytest.approx((2.0 * (1 / 6 + 1 / 6) / 2) / 2, abs=1e-15)   # 2 is not strictly below 2
    tie = pkg.homography_auc(np.array([1.0, 1.0, np.inf]), thresholds=(3,))
    assert tie[0] == pytest.approx((1.0 * (1 / 3) / 2 + 0.0 + 2.0 * (2 / 3)) / 3, abs=1e-15)
    summary = pkg.match_homography_auc(dict(corner_sq=sq, counts=counts))
    assert summary['auc'] == [100.0 * a for a in pkg.homography_auc(got)] and summary['n_no_homography'] == 3
    assert summary['n_pairs'] == 6 and summary['thresholds'] == (3, 5, 10)
    # transfer_points
    P, k1, k2, _ = hro.make_scene(30, seed=12)
    H = P[:9]
    pts = k1.astype(np.float64)
    fwd = pkg.transfer_points(H.reshape(3, 3), pts)
    assert isinstance(fwd, np.ndarray) and np.array_equal(fwd, hro.transfer_points(H, pts))
    assert np.abs(fwd - k2).max() < 1e-4                                        # float32 pixels
    back = pkg.transfer_points(torch.from_numpy(H), torch.from_numpy(fwd), inverse=True)
    assert torch.is_tensor(back) and np.array_equal(back.numpy(), hro.transfer_points(H, fwd, inverse=True))
    assert np.abs(back.numpy() - pts).max() < 1e-9
    two = pkg.transfer_points(np.stack([H, np.eye(3).reshape(9)]), pts, offsets=[2, 10, 25])
    assert np.isnan(two[:2]).all() and np.isnan(two[25:]).all()
    assert np.array_equal(two[2:10], fwd[2:10]) and np.array_equal(two[10:25], pts[10:25])
    with pytest.raises(ValueError, match='offsets'):
        pkg.transfer_points(np.stack([H, H]), pts)


def test_fixture_is_its_recipe(pinned):
    """The fixture's inputs are regenerated from the recipe bit for bit, its records are the specification's, and the
    margins of every pinned list hold: no decision of the pinned call hangs on a last bit."""
    blocks, lists = pinned
    rec = EXPECTED['pinned']
    assert rec['recipe'] == [list(r) for r in hro.PINNED] and rec['seed'] == hro.PINNED_SEED
    assert [len(k1) for k1, _ in lists][:11] == [0, 3, 4, 5, 63, 64, 65, 255, 256, 257, 600] and len(lists) == 16
    assert sorted(rec['n_hyp']) == sorted(str(n) for n in hro.PINNED_HYPOTHESES) == sorted(['1', '255', '256', '257', '600'])
    assert cvo.sha(blocks) == rec['blocks_sha256']
    assert [cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists] == rec['kpts_sha256']
    low = dict(threshold=np.inf, positive=np.inf)
    for n in hro.PINNED_HYPOTHESES:
        for r in hro.PINNED_REFITS:
            results = hro.estimate_lists(blocks, lists, n, hro.PINNED_SEED, hro.PINNED_THR, r)
            assert [hro.list_record(res) for res in results] == rec['n_hyp'][str(n)][str(r)], (n, r)
            for res in results:
                assert hro.margins_hold(res)
                assert res['counts'][4] >= res['counts'][3] and res['counts'][5] <= r
                for k in low:
                    low[k] = min(low[k], res['margins'].get(k, np.inf))
    assert low == rec['margins'] and min(low.values()) >= hro.MIN_MARGIN
    # the refit does something in the pinned call: some list accepts a round, some list gains inliers
    last = [r['counts'] for r in rec['n_hyp']['600']['2']]
    assert any(c[5] > 0 for c in last) and any(c[4] > c[3] for c in last)


@pytest.fixture(scope='module')
def hostmath(tmp_path_factory):
    """``csrc/homography_ransac_math.h`` compiled for the host (tools/homography_ransac_hostmath.cpp)."""
    out = tmp_path_factory.mktemp('hostmath')
    subprocess.run(['make', '-C', str(REPO / 'imagematching_oetr_amd' / 'csrc'), 'hostmath-homography_ransac',
                    f'HOSTCHECK_BIN={out}'], check=True, capture_output=True)
    lib = ctypes.CDLL(str(out / 'libhomography_ransac_hostmath.so'))
    vp = ctypes.c_void_p
    lib.hr_host_estimate.restype = None
    lib.hr_host_estimate.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_double, ctypes.c_int, vp] + [vp] * 7
    lib.hr_host_sample.restype = None
    lib.hr_host_sample.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, vp]
    lib.hr_host_tree_sum.restype = ctypes.c_double
    lib.hr_host_tree_sum.argtypes = [vp]

    def estimate(P, k1, k2, n_hyp=256, seed=0, px_thr=3.0, refit_iters=2, pair_id=0, models=None):
        P, k1, k2 = (np.ascontiguousarray(P, np.float64), np.ascontiguousarray(k1, np.float32),
                     np.ascontiguousarray(k2, np.float32))
        m = len(k1)
        given = None if models is None else np.ascontiguousarray(models, np.float64).reshape(-1, 9)
        n = n_hyp if given is None else len(given)
        o = dict(models=np.zeros((n, 9)), model_counts=np.zeros(n, np.int32), model=np.zeros(9), H=np.zeros(9),
                 corner_sq=np.zeros(4), counts=np.zeros(6, np.int32), inliers=np.zeros(max(m, 1), np.uint8))
        at = lambda a: a.ctypes.data
        lib.hr_host_estimate(at(P), at(k1) if m else None, at(k2) if m else None, m, n, seed, pair_id, px_thr,
                             refit_iters, None if given is None else at(given), *(at(o[k]) for k in OUTPUTS))
        o['inliers'] = o['inliers'][:m]
        return o

    lib.estimate = estimate
    return lib


def test_device_arithmetic_compiled_for_the_host_equals_the_specification(pinned, hostmath):
    """Before any device run: the header the kernels include, with the kernels' loops restated serially, gives every
    output of the specification bit for bit - the pinned lists, the degenerate ones, the refit's refusals, bad sizes."""
    blocks, lists = pinned

    def same(tag, want, got):
        for k in OUTPUTS:
            assert mso.equal_bits(np.asarray(want[k]), got[k]), (tag, k)

    for p, (k1, k2) in enumerate(lists):
        for n, r in ((1, 2), (255, 0), (257, 1), (600, 2)):
            same((p, n, r), hro.estimate(blocks[p], k1, k2, n, hro.PINNED_SEED, hro.PINNED_THR, r, p),
                 hostmath.estimate(blocks[p], k1, k2, n, hro.PINNED_SEED, hro.PINNED_THR, r, p))
    for name, (P, k1, k2) in hro.degenerate_lists().items():
        same(name, hro.estimate(P, k1, k2, 16, 0, 3.0, 2, 1), hostmath.estimate(P, k1, k2, 16, 0, 3.0, 2, 1))
        bad = P.copy()
        bad[10] = 480.5
        same(name + ' bad', hro.estimate(bad, k1, k2, 16), hostmath.estimate(bad, k1, k2, 16))
    for name, (P, k1, k2, M, thr) in hro.refit_cases().items():
        same(name, hro.estimate(P, k1, k2, px_thr=thr, models=M), hostmath.estimate(P, k1, k2, px_thr=thr, models=M))
    for rec in EXPECTED['noisy'][:4]:
        P, k1, k2, _ = hro.make_scene(hro.NOISY['n'], seed=2000 + 20 * rec['scene'] + rec['draw'],
                                      noise=hro.NOISY['noise'], outliers=rec['outliers'])
        same('noisy', hro.estimate(P, k1, k2, 256, 1, 3.0, 4, rec['scene']),
             hostmath.estimate(P, k1, k2, 256, 1, 3.0, 4, rec['scene']))
    # the sampler and the tree on their own
    for length in (4, 5, 64, 100000):
        idx = np.zeros((300, 4), np.int64)
        hostmath.hr_host_sample(9, 77, 300, length, idx.ctypes.data)
        assert np.array_equal(idx, hro.sample(9, 77, 300, length))
    part = np.random.default_rng(3).standard_normal(256) * 1e3
    assert hostmath.hr_host_tree_sum(part.ctypes.data) == hro.tree_sum(part)
