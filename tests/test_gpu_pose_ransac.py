"""GPU tests of the relative-pose extension (``oetr_pose_ransac``, ``csrc/pose_ransac.hip``; ``pose_ransac.py``;
``evaluate.pose_errors`` / ``match_pose_auc``).  There is no tolerance anywhere: every output - the workspace's models
(NaN patterns included) and per-model counts, ``model``, ``pose``, ``cosines``, ``counts``, ``inliers`` - is compared
BIT FOR BIT (``mso.equal_bits``: NaN equals NaN whatever its payload) with the float64 specification
``tests/pose_ransac_oracle.py``, whose pinned lists keep every inlier and cheirality decision away from last-bit differences (asserted in
``tests/test_pose_ransac_cpu.py``).  The first test pins the one assumption the parity rests on: the device's float64
square root equals ``np.sqrt``.  The fixture is 16 lists, 3865 matches, at most 771 models per list."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import match_score_oracle as mso  # noqa: E402
import pose_ransac_oracle as pro  # noqa: E402

pytestmark = pytest.mark.gpu
EXPECTED = json.loads((REPO / 'tests' / 'pose_ransac_expected.json').read_text())
KEYS = ('model', 'pose', 'cosines', 'counts', 'inliers')


def host(out):
    from imagematching_oetr_amd.pose_ransac import workspace_views
    got = {k: out[k].cpu().numpy() for k in KEYS if k in out}
    models, model_counts = workspace_views(out)
    got['models'], got['model_counts'] = models.cpu().numpy(), model_counts.cpu().numpy()
    return got


def assert_pairs(got, wants, bounds, tag=None, models=True):
    """Every pair of a call against its specified result, by bits."""
    for p, want in enumerate(wants):
        lo, hi = int(bounds[p]), int(bounds[p + 1])
        if models:
            assert mso.equal_bits(got['models'][p], want['models']), (tag, p, 'models')
        assert np.array_equal(got['model_counts'][p], want['model_counts']), (tag, p, 'model_counts')
        for k in ('model', 'pose', 'cosines'):
            assert mso.equal_bits(got[k][p], want[k]), (tag, p, k, got[k][p], want[k])
        assert got['counts'][p].tolist() == want['counts'].tolist(), (tag, p, got['counts'][p], want['counts'])
        if 'inliers' in got:
            assert np.array_equal(got['inliers'][lo:hi], want['inliers']), (tag, p, 'inliers')


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert mso.equal_bits(a[k], b[k]), k


@pytest.fixture(scope='module')
def pinned(gpu):
    """The pinned lists, their specified results per ``n_hyp`` and the device inputs: made once, shared, never
    modified."""
    blocks, lists, _ = pro.pinned_call(EXPECTED['pinned']['draws'])
    assert [cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists] == EXPECTED['pinned']['kpts_sha256']
    assert cvo.sha(blocks) == EXPECTED['pinned']['blocks_sha256']        # a wrong input cannot pass as a wrong kernel
    lengths = [len(k1) for k1, _ in lists]
    k1, k2 = np.concatenate([a for a, _ in lists]), np.concatenate([b for _, b in lists])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    wants = {n: pro.estimate_lists(blocks, lists, n, pro.PINNED_SEED) for n in pro.PINNED_HYPOTHESES}
    return dict(blocks=blocks, lists=lists, lengths=lengths, bounds=np.concatenate([[0], np.cumsum(lengths)]),
                params=t(blocks), k1=t(k1), k2=t(k2), host_k=(k1, k2), wants=wants)


def sqrt_inputs():
    """2^20 normal doubles over 1e-30 .. 1e30: random mantissas and exponents, mantissas at 1 +- ulp (and 2 +- ulp:
    both parities of the exponent), perfect squares, and squares +- one ulp."""
    rng = np.random.default_rng(5)
    n = 1 << 20
    x = np.exp(rng.uniform(np.log(1e-30), np.log(1e30), n))
    e = np.ldexp(1.0, rng.integers(-99, 100, 1 << 16))
    x[:1 << 16] = e
    x[1 << 16:2 << 16] = np.nextafter(e, np.inf)
    x[2 << 16:3 << 16] = np.nextafter(e, 0.0)
    r = np.floor(rng.uniform(1.0, 2.0 ** 26, 1 << 16))                    # r * r is exact
    x[3 << 16:4 << 16] = r * r
    x[4 << 16:5 << 16] = np.nextafter(r * r, np.inf)
    x[5 << 16:6 << 16] = np.nextafter(r * r, 0.0)
    m = 1.0 + rng.integers(0, 1 << 52, 1 << 16) * 2.0 ** -52                # m * m rounded: near-ties of the root
    x[6 << 16:7 << 16] = (m * m) * np.ldexp(1.0, rng.integers(-90, 90, 1 << 16))
    assert np.isfinite(x).all() and (x >= 1e-31).all() and (x <= 1e31).all()
    return x


def test_device_sqrt_is_numpys(gpu):
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd.hip_engine import _check, _stream
    lib = pkg.load_library()
    x = sqrt_inputs()
    xd = torch.from_numpy(x).to(gpu)
    yd = torch.empty_like(xd)
    with torch.cuda.device(gpu):
        _check(lib, lib.oetr_pose_ransac_sqrt(xd.data_ptr(), yd.data_ptr(), xd.numel(), _stream(gpu)),
               'oetr_pose_ransac_sqrt')
    y, want = yd.cpu().numpy(), np.sqrt(x)
    differ = y.view(np.uint64) != want.view(np.uint64)
    print('sqrt: %d of %d differ' % (int(differ.sum()), x.size))
    assert not differ.any(), (int(differ.sum()), x[differ][:4], y[differ][:4], want[differ][:4])


@pytest.mark.parametrize('n_hyp', pro.PINNED_HYPOTHESES)
def test_pinned_call_equals_the_specification_and_the_fixture(gpu, pinned, n_hyp):
    import imagematching_oetr_amd as pkg
    assert pinned['lengths'][:11] == [0, 6, 7, 8, 63, 64, 65, 255, 256, 257, 600] and len(pinned['lengths']) == 16
    out = pkg.estimate_poses(pinned['params'], pinned['k1'], pinned['k2'], lengths=pinned['lengths'], n_hyp=n_hyp,
                             seed=pro.PINNED_SEED)
    M = int(pinned['bounds'][-1])
    assert out['model'].dtype == torch.float64 and out['model'].shape == (16, 9) and out['model'].is_cuda
    assert out['pose'].shape == (16, 12) and out['cosines'].shape == (16, 2)
    assert out['counts'].dtype == torch.int32 and out['counts'].shape == (16, 5)
    assert out['inliers'].dtype == torch.uint8 and out['inliers'].shape == (M,) and out['n_models'] == 3 * n_hyp
    got = host(out)
    wants = pinned['wants'][n_hyp]
    assert_pairs(got, wants, pinned['bounds'], n_hyp)
    records = EXPECTED['pinned']['n_hyp'][str(n_hyp)]
    assert got['counts'].tolist() == [rec['counts'] for rec in records]
    for p, rec in enumerate(records):
        assert cvo.sha(np.nan_to_num(got['models'][p], nan=-7.0)) == rec['models_sha256'], p
        assert cvo.sha(got['model_counts'][p]) == rec['model_counts_sha256'], p
        assert cvo.sha(np.nan_to_num(got['pose'][p], nan=-7.0)) == rec['pose_sha256'], p
    # lists of fewer than 7 rows: no pose
    for p in (0, 1):
        assert got['counts'][p].tolist() == [pinned['lengths'][p], 0, -1, 0, 0]
        assert np.isnan(got['model'][p]).all() and np.isnan(got['pose'][p]).all() and np.isnan(got['cosines'][p]).all()
    # the summary equals the specification's, which restates the reference's
    errs = pkg.pose_errors(out)
    spec = pro.pose_errors(np.stack([w['cosines'] for w in wants]), np.stack([w['counts'] for w in wants]))
    for k, want in zip(('err_R', 'err_t', 'pose_error'), spec):
        assert mso.equal_bits(errs[k], want), k
    assert np.isinf(errs['pose_error'][:2]).all()
    auc = pkg.match_pose_auc(out)
    assert auc['auc'] == [100.0 * a for a in pro.pose_auc(spec[2])] and auc['n_no_pose'] == int(np.isinf(spec[2]).sum())


def test_host_inputs_offsets_float16_and_no_inliers(gpu, pinned):
    import imagematching_oetr_amd as pkg
    n_hyp = 85
    full = host(pkg.estimate_poses(pinned['params'], pinned['k1'], pinned['k2'], lengths=pinned['lengths'],
                                   n_hyp=n_hyp, seed=pro.PINNED_SEED))
    # host arrays, uploaded
    got = host(pkg.estimate_poses(pinned['blocks'], *pinned['host_k'], lengths=pinned['lengths'], n_hyp=n_hyp,
                                  seed=pro.PINNED_SEED))
    assert_same(got, full, KEYS + ('models', 'model_counts'))
    # inliers=False: the same everything else
    bare = pkg.estimate_poses(pinned['params'], pinned['k1'], pinned['k2'], lengths=pinned['lengths'], n_hyp=n_hyp,
                              seed=pro.PINNED_SEED, inliers=False)
    assert 'inliers' not in bare
    assert_same(host(bare), full, ('model', 'pose', 'cosines', 'counts', 'models', 'model_counts'))
    # device offsets with rows in no list before the first and after the last list: 0 there, the lists as before;
    # the stale contents of a reused `out` are overwritten
    head, tail = 70, 67
    filler = lambda m: torch.full((m, 2), 3.0, device=gpu)
    k1 = torch.cat([filler(head), pinned['k1'], filler(tail)])
    k2 = torch.cat([filler(head), pinned['k2'], filler(tail)])
    offsets = torch.from_numpy((pinned['bounds'] + head).astype(np.int32)).to(gpu)
    out = pkg.estimate_poses(pinned['params'], k1, k2, offsets=offsets, n_hyp=n_hyp, seed=pro.PINNED_SEED)
    out['inliers'].fill_(9)
    out['counts'].fill_(-5)
    again = pkg.estimate_poses(pinned['params'], k1, k2, offsets=offsets, n_hyp=n_hyp, seed=pro.PINNED_SEED, out=out)
    assert again is out
    shifted = host(out)
    assert not shifted['inliers'][:head].any() and not shifted['inliers'][-tail:].any()
    shifted['inliers'] = shifted['inliers'][head:-tail]
    assert_same(shifted, full, KEYS + ('models', 'model_counts'))
    # float16 keypoints are widened exactly
    h1, h2 = pinned['k1'].half(), pinned['k2'].half()
    a = host(pkg.estimate_poses(pinned['params'], h1, h2, lengths=pinned['lengths'], n_hyp=n_hyp, seed=3))
    b = host(pkg.estimate_poses(pinned['params'], h1.float(), h2.float(), lengths=pinned['lengths'], n_hyp=n_hyp, seed=3))
    assert_same(a, b, KEYS + ('models', 'model_counts'))
    # another seed gives other samples; another threshold other counts
    other = host(pkg.estimate_poses(pinned['params'], pinned['k1'], pinned['k2'], lengths=pinned['lengths'],
                                    n_hyp=n_hyp, seed=pro.PINNED_SEED + 1))
    assert not mso.equal_bits(other['models'], full['models'])
    want = pro.estimate_lists(pinned['blocks'][10:12], pinned['lists'][10:12], 8, 7, px_thr=2.5)
    got = host(pkg.estimate_poses(pinned['blocks'][10:12], np.concatenate([a for a, _ in pinned['lists'][10:12]]),
                                  np.concatenate([b for _, b in pinned['lists'][10:12]]), lengths=[600, 300], n_hyp=8,
                                  seed=7, px_thr=2.5))
    assert_pairs(got, want, [0, 600, 900], 'px_thr')


@pytest.mark.parametrize('n_models', [1, 255, 256, 257])
def test_callers_models(gpu, pinned, n_models):
    """The ``models=`` route: models taken from the specification's solver, NaN models and an all-zero model among
    them; the scoring kernel, the selection and the decomposition on their own."""
    import imagematching_oetr_amd as pkg
    pairs = (2, 6, 9, 10, 12, 15)
    blocks = pinned['blocks'][list(pairs)]
    lists = [pinned['lists'][p] for p in pairs]
    models = np.stack([pinned['wants'][257][p]['models'][:n_models].copy() for p in pairs])      # NaN models among them
    if n_models > 1:
        models[:, n_models // 2] = 0.0                                   # all zero: finite, no inliers
        models[0, :] = np.nan                                            # a pair with no finite model
        assert np.isnan(models).any() and np.isfinite(models[1]).all(1).any()
    wants = pro.estimate_lists(blocks, lists, models=models)
    lengths = [len(k1) for k1, _ in lists]
    out = pkg.estimate_poses(blocks, np.concatenate([a for a, _ in lists]), np.concatenate([b for _, b in lists]),
                             lengths=lengths, models=models)
    assert out['n_models'] == n_models
    got = host(out)
    assert_pairs(got, wants, np.concatenate([[0], np.cumsum(lengths)]), n_models, models=False)
    if n_models > 1:
        assert got['counts'][0].tolist() == [lengths[0], 0, -1, 0, 0] and np.isnan(got['pose'][0]).all()
        assert (got['model_counts'][:, n_models // 2][1:] == 0).all()


def test_degenerate_lists(gpu):
    """Nine copies of one row, an EXACTLY collinear list, NaN keypoints: no model and no pose; collinear rows in
    general position (not exactly singular: a stated departure) give the specification's finite models, bit for bit."""
    import imagematching_oetr_amd as pkg
    cases = pro.degenerate_lists()
    names = ('copies', 'collinear_exact', 'collinear', 'nan')
    blocks = np.stack([cases[n][0] for n in names])
    lists = [cases[n][1:] for n in names]
    ids = np.array([1, 2, 0, 3], np.int32)                                # the collinear list as pair 0: the recorded one
    wants = pro.estimate_lists(blocks, lists, 16, 0, pair_ids=ids)
    out = pkg.estimate_poses(blocks, np.concatenate([a for a, _ in lists]), np.concatenate([b for _, b in lists]),
                             lengths=[9] * 4, n_hyp=16, seed=0, pair_ids=ids)
    got = host(out)
    assert_pairs(got, wants, [0, 9, 18, 27, 36], 'degenerate')
    for p in (0, 1, 3):
        assert got['counts'][p].tolist() == [9, 0, -1, 0, 0] and np.isnan(got['models'][p]).all()
        assert np.isnan(got['pose'][p]).all() and not got['inliers'][9 * p:9 * p + 9].any()
    assert got['counts'][2].tolist() == EXPECTED['degenerate']['collinear_counts'] and np.isfinite(got['pose'][2]).all()


def test_pair_ids_run_to_run_and_capture(gpu, pinned):
    import imagematching_oetr_amd as pkg
    n_hyp = 86
    lengths, bounds = pinned['lengths'], pinned['bounds']
    full = host(pkg.estimate_poses(pinned['params'], pinned['k1'], pinned['k2'], lengths=lengths, n_hyp=n_hyp,
                                   seed=pro.PINNED_SEED))
    # a permuted pair list with its ids: permuted, bit-equal results
    perm = np.random.default_rng(1).permutation(16)
    k1 = np.concatenate([pinned['lists'][p][0] for p in perm])
    k2 = np.concatenate([pinned['lists'][p][1] for p in perm])
    out = pkg.estimate_poses(pinned['blocks'][perm], k1, k2, lengths=[lengths[p] for p in perm], n_hyp=n_hyp,
                             seed=pro.PINNED_SEED, pair_ids=perm.astype(np.int32))
    got = host(out)
    at = np.concatenate([[0], np.cumsum([lengths[p] for p in perm])])
    for i, p in enumerate(perm):
        for k in ('model', 'pose', 'cosines', 'counts', 'models', 'model_counts'):
            assert mso.equal_bits(got[k][i], full[k][p]), (k, i, p)
        assert np.array_equal(got['inliers'][at[i]:at[i + 1]], full['inliers'][bounds[p]:bounds[p + 1]])
    # without the ids the samples follow the position
    plain = host(pkg.estimate_poses(pinned['blocks'][perm], k1, k2, lengths=[lengths[p] for p in perm], n_hyp=n_hyp,
                                    seed=pro.PINNED_SEED))
    assert not mso.equal_bits(plain['models'], got['models'])
    # run to run
    for _ in range(3):
        again = host(pkg.estimate_poses(pinned['params'], pinned['k1'], pinned['k2'], lengths=lengths, n_hyp=n_hyp,
                                        seed=pro.PINNED_SEED))
        assert_same(again, full, KEYS + ('models', 'model_counts'))
    # captured with default settings: device inputs only; a replay estimates what the buffers hold at replay time
    offsets = torch.from_numpy(bounds.astype(np.int32)).to(gpu)
    k1d, k2d = pinned['k1'].clone(), pinned['k2'].clone()
    out = pkg.estimate_poses(pinned['params'], k1d, k2d, offsets=offsets, n_hyp=n_hyp, seed=pro.PINNED_SEED)
    torch.cuda.synchronize(gpu)
    for k in KEYS:
        out[k].fill_(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.device(gpu):
        with torch.cuda.graph(graph):
            pkg.estimate_poses(pinned['params'], k1d, k2d, offsets=offsets, n_hyp=n_hyp, seed=pro.PINNED_SEED, out=out)
            with pytest.raises(ValueError, match='inside a graph capture'):
                pkg.estimate_poses(pinned['params'], k1d, k2d, lengths=lengths, n_hyp=n_hyp, out=out)
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert_same(host(out), full, KEYS + ('models', 'model_counts'))
        k1d.copy_(pinned['k1'].flip(0))                                   # other rows: other results on replay
        graph.replay()
        torch.cuda.synchronize(gpu)
    moved = host(out)
    assert not mso.equal_bits(moved['models'], full['models'])
    lists = []
    flipped = pinned['host_k'][0][::-1]
    for p in range(16):
        lists.append((flipped[bounds[p]:bounds[p + 1]], pinned['lists'][p][1]))
    for p in (4, 11):                      # two lists of the replay, specified (their models: no margins were drawn)
        want = pro.estimate(pinned['blocks'][p], *lists[p], n_hyp, pro.PINNED_SEED, 1.0, p)
        assert mso.equal_bits(moved['models'][p], want['models']) and moved['counts'][p][0] == want['counts'][0]
