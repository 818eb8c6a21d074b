"""GPU tests of the homography-estimation extension (``oetr_homography_ransac``, ``csrc/homography_ransac.hip``;
``homography_ransac.py``; ``evaluate.homography_errors`` / ``match_homography_auc``).  There is no tolerance anywhere:
every output - the workspace's models (NaN patterns included) and per-model counts, ``model``, ``H``, ``corner_sq``,
``counts``, ``inliers`` - is compared BIT FOR BIT (``mso.equal_bits``: NaN equals NaN whatever its payload) with the
float64 specification ``tests/homography_ransac_oracle.py``, whose pinned lists keep every inlier and acceptance
decision away from last-bit differences (asserted in ``tests/test_homography_ransac_cpu.py``).  The one assumption the
parity rests on - the device's float64 square root equals ``np.sqrt`` - is pinned by
``tests/test_gpu_pose_ransac.py::test_device_sqrt_is_numpys``.  The fixture is 16 lists, 3545 matches, at most 600
models per list."""
import json
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

pytestmark = pytest.mark.gpu
EXPECTED = json.loads((REPO / 'tests' / 'homography_ransac_expected.json').read_text())
KEYS = ('model', 'H', 'corner_sq', 'counts', 'inliers')
ALL = KEYS + ('models', 'model_counts')
SEED, THR = hro.PINNED_SEED, hro.PINNED_THR


def host(out):
    from imagematching_oetr_amd.homography_ransac import workspace_views
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
        for k in ('model', 'H', 'corner_sq'):
            assert mso.equal_bits(got[k][p], want[k]), (tag, p, k, got[k][p], want[k])
        assert got['counts'][p].tolist() == want['counts'].tolist(), (tag, p, got['counts'][p], want['counts'])
        if 'inliers' in got:
            assert np.array_equal(got['inliers'][lo:hi], want['inliers']), (tag, p, 'inliers')


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert mso.equal_bits(a[k], b[k]), k


def cat(lists):
    return np.concatenate([a for a, _ in lists]), np.concatenate([b for _, b in lists])


@pytest.fixture(scope='module')
def pinned(gpu):
    """The pinned lists and the device inputs: made once, shared, never modified.  ``want(n, r)``: the specified
    results at ``n_hyp`` n and ``refit_iters`` r, computed once each."""
    blocks, lists, _ = hro.pinned_call(EXPECTED['pinned']['draws'])
    assert [cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists] == EXPECTED['pinned']['kpts_sha256']
    assert cvo.sha(blocks) == EXPECTED['pinned']['blocks_sha256']        # a wrong input cannot pass as a wrong kernel
    lengths = [len(k1) for k1, _ in lists]
    k1, k2 = cat(lists)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    cache = {}

    def want(n, r, seed=SEED, thr=THR):
        key = (n, r, seed, thr)
        if key not in cache:
            cache[key] = hro.estimate_lists(blocks, lists, n, seed, thr, r)
        return cache[key]

    return dict(blocks=blocks, lists=lists, lengths=lengths, bounds=np.concatenate([[0], np.cumsum(lengths)]),
                params=t(blocks), k1=t(k1), k2=t(k2), host_k=(k1, k2), want=want)


def run(pinned, n_hyp, refit, **kw):
    import imagematching_oetr_amd as pkg
    kw.setdefault('seed', SEED)
    return pkg.estimate_homographies(pinned['params'], pinned['k1'], pinned['k2'], lengths=pinned['lengths'],
                                     n_hyp=n_hyp, px_thr=THR, refit_iters=refit, **kw)


@pytest.mark.parametrize('refit', hro.PINNED_REFITS)
@pytest.mark.parametrize('n_hyp', hro.PINNED_HYPOTHESES)
def test_pinned_call_equals_the_specification_and_the_fixture(gpu, pinned, n_hyp, refit):
    import imagematching_oetr_amd as pkg
    assert pinned['lengths'][:11] == [0, 3, 4, 5, 63, 64, 65, 255, 256, 257, 600] and len(pinned['lengths']) == 16
    out = run(pinned, n_hyp, refit)
    M = int(pinned['bounds'][-1])
    assert out['model'].dtype == torch.float64 and out['model'].shape == (16, 9) and out['model'].is_cuda
    assert out['H'].shape == (16, 9) and out['corner_sq'].shape == (16, 4)
    assert out['counts'].dtype == torch.int32 and out['counts'].shape == (16, 6)
    assert out['inliers'].dtype == torch.uint8 and out['inliers'].shape == (M,) and out['n_models'] == n_hyp
    got = host(out)
    wants = pinned['want'](n_hyp, refit)
    assert_pairs(got, wants, pinned['bounds'], (n_hyp, refit))
    records = EXPECTED['pinned']['n_hyp'][str(n_hyp)][str(refit)]
    assert got['counts'].tolist() == [rec['counts'] for rec in records]
    z, sha = (lambda a: np.nan_to_num(a, nan=-7.0)), (lambda a: cvo.sha(a)[:16])
    for p, rec in enumerate(records):
        lo, hi = pinned['bounds'][p], pinned['bounds'][p + 1]
        assert sha(z(got['models'][p])) == rec['models'] and sha(got['model_counts'][p]) == rec['model_counts'], p
        assert sha(z(got['model'][p])) == rec['model'] and sha(z(got['H'][p])) == rec['H'], p
        assert sha(z(got['corner_sq'][p])) == rec['corner_sq'] and sha(got['inliers'][lo:hi]) == rec['inliers'], p
        sel = got['counts'][p][2]
        if sel >= 0:
            assert sha(z(got['models'][p][sel])) == rec['selected'], p
    # lists of fewer than 4 rows: no homography
    for p in (0, 1):
        assert got['counts'][p].tolist() == [pinned['lengths'][p], 0, -1, 0, 0, 0]
        assert np.isnan(got['model'][p]).all() and np.isnan(got['H'][p]).all() and np.isnan(got['corner_sq'][p]).all()
    # the delivered model never has fewer inliers than the selected one, and marks exactly its inliers
    assert (got['counts'][:, 4] >= got['counts'][:, 3]).all() and (got['counts'][:, 5] <= refit).all()
    assert [int(got['inliers'][pinned['bounds'][p]:pinned['bounds'][p + 1]].sum()) for p in range(16)] \
        == got['counts'][:, 4].tolist()
    # the summary equals the specification's
    errs = pkg.homography_errors(out)
    spec = hro.homography_errors(np.stack([w['corner_sq'] for w in wants]), np.stack([w['counts'] for w in wants]))
    assert mso.equal_bits(errs, spec) and np.isinf(errs[:2]).all()
    auc = pkg.match_homography_auc(out)
    assert auc['auc'] == [100.0 * a for a in hro.homography_auc(spec)]
    assert auc['n_no_homography'] == int(np.isinf(spec).sum())


def test_host_inputs_offsets_float16_and_no_inliers(gpu, pinned):
    import imagematching_oetr_amd as pkg
    n_hyp, refit = 255, 2
    full = host(run(pinned, n_hyp, refit))
    # host arrays, uploaded
    got = host(pkg.estimate_homographies(pinned['blocks'], *pinned['host_k'], lengths=pinned['lengths'], n_hyp=n_hyp,
                                         px_thr=THR, refit_iters=refit, seed=SEED))
    assert_same(got, full, ALL)
    # inliers=False: the same everything else
    bare = run(pinned, n_hyp, refit, inliers=False)
    assert 'inliers' not in bare
    assert_same(host(bare), full, ('model', 'H', 'corner_sq', 'counts', 'models', 'model_counts'))
    # device offsets with rows in no list before the first and after the last list: 0 there, the lists as before;
    # the stale contents of a reused `out` are overwritten
    head, tail = 70, 67
    filler = lambda m: torch.full((m, 2), 3.0, device=gpu)
    k1 = torch.cat([filler(head), pinned['k1'], filler(tail)])
    k2 = torch.cat([filler(head), pinned['k2'], filler(tail)])
    offsets = torch.from_numpy((pinned['bounds'] + head).astype(np.int32)).to(gpu)
    kw = dict(offsets=offsets, n_hyp=n_hyp, px_thr=THR, refit_iters=refit, seed=SEED)
    out = pkg.estimate_homographies(pinned['params'], k1, k2, **kw)
    for k in KEYS:
        out[k].fill_(9)
    out['workspace'].fill_(0x5A)
    again = pkg.estimate_homographies(pinned['params'], k1, k2, out=out, **kw)
    assert again is out
    shifted = host(out)
    assert not shifted['inliers'][:head].any() and not shifted['inliers'][-tail:].any()
    shifted['inliers'] = shifted['inliers'][head:-tail]
    assert_same(shifted, full, ALL)
    # float16 keypoints are widened exactly
    h1, h2 = pinned['k1'].half(), pinned['k2'].half()
    kw = dict(lengths=pinned['lengths'], n_hyp=n_hyp, seed=3)
    a = host(pkg.estimate_homographies(pinned['params'], h1, h2, **kw))
    b = host(pkg.estimate_homographies(pinned['params'], h1.float(), h2.float(), **kw))
    assert_same(a, b, ALL)
    # another seed gives other samples; another threshold is the specification's at that threshold
    other = host(run(pinned, n_hyp, refit, seed=SEED + 1))
    assert not mso.equal_bits(other['models'], full['models'])
    want = hro.estimate_lists(pinned['blocks'][9:11], pinned['lists'][9:11], 8, 7, 5.5, 1)
    got = host(pkg.estimate_homographies(pinned['blocks'][9:11], *cat(pinned['lists'][9:11]), lengths=[257, 600],
                                         n_hyp=8, seed=7, px_thr=5.5, refit_iters=1))
    assert_pairs(got, want, [0, 257, 857], 'px_thr')


@pytest.mark.parametrize('n_models', [1, 255, 256, 257])
def test_callers_models(gpu, pinned, n_models):
    """The ``models=`` route: models taken from the specification's solver, NaN models and an all-zero model among
    them, a pair with no finite model and a pair with bad sizes; the scoring kernel, the selection and the refit on
    their own."""
    import imagematching_oetr_amd as pkg
    pairs = (4, 6, 9, 10, 12, 15)
    blocks = pinned['blocks'][list(pairs)].copy()
    lists = [pinned['lists'][p] for p in pairs]
    models = np.stack([pinned['want'](600, 0)[p]['models'][:n_models].copy() for p in pairs])    # NaN models among them
    if n_models > 1:
        models[:, n_models // 2] = 0.0                                   # all zero: finite, no inliers
        models[0, :] = np.nan                                            # a pair with no finite model
        blocks[2, 11] = 640.5                                            # a pair with bad sizes
        assert np.isnan(models).any() and np.isfinite(models[1]).all(1).any()
    wants = hro.estimate_lists(blocks, lists, px_thr=THR, refit_iters=2, models=models)
    lengths = [len(k1) for k1, _ in lists]
    out = pkg.estimate_homographies(blocks, *cat(lists), lengths=lengths, px_thr=THR, refit_iters=2, models=models)
    assert out['n_models'] == n_models
    got = host(out)
    assert_pairs(got, wants, np.concatenate([[0], np.cumsum(lengths)]), n_models, models=False)
    if n_models > 1:
        assert got['counts'][0].tolist() == [lengths[0], 0, -1, 0, 0, 0] and np.isnan(got['H'][0]).all()
        assert got['counts'][2].tolist() == [-1] * 6 and np.isnan(got['H'][2]).all()
        assert (got['model_counts'][2] == -1).all() and not got['inliers'][sum(lengths[:2]):sum(lengths[:3])].any()
        assert (got['model_counts'][:, n_models // 2][[1, 3, 4, 5]] == 0).all()
        assert (got['counts'][[1, 3, 4, 5], 2] >= 0).all()               # the other pairs unaffected


def test_degenerate_lists_and_the_refits_refusals(gpu):
    """The degenerate lists in one call: four copies of one row, a list of 3, NaN rows, an EXACTLY collinear list - no
    model; collinear rows in general position (not recognised: a stated departure) - the specification's counters.
    Then the refit's two refusals through ``models=``: a zero pivot, and a candidate with fewer inliers."""
    import imagematching_oetr_amd as pkg
    cases = hro.degenerate_lists()
    names = ('copies', 'three', 'nan', 'collinear_exact', 'collinear')
    blocks = np.stack([cases[n][0] for n in names])
    lists = [cases[n][1:] for n in names]
    ids = np.array([1, 2, 3, 4, 0], np.int32)                            # the collinear list as pair 0: the recorded one
    wants = hro.estimate_lists(blocks, lists, 16, 0, THR, 2, pair_ids=ids)
    lengths = [len(a) for a, _ in lists]
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    out = pkg.estimate_homographies(blocks, *cat(lists), lengths=lengths, n_hyp=16, seed=0, px_thr=THR, refit_iters=2,
                                    pair_ids=ids)
    got = host(out)
    assert_pairs(got, wants, bounds, 'degenerate')
    for p in range(4):
        assert got['counts'][p].tolist() == [lengths[p], 0, -1, 0, 0, 0] and np.isnan(got['models'][p]).all()
        assert np.isnan(got['H'][p]).all() and not got['inliers'][bounds[p]:bounds[p + 1]].any()
    assert got['counts'][4].tolist() == EXPECTED['degenerate']['collinear']
    for name, (P, k1, k2, M, thr) in hro.refit_cases().items():
        want = hro.estimate(P, k1, k2, px_thr=thr, models=M)
        got = host(pkg.estimate_homographies(P[None], k1, k2, lengths=[len(k1)], px_thr=thr, refit_iters=2,
                                             models=M[None]))
        assert_pairs(got, [want], [0, len(k1)], name, models=False)
        assert got['counts'][0].tolist() == EXPECTED['refit'][name]['counts'] and got['counts'][0][5] == 0
        assert mso.equal_bits(got['model'][0], M[0])                     # the minimal model stays


def test_pair_ids_run_to_run_and_capture(gpu, pinned):
    import imagematching_oetr_amd as pkg
    n_hyp, refit = 256, 2
    lengths, bounds = pinned['lengths'], pinned['bounds']
    full = host(run(pinned, n_hyp, refit))
    # a permuted pair list with its ids: permuted, bit-equal results
    perm = np.random.default_rng(1).permutation(16)
    k1, k2 = cat([pinned['lists'][p] for p in perm])
    kw = dict(lengths=[lengths[p] for p in perm], n_hyp=n_hyp, px_thr=THR, refit_iters=refit, seed=SEED)
    got = host(pkg.estimate_homographies(pinned['blocks'][perm], k1, k2, pair_ids=perm.astype(np.int32), **kw))
    at = np.concatenate([[0], np.cumsum([lengths[p] for p in perm])])
    for i, p in enumerate(perm):
        for k in ('model', 'H', 'corner_sq', 'counts', 'models', 'model_counts'):
            assert mso.equal_bits(got[k][i], full[k][p]), (k, i, p)
        assert np.array_equal(got['inliers'][at[i]:at[i + 1]], full['inliers'][bounds[p]:bounds[p + 1]])
    # without the ids the samples follow the position
    plain = host(pkg.estimate_homographies(pinned['blocks'][perm], k1, k2, **kw))
    assert not mso.equal_bits(plain['models'], got['models'])
    # run to run
    for _ in range(3):
        assert_same(host(run(pinned, n_hyp, refit)), full, ALL)
    # captured with default settings: device inputs only; a replay estimates what the buffers hold at replay time
    offsets = torch.from_numpy(bounds.astype(np.int32)).to(gpu)
    k1d, k2d = pinned['k1'].clone(), pinned['k2'].clone()
    kw = dict(n_hyp=n_hyp, px_thr=THR, refit_iters=refit, seed=SEED)
    out = pkg.estimate_homographies(pinned['params'], k1d, k2d, offsets=offsets, **kw)
    torch.cuda.synchronize(gpu)
    for k in KEYS:
        out[k].fill_(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.device(gpu):
        with torch.cuda.graph(graph):
            pkg.estimate_homographies(pinned['params'], k1d, k2d, offsets=offsets, out=out, **kw)
            with pytest.raises(ValueError, match='inside a graph capture'):
                pkg.estimate_homographies(pinned['params'], k1d, k2d, lengths=lengths, out=out, **kw)
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert_same(host(out), full, ALL)
        k1d.copy_(pinned['k1'].flip(0))                                   # other rows: other results on replay
        graph.replay()
        torch.cuda.synchronize(gpu)
    moved = host(out)
    assert not mso.equal_bits(moved['models'], full['models'])
    flipped = pinned['host_k'][0][::-1]
    for p in (4, 11):                      # two lists of the replay, specified (their models: no margins were drawn)
        want = hro.estimate(pinned['blocks'][p], flipped[bounds[p]:bounds[p + 1]], pinned['lists'][p][1], n_hyp, SEED,
                            THR, refit, p)
        assert mso.equal_bits(moved['models'][p], want['models']) and moved['counts'][p][0] == want['counts'][0]


def test_more_pairs_than_one_grid_dimension(gpu):
    """65 538 pairs of 5-row lists at n_hyp 4 in one call: six distinct lists repeated, each pair named to the sampler
    by its list (``pair_ids = p % 6``), so six specified results cover every pair."""
    import imagematching_oetr_amd as pkg
    n, kinds = 65538, 6
    scenes = [hro.make_scene(5, seed=700 + i, noise=0.2 * (i % 2)) for i in range(kinds)]
    wants = [hro.estimate(P, k1, k2, 4, 5, THR, 2, i) for i, (P, k1, k2, _) in enumerate(scenes)]
    assert any(w['counts'][2] >= 0 for w in wants)
    reps = -(-n // kinds)
    tile = lambda a: np.concatenate([a] * reps)[:n * (len(a) // kinds)]
    blocks = tile(np.stack([s[0] for s in scenes]))
    k1, k2 = tile(np.concatenate([s[1] for s in scenes])), tile(np.concatenate([s[2] for s in scenes]))
    ids = (np.arange(n) % kinds).astype(np.int32)
    out = pkg.estimate_homographies(blocks, k1, k2, lengths=[5] * n, n_hyp=4, seed=5, px_thr=THR, refit_iters=2,
                                    pair_ids=ids)
    got = host(out)
    for k in ('model', 'H', 'corner_sq', 'counts', 'models', 'model_counts'):
        assert mso.equal_bits(got[k], tile(np.stack([w[k] for w in wants]))), k
    assert np.array_equal(got['inliers'], tile(np.concatenate([w['inliers'] for w in wants])))


def test_delivered_homography_feeds_the_planar_entries_unchanged(gpu, pinned):
    """``H`` as delivered goes into ``score_matches_homography`` and ``overlap_boxes_from_homography``; both agree with
    their own oracles on that ``H``."""
    import imagematching_oetr_amd as pkg
    pairs = [6, 10, 11]
    lists = [pinned['lists'][p] for p in pairs]
    lengths = [len(a) for a, _ in lists]
    k1, k2 = cat(lists)
    out = pkg.estimate_homographies(pinned['blocks'][pairs], k1, k2, lengths=lengths, n_hyp=64, px_thr=THR, seed=SEED)
    H = out['H'].reshape(-1, 3, 3)
    assert torch.isfinite(H).all().item()
    scored = pkg.score_matches_homography(H, k1, k2, lengths=lengths)
    size = (48, 64)                                                       # small pictures: the boxes are per pixel
    scale = (640 / 64, 480 / 48)
    small = pkg.rescale_homography(H, scale, scale)
    boxes = pkg.overlap_boxes_from_homography(small, size, size)
    Hh, sh = H.cpu().numpy(), small.cpu().numpy()
    dist, counts = scored['dist_sq'].cpu().numpy(), scored['counts'].cpu().numpy()
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    inl = out['inliers'].cpu().numpy().astype(bool)
    for i, (a, b) in enumerate(lists):
        want = hmo.score(Hh[i], a, b)
        assert mso.equal_bits(dist[bounds[i]:bounds[i + 1]], want['dist_sq']) and counts[i].tolist() == want['counts'].tolist()
        assert (dist[bounds[i]:bounds[i + 1]][inl[bounds[i]:bounds[i + 1]]] < THR * THR * 1.01).all()   # the same rows
        box = hmo.overlap_box(sh[i], 64, 48, 64, 48)
        assert boxes['overlap_count'][i].item() == box['count'] > 0
        assert boxes['overlap_box1'][i].cpu().numpy().astype(np.int64).tolist() == box['box1'].tolist()
        assert boxes['overlap_box2'][i].cpu().numpy().astype(np.int64).tolist() == box['box2'].tolist()
