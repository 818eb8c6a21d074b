"""GPU tests of the keypoint-repeatability extension (``oetr_keypoint_repeatability``, ``csrc/keypoint_score.hip``;
``keypoint_score.py``; ``evaluate.keypoint_repeatability``).  There is no tolerance anywhere: counters and nearest
neighbours are compared for equality and every distance BIT FOR BIT (``mso.equal_bits``: NaN equals NaN whatever its
payload) with the float64 restatement ``tests/keypoint_score_oracle.py``, whose pinned sets keep every distance >= 1e-6
relative from every threshold and every coordinate off a ``.5`` tie (asserted in ``tests/test_keypoint_score_cpu.py``).
The kernel's query tile and its LDS target tile are 256 keypoints, its wave 64: the pinned counts 63 / 64 / 65 and
255 / 256 / 257 straddle them by one on each side, as sources and as targets; 511 / 512 / 513 the second tile.  The
whole fixture is 48 pairs over 12 pictures of at most 600 keypoints and 56 x 56 pixels."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import keypoint_score_oracle as kso  # noqa: E402
import match_score_oracle as mso  # noqa: E402

pytestmark = pytest.mark.gpu
EXPECTED = json.loads((REPO / 'tests' / 'keypoint_score_expected.json').read_text())
THR = tuple(EXPECTED['thresholds'])
KEYS = ('counts', 'nearest', 'dist_sq')


def depth_set(gpu, views):
    import imagematching_oetr_amd as pkg
    ds = pkg.DepthSet(gpu)
    for k, v in enumerate(views):
        assert ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose']) == k
    return ds


def host(out):
    return {k: out[k].cpu().numpy() for k in KEYS if k in out}


def restate(views, kps, pairs, blocks, max_kp, thresholds=THR):
    """The restatement of a pair list over the slots ``views`` / ``kps`` -> (results, the device's layout of them)."""
    results = [kso.score(views[i]['depth'], views[j]['depth'], blocks[p], kps[i], kps[j], thresholds)
               for p, (i, j) in enumerate(pairs)]
    return results, dict(zip(KEYS, kso.padded(results, max_kp)))


def assert_same(a, b, keys=KEYS, tag=None):
    for k in keys:
        assert a[k].shape == b[k].shape and mso.equal_bits(a[k], b[k]), (tag, k)


def concatenated(kps, gpu):
    """-> (cat float32 [N,2], kp_offsets int32 [n+1]) on the device."""
    cat = torch.from_numpy(np.concatenate(kps).astype(np.float32).reshape(-1, 2)).to(gpu)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.int32)).to(gpu)
    return cat, offsets


@pytest.fixture(scope='module')
def pinned(gpu):
    """The fixture's scene and its three keypoint sets as ONE set of 12 pictures (slot 4 s + k: view k with the
    keypoints of set s), their restated results, and the ONE call that scores all 48 pairs with the restatement's
    parameter blocks: computed once, shared, never modified."""
    import imagematching_oetr_amd as pkg
    scene = mso.make_scene(tuple(tuple(s) for s in EXPECTED['sizes']), EXPECTED['seed'])
    assert [cvo.sha(v['depth']) for v in scene] == EXPECTED['depth_sha256']
    views, kps, pairs = [], [], []
    for s, rec in enumerate(EXPECTED['sets']):
        sets = kso.make_keypoints(scene, rec['counts'], rec['seed'])
        assert [cvo.sha(k) for k in sets] == rec['kpts_sha256']          # the inputs first
        views += scene
        kps += sets
        pairs += [(4 * s + i, 4 * s + j) for i, j in kso.PAIRS]
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in pairs])
    assert [cvo.sha(b) for b in blocks[:16]] == EXPECTED['params_sha256']
    results, want = restate(views, kps, pairs, blocks, 600)
    ds = depth_set(gpu, views)
    dev_kps = [torch.from_numpy(k).to(gpu) for k in kps]
    out = pkg.score_keypoints(ds, pairs, dev_kps, THR, params=blocks)
    torch.cuda.synchronize()
    return dict(scene=scene, views=views, kps=kps, pairs=pairs, blocks=blocks, results=results, want=want, ds=ds,
                dev_kps=dev_kps, out=out, got=host(out))


def test_pinned_pairs_equal_the_restatement_and_the_fixture(pinned):
    out, got, want = pinned['out'], pinned['got'], pinned['want']
    assert out['counts'].dtype == torch.int32 and out['counts'].shape == (48, 2, 6) and out['counts'].is_cuda
    assert out['nearest'].dtype == torch.int32 and out['nearest'].shape == (48, 2, 600)
    assert out['dist_sq'].dtype == torch.float64 and out['dist_sq'].shape == (48, 2, 600) and out['thresholds'] == THR
    for p in range(48):                                                          # pair by pair, for the message
        for k in KEYS:
            assert mso.equal_bits(got[k][p], want[k][p]), (p, pinned['pairs'][p], k)
    assert got['counts'].tolist() == [p['counts'] for s in EXPECTED['sets'] for p in s['pairs']]
    sizes = {tuple(pinned['views'][i]['depth'].shape) for i, _ in pinned['pairs']}
    assert {(1, 1), (7, 5)} <= sizes and sum(i == j for i, j in pinned['pairs']) == 12       # small maps, self pairs
    # rows past a picture's count, and what the tests below rely on: kept rows, +inf rows, ties
    n_src = got['counts'][:, :, 0]
    for p in range(48):
        for s in range(2):
            assert (got['nearest'][p, s, n_src[p, s]:] == -1).all() and np.isnan(got['dist_sq'][p, s, n_src[p, s]:]).all()
    assert np.isposinf(got['dist_sq']).sum() > 20 and (got['nearest'] >= 0).sum() > 3000


def test_counts_around_the_second_tile(gpu, pinned):
    """511 / 512 / 513 keypoints, as sources (the third query tile begins at 512) and as targets (the third LDS tile)."""
    import imagematching_oetr_amd as pkg
    scene = pinned['scene']
    views = [scene[2], scene[3], scene[2], scene[1]]
    counts = (511, 512, 513, 600)
    kps, _, _, (thr, tie) = kso.draw_set(views, counts, 300)
    assert thr >= kso.MIN_THRESHOLD_MARGIN and tie >= kso.MIN_TIE_MARGIN
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in kso.PAIRS])
    _, want = restate(views, kps, kso.PAIRS, blocks, 600)
    out = pkg.score_keypoints(depth_set(gpu, views), list(kso.PAIRS), kps, THR, params=blocks)       # host keypoints
    got = host(out)
    assert out['nearest'].shape == (16, 2, 600)
    assert (want['nearest'] >= 512).any() and (want['nearest'][:, :, 512:] >= 0).any()      # both third tiles are used
    for p in range(16):
        for k in KEYS:
            assert mso.equal_bits(got[k][p], want[k][p]), (p, kso.PAIRS[p], k)


def test_depth_set_route_with_the_devices_own_blocks(pinned):
    """``params=None``: the blocks come from the set's cameras (``match_params``); restated with those very blocks,
    everything is equal - self pairs, whose ``t`` is a rounding residue, included."""
    import imagematching_oetr_amd as pkg
    ds = pinned['ds']
    index = torch.tensor(pinned['pairs'], dtype=torch.int32, device=ds.device)
    blocks = pkg.match_params(ds, index[:, 0].contiguous(), index[:, 1].contiguous()).cpu().numpy()
    assert blocks.shape == (48, 20) and np.allclose(blocks, pinned['blocks'], rtol=1e-9, atol=1e-9)
    got = host(pkg.score_keypoints(ds, index, pinned['dev_kps'], THR))
    _, want = restate(pinned['views'], pinned['kps'], pinned['pairs'], blocks, 600)
    assert_same(got, want, tag='depth set')


def test_pairs_that_are_not_vouched_for(gpu, pinned):
    """Indices -1 and ``len(ds)`` among good pairs: -1 / NaN rows, every counter -1; a picture over ``max_kp`` leaves
    its pairs at -1; every other pair is what it is in the plain call."""
    import imagematching_oetr_amd as pkg
    ds, n = pinned['ds'], len(pinned['ds'])
    assert n == 12
    bad = {2: (-1, 2), 5: (2, n), 9: (n, -1), 20: (1 << 30, 0), 47: (-(1 << 31), -(1 << 31))}
    pairs = [bad.get(p, pair) for p, pair in enumerate(pinned['pairs'])]
    got = host(pkg.score_keypoints(ds, pairs, pinned['dev_kps'], THR, params=pinned['blocks']))
    for p in range(48):
        if p in bad:
            assert (got['counts'][p] == -1).all() and (got['nearest'][p] == -1).all() and np.isnan(got['dist_sq'][p]).all(), p
        else:
            for k in KEYS:
                assert mso.equal_bits(got[k][p], pinned['got'][k][p]), (p, k)
    summary = pkg.keypoint_repeatability({'counts': torch.from_numpy(got['counts'])})
    assert (summary['n_pairs'], summary['n_not_scored']) == (43, 5)
    # max_kp = 300 vouches for no picture of 600 keypoints: slots 2, 11
    cat, offsets = concatenated(pinned['kps'], gpu)
    out = pkg.score_keypoints(ds, pinned['pairs'], (cat, offsets, 300), THR, params=pinned['blocks'])
    got = host(out)
    assert out['nearest'].shape == (48, 2, 300)
    over = [p for p, (i, j) in enumerate(pinned['pairs']) if len(pinned['kps'][i]) > 300 or len(pinned['kps'][j]) > 300]
    assert len(over) == 14
    for p in range(48):
        if p in over:
            assert (got['counts'][p] == -1).all() and (got['nearest'][p] == -1).all() and np.isnan(got['dist_sq'][p]).all(), p
        else:
            assert got['counts'][p].tolist() == pinned['got']['counts'][p].tolist(), p
            assert mso.equal_bits(got['nearest'][p], pinned['got']['nearest'][p, :, :300]), p
            assert mso.equal_bits(got['dist_sq'][p], pinned['got']['dist_sq'][p, :, :300]), p
    # offsets that point outside the keypoint array: the pictures that own such rows are not vouched for
    broken = offsets.clone()
    broken[3] = -5                                                   # picture 2 would begin, picture 1... end before 0
    broken[12] = cat.shape[0] + 1                                    # picture 11 would end past the array
    got = host(pkg.score_keypoints(ds, pinned['pairs'], (cat, broken, 600), THR, params=pinned['blocks']))
    for p, (i, j) in enumerate(pinned['pairs']):
        if {i, j} & {2, 3, 11}:                                      # 2: negative count, 3: begins below 0, 11: ends past N
            assert (got['counts'][p] == -1).all() and (got['nearest'][p] == -1).all(), p
        else:
            assert_same({k: got[k][p] for k in KEYS}, {k: pinned['got'][k][p] for k in KEYS}, tag=p)


def test_runs_are_identical_and_do_not_depend_on_the_order_of_the_list(pinned):
    import imagematching_oetr_amd as pkg
    ds = pinned['ds']
    again = host(pkg.score_keypoints(ds, pinned['pairs'], pinned['dev_kps'], THR, params=pinned['blocks']))
    assert_same(again, pinned['got'])
    assert np.array_equal(again['dist_sq'].view(np.uint64), pinned['got']['dist_sq'].view(np.uint64))   # NaN payloads too
    order = np.random.default_rng(4).permutation(48)
    got = host(pkg.score_keypoints(ds, [pinned['pairs'][k] for k in order], pinned['dev_kps'], THR,
                                   params=pinned['blocks'][order]))
    for k in KEYS:
        assert np.array_equal(got[k].view(np.uint64 if k == 'dist_sq' else got[k].dtype),
                              pinned['got'][k][order].view(np.uint64 if k == 'dist_sq' else got[k].dtype)), k


def test_counters_only_float16_out_reuse_and_thresholds(gpu, pinned):
    import imagematching_oetr_amd as pkg
    ds, pairs, blocks = pinned['ds'], pinned['pairs'], pinned['blocks']
    bare = pkg.score_keypoints(ds, pairs, pinned['dev_kps'], THR, nearest=False, params=blocks)
    assert sorted(k for k in bare if not k.startswith('_')) == ['counts', 'thresholds']
    assert_same(host(bare), pinned['got'], ('counts',))
    # out= is written into again: same storage, same result
    out = pkg.score_keypoints(ds, pairs, pinned['dev_kps'], THR, params=blocks)
    ptrs = {k: out[k].data_ptr() for k in KEYS}
    for k in KEYS:
        out[k].fill_(1)
    assert pkg.score_keypoints(ds, pairs, pinned['dev_kps'], THR, params=blocks, out=out) is out
    assert {k: out[k].data_ptr() for k in KEYS} == ptrs
    assert_same(host(out), pinned['got'])
    with pytest.raises(ValueError, match='other sizes'):
        pkg.score_keypoints(ds, pairs[:3], pinned['dev_kps'], THR, params=blocks[:3], out=out)
    with pytest.raises(ValueError, match='other sizes'):
        pkg.score_keypoints(ds, pairs, pinned['dev_kps'], THR[:2], params=blocks, out=out)
    with pytest.raises(ValueError, match='12 depth maps'):
        pkg.score_keypoints(ds, pairs, pinned['dev_kps'][:5], THR)
    # other thresholds: eight, none, and a NaN one that counts nothing
    eight = (0.5, 1, 2, 3, 5, 8, float('nan'), 1e6)
    got = host(pkg.score_keypoints(ds, pairs[16:32], pinned['dev_kps'], eight, params=blocks[16:32]))
    _, want = restate(pinned['views'], pinned['kps'], pairs[16:32], blocks[16:32], 600, eight)
    assert_same(got, want, tag='eight thresholds')
    assert (got['counts'][:, :, 8] == 0).all() and got['counts'].shape == (16, 2, 10) and got['counts'][:, :, 9].sum() > 0
    none = pkg.score_keypoints(ds, pairs, pinned['dev_kps'], (), params=blocks)
    assert none['counts'].shape == (48, 2, 2) and np.array_equal(none['counts'].cpu().numpy(), pinned['got']['counts'][:, :, :2])
    assert mso.equal_bits(none['dist_sq'].cpu().numpy(), pinned['got']['dist_sq'])
    # float16 keypoints are widened: the score of the float32 keypoints of the same values, and the restatement's
    half = [k.half() for k in pinned['dev_kps'][8:12]]
    idx = [(i, j) for i, j in kso.PAIRS]
    sub = depth_set(gpu, pinned['scene'])
    a = host(pkg.score_keypoints(sub, idx, half, THR, params=blocks[:16]))
    b = host(pkg.score_keypoints(sub, idx, [k.float() for k in half], THR, params=blocks[:16]))
    assert_same(a, b, tag='float16')
    _, want = restate(pinned['scene'], [k.cpu().numpy() for k in half], idx, blocks[:16], 600)
    assert_same(a, want, tag='float16 restated')


def test_empty_calls(gpu, pinned):
    import imagematching_oetr_amd as pkg
    ds = pinned['ds']
    out = pkg.score_keypoints(ds, [], pinned['dev_kps'], THR)
    assert out['counts'].shape == (0, 2, 6) and out['nearest'].shape == (0, 2, 600) and out['dist_sq'].shape == (0, 2, 600)
    none = [torch.zeros(0, 2, device=gpu)] * 12
    out = pkg.score_keypoints(ds, pinned['pairs'][:3] + [(-1, 0)], none, THR)
    assert out['counts'].tolist() == [[[0] * 6] * 2] * 3 + [[[-1] * 6] * 2]
    assert out['nearest'].shape == (4, 2, 0) and out['dist_sq'].shape == (4, 2, 0)
    assert pkg.ground_truth_matches(out, 3.0).shape == (4, 0)
    summary = pkg.keypoint_repeatability(out)
    assert summary['repeatability'][:3].tolist() == [[0.0] * 4] * 3 and (summary['n_pairs'], summary['n_not_scored']) == (3, 1)
    # pictures 4 .. 7 are the set with an EMPTY picture (slot 4): -1 / +inf towards it, nothing from it
    got = pinned['got']
    p = pinned['pairs'].index((5, 4))
    kept = got['counts'][p, 0, 1]
    assert got['counts'][p].tolist() == [[64, kept, 0, 0, 0, 0], [0] * 6] and kept > 0
    assert np.isposinf(got['dist_sq'][p, 0]).sum() == kept and (got['nearest'][p] == -1).all()


def test_the_call_is_captured_and_replayed_on_new_keypoints_offsets_and_pairs(gpu, pinned):
    """Enqueue-only, no host read: captured with default settings; a replay scores what the keypoint, offset and
    pair tensors hold at replay time."""
    import imagematching_oetr_amd as pkg
    ds, views = pinned['ds'], pinned['views']
    cat, offsets = concatenated(pinned['kps'], gpu)
    index = torch.tensor(pinned['pairs'], dtype=torch.int32, device=gpu)
    first = host(pkg.score_keypoints(ds, index, (cat, offsets, 600), THR))       # also uploads the table
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.score_keypoints(ds, index, (cat, offsets, 600), THR)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(host(captured), first)
    # other keypoints (the sets drawn again, their counts moved on by one set), other offsets, the pair list reversed
    kps = []
    for s in range(3):
        kps += kso.make_keypoints(pinned['scene'], kso.COUNTS[(s + 1) % 3], 700 + s)
    assert sum(len(k) for k in kps) == cat.shape[0] and [len(k) for k in kps] != [len(k) for k in pinned['kps']]
    new_cat, new_offsets = concatenated(kps, gpu)
    pairs = pinned['pairs'][::-1]
    cat.copy_(new_cat)
    offsets.copy_(new_offsets)
    index.copy_(torch.tensor(pairs, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    replayed = host(captured)
    fresh = host(pkg.score_keypoints(ds, pairs, [torch.from_numpy(k).to(gpu) for k in kps], THR))
    assert_same(replayed, fresh, tag='replay')
    blocks = pkg.match_params(ds, index[:, 0].contiguous(), index[:, 1].contiguous()).cpu().numpy()
    _, want = restate(views, kps, pairs, blocks, 600)
    assert_same(replayed, want, ('nearest', 'dist_sq'), tag='replay restated')    # no margin was drawn for these sets
    assert not np.array_equal(replayed['counts'], first['counts'])


def test_ground_truth_matches_against_a_numpy_mutual_check(pinned):
    import imagematching_oetr_amd as pkg
    near, dist = pinned['want']['nearest'], pinned['want']['dist_sq']
    for px in (1.0, 3.0):
        got = pkg.ground_truth_matches(pinned['out'], px)
        assert got.dtype == torch.int32 and got.shape == (48, 600) and got.is_cuda
        want = np.full((48, 600), -1, np.int32)
        for p in range(48):
            for a in range(600):
                b = near[p, 0, a]
                if b >= 0 and near[p, 1, b] == a and dist[p, 0, a] < px * px and dist[p, 1, b] < px * px:
                    want[p, a] = b
        assert np.array_equal(got.cpu().numpy(), want), px
        assert (want >= 0).sum() > 500
    # a match list is a permutation of part of both sides: no target is matched twice
    for row in want:
        hit = row[row >= 0]
        assert len(np.unique(hit)) == len(hit)


def test_keypoint_repeatability_of_the_pinned_call(pinned):
    import imagematching_oetr_amd as pkg
    res = pkg.keypoint_repeatability(pinned['out'])
    want = kso.repeatability(pinned['want']['counts'])
    assert np.array_equal(res['repeatability'], want) and np.array_equal(res['mean_repeatability'], want.mean(0))
    assert res['thresholds'] == THR and (res['n_pairs'], res['n_not_scored']) == (48, 0)


def test_score_keypoints_refuses_malformed_inputs(gpu, pinned):
    import imagematching_oetr_amd as pkg
    ds, pairs = pinned['ds'], pinned['pairs'][:2]
    cat, offsets = concatenated(pinned['kps'], gpu)
    for keypoints, message in (((cat.cpu(), offsets, 600), 'device tensors'), ((cat, offsets.cpu(), 600), 'device tensors'),
                               ((cat.half(), offsets, 600), 'must be float32'), ((cat, offsets, -1), 'max_kp must be >= 0'),
                               ((cat, offsets[:-1], 600), r'keypoints\[1\] must be'), ((cat, offsets.long(), 600), r'keypoints\[1\] must be'),
                               ((cat.reshape(-1), offsets, 600), r'must be \[M,2\]'),
                               ([k.reshape(-1) for k in pinned['dev_kps']], r'must be \[M,2\]'),
                               ([k.long() for k in pinned['dev_kps']], 'float32 or float16')):
        with pytest.raises(ValueError, match=message):
            pkg.score_keypoints(ds, pairs, keypoints, THR)
    with pytest.raises(ValueError, match='int32'):
        pkg.score_keypoints(ds, torch.tensor(pairs, device=gpu), pinned['dev_kps'], THR)            # int64 pairs
    with pytest.raises(ValueError, match='params must be'):
        pkg.score_keypoints(ds, pairs, pinned['dev_kps'], THR, params=torch.from_numpy(pinned['blocks'][:2, :19].copy()).to(gpu))
    with pytest.raises(ValueError, match='at most 8'):
        pkg.score_keypoints(ds, pairs, pinned['dev_kps'], range(9))
