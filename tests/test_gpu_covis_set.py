"""GPU tests of the depth-map-set extension (``oetr_covis_boxes_indexed`` / ``oetr_covis_select``,
``csrc/covis.hip``; ``covis_set.py``; ``evaluate.evaluate_indexed``).  Boxes, valid and count are integers and are
compared for EQUALITY with the float64 restatement (``tests/covis_set_oracle.py``): every ordered pair of every set
has a decision margin >= 1e-9 (the set is re-drawn until it has; no pair is left out), and a self pair - whose
margin is zero by construction - is restated with the very ``T`` the device used."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import covis_set_oracle as cso  # noqa: E402

pytestmark = pytest.mark.gpu
# the mixed set plus a 1 x 1 map, 41 x 50 = 2050 pixels (one full workgroup of 2048 and 2) and 64 x 64 (exactly two)
SIZES = cso.SIZES + ((1, 1), (41, 50), (64, 64))
KEYS = ('overlap_box1', 'overlap_box2', 'overlap_valid', 'overlap_count')


@functools.lru_cache(maxsize=None)
def the_set(sizes=SIZES, seed=0):
    """(views, restated results of all ordered pairs): computed once, shared, never modified."""
    return cso.checked_set(sizes, seed)


def depth_set(gpu, views):
    import imagematching_oetr_amd as pkg
    ds = pkg.DepthSet(gpu)
    for k, v in enumerate(views):
        assert ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose'], v['bbox'], v['ratio']) == k
    return ds


def host(out):
    return {k: out[k].cpu().numpy() for k in KEYS}


def assert_pair(got, p, e, tag=None):
    assert np.array_equal(got['overlap_box1'][p], np.asarray(e['box1'], np.float32)), (tag, p, got['overlap_box1'][p], e['box1'])
    assert np.array_equal(got['overlap_box2'][p], np.asarray(e['box2'], np.float32)), (tag, p, got['overlap_box2'][p], e['box2'])
    assert bool(got['overlap_valid'][p]) == bool(e['valid']) and int(got['overlap_count'][p]) == int(e['count']), \
        (tag, p, got['overlap_count'][p], e['count'])


def assert_same(a, b):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


def test_all_ordered_pairs_and_self_pairs_equal_the_restatement(gpu):
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd.covis_set import pair_params
    views, results = the_set()
    ds = depth_set(gpu, views)
    assert len(ds) == 9 and ds.max_pixels == 64 * 64 and ds.shape(7) == (41, 50)
    pairs = sorted(results) + [(i, i) for i in range(len(views))]
    out = pkg.overlap_boxes_indexed(ds, pairs)
    assert sorted(k for k in out if k != 'workspace') == sorted(KEYS)
    assert out['overlap_box1'].dtype == torch.float32 and out['overlap_valid'].dtype == torch.bool
    assert out['overlap_count'].dtype == torch.int32 and out['overlap_box1'].device.type == 'cuda'
    got = host(out)
    for p, pair in enumerate(sorted(results)):
        assert results[pair]['margin'] >= cso.MIN_MARGIN
        assert_pair(got, p, results[pair], pair)
    assert sum(bool(v) for v in got['overlap_valid'][:len(results)]) == sum(r['valid'] for r in results.values()) > 40
    # self pairs, with the device's own T
    idx = torch.arange(len(views), dtype=torch.int32, device=gpu)
    T = pair_params(ds, idx, idx)[:, :16].cpu().numpy().reshape(-1, 4, 4)
    for i in range(len(views)):
        e = cso.restate_pair(views, i, i, T=T[i])
        assert_pair(got, len(results) + i, e, ('self', i))
    assert int(got['overlap_count'][len(results) + 5]) > 2000        # a self pair sees nearly every pixel with depth


def test_pinned_square_scenes_through_the_indexed_entry(gpu):
    """The six scenes of ``tests/covis_expected.json`` (the reference's results), two slots each, one set of six
    sizes, one call."""
    import imagematching_oetr_amd as pkg
    pinned = json.loads((REPO / 'tests' / 'covis_expected.json').read_text())['scenes']
    ds = pkg.DepthSet(gpu)
    for e in pinned:
        scene, _ = cvo.checked_scene(e['kind'], e['size'], e['size'], e['seed'])
        assert cvo.sha(scene['depth1']) == e['depth1_sha256'] and cvo.sha(scene['depth2']) == e['depth2_sha256']
        for s in ('1', '2'):
            ds.add(torch.from_numpy(scene['depth' + s]), scene['intrinsics' + s], scene['pose' + s], scene['bbox' + s],
                   scene['ratio' + s])
    assert len(pinned) == 6 and len({ds.shape(2 * k) for k in range(6)}) == 6
    got = host(pkg.overlap_boxes_indexed(ds, [(2 * k, 2 * k + 1) for k in range(6)]))
    for k, e in enumerate(pinned):
        assert_pair(got, k, e, e['kind'])


def test_equal_size_subset_equals_the_stacked_entry_bit_for_bit(gpu):
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd.covis import covis_boxes
    from imagematching_oetr_amd.covis_set import pair_params
    views, results = the_set(((56, 56),) * 4, 5)
    ds = depth_set(gpu, views)
    pairs = torch.tensor(sorted(results) + [(2, 2)], dtype=torch.int32, device=gpu)
    out = pkg.overlap_boxes_indexed(ds, pairs)
    stacked = torch.stack([torch.from_numpy(v['depth']) for v in views]).to(gpu)
    idx1, idx2 = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    ref = covis_boxes(stacked.index_select(0, idx1.long()).contiguous(), stacked.index_select(0, idx2.long()).contiguous(),
                      pair_params(ds, idx1, idx2))
    assert_same(out, ref)
    assert int(out['overlap_count'].min()) > 0
    got = host(out)
    for p, pair in enumerate(sorted(results)):
        assert_pair(got, p, results[pair], pair)


def test_result_does_not_depend_on_pair_order_or_duplicates(gpu):
    import imagematching_oetr_amd as pkg
    views, results = the_set()
    ds = depth_set(gpu, views)
    pairs = sorted(results)
    base = host(pkg.overlap_boxes_indexed(ds, pairs))
    order = np.random.default_rng(3).permutation(len(pairs))
    shuffled = [pairs[k] for k in order] + [pairs[0]] * 5 + [pairs[7], pairs[7]]
    got = host(pkg.overlap_boxes_indexed(ds, shuffled))
    src = list(order) + [0] * 5 + [7, 7]
    for k in KEYS:
        assert np.array_equal(got[k], base[k][src]), k


def _table_with(ds, gpu, edit):
    """The set's device table with ``edit(rows)`` applied on a host copy (a ctypes array of ``oetr_covis_map``)."""
    from imagematching_oetr_amd.hip_engine import _CovisMap
    table, _ = ds._commit()
    rows = (_CovisMap * len(ds)).from_buffer_copy(table.cpu().numpy().tobytes())
    edit(rows)
    return torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(gpu)


def test_pairs_that_must_not_be_dereferenced(gpu):
    """Index -1 or n_maps, a NULL map, H = 0, H * W > max_pixels: zero boxes, valid 0, count -1; every other pair
    of the call is what it is without them."""
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd.covis_set import covis_boxes_indexed, pair_params
    views, results = the_set()
    ds = depth_set(gpu, views)
    n = len(views)
    good = sorted(results)
    base = host(pkg.overlap_boxes_indexed(ds, good))

    def check(got, pairs, bad):
        assert any(bad) and not all(bad)
        for p, pair in enumerate(pairs):
            if bad[p]:
                assert int(got['overlap_count'][p]) == -1 and not got['overlap_valid'][p], (p, pair)
                assert not got['overlap_box1'][p].any() and not got['overlap_box2'][p].any(), (p, pair)
            else:
                q = good.index(pair)
                for k in KEYS:
                    assert np.array_equal(got[k][p], base[k][q]), (k, p, pair)

    # indices outside the set, through the public entry, between good neighbours
    pairs = [good[0], (-1, 2), good[1], (2, n), (n, -1), good[2], (0, 1 << 20), good[3]]
    check(host(pkg.overlap_boxes_indexed(ds, pairs)), pairs, [not (0 <= i < n and 0 <= j < n) for i, j in pairs])
    # a NULL map and a map with H = 0 in the table; a max_pixels below two of the maps
    pairs_t = torch.tensor(good, dtype=torch.int32, device=gpu)
    idx1, idx2 = pairs_t[:, 0].contiguous(), pairs_t[:, 1].contiguous()
    params = pair_params(ds, idx1, idx2)

    def edit(rows):
        rows[2].depth = None
        rows[3].H = 0
    got = host(covis_boxes_indexed(_table_with(ds, gpu, edit), n, ds.max_pixels, idx1, idx2, params))
    check(got, good, [2 in pair or 3 in pair for pair in good])

    def edit_w(rows):
        rows[0].W = 8193
    got = host(covis_boxes_indexed(_table_with(ds, gpu, edit_w), n, ds.max_pixels, idx1, idx2, params))
    check(got, good, [0 in pair for pair in good])
    table, _ = ds._commit()
    limit = 64 * 48                                                  # vouches for 3072 pixels: 56 x 56 and 64 x 64 exceed it
    too_big = [k for k, s in enumerate(SIZES) if s[0] * s[1] > limit]
    assert too_big == [2, 5, 8]
    got = host(covis_boxes_indexed(table, n, limit, idx1, idx2, params))
    check(got, good, [pair[0] in too_big or pair[1] in too_big for pair in good])


def test_runs_are_bit_identical_and_a_dirty_workspace_is_as_good(gpu):
    import imagematching_oetr_amd as pkg
    views, results = the_set()
    ds = depth_set(gpu, views)
    pairs = sorted(results)
    out = pkg.overlap_boxes_indexed(ds, pairs)
    first = {k: out[k].clone() for k in KEYS}
    ws = out['workspace']
    pkg.overlap_boxes_indexed(ds, pairs, out=out)
    assert_same(out, first)
    ws.fill_(0xA5)
    for k in KEYS:
        out[k].fill_(1)
    pkg.overlap_boxes_indexed(ds, pairs, out=out)
    assert out['workspace'] is ws
    assert_same(out, first)
    # other pairs on the same outputs and workspace: nothing of the first call is left
    pkg.overlap_boxes_indexed(ds, pairs[::-1], out=out)
    for k in KEYS:
        assert torch.equal(out[k], first[k].flip(0)), k


def test_captured_into_a_hip_graph_and_replayed_on_new_indices(gpu):
    """Enqueue-only, no host read: captured with default settings; a replay computes the pairs the index tensor
    holds at replay time."""
    import imagematching_oetr_amd as pkg
    views, results = the_set()
    ds = depth_set(gpu, views)
    pairs = sorted(results)
    first, second = pairs[:24], pairs[40:64]
    index = torch.tensor(first, dtype=torch.int32, device=gpu)
    eager = {k: v.clone() for k, v in pkg.overlap_boxes_indexed(ds, index).items()}     # also uploads the table
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.overlap_boxes_indexed(ds, index)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(captured, eager)
    index.copy_(torch.tensor(second, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    got = host(captured)
    for p, pair in enumerate(second):
        assert_pair(got, p, results[pair], pair)
    got = host(eager)
    for p, pair in enumerate(first):
        assert_pair(got, p, results[pair], pair)


@pytest.mark.parametrize('n', [3, 14])
def test_workspace_clear_replayed_three_times_with_copies_between(gpu, n):
    """The call's workspace clear under graph replay (64 bytes a pair: 192 and 896 bytes; ``clear_acc``, a kernel
    since a memset node of the stacked entry failed this pattern: ``tests/test_gpu_covis.py``).  Three replays with ``copy_`` of new indices between them: after each the boxes are the restatement of the pairs the
    index tensor held, and the bytes around the workspace are untouched.  The second list's pairs look at view
    ``AWAY_VIEW`` (no inlier) where the first list's have hundreds: nothing may be left in the accumulators."""
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd import hip_engine
    guard = 64
    views, results = the_set()
    ds = depth_set(gpu, views)
    pairs = sorted(results)
    seen = [p for p in pairs if results[p]['valid']]
    away = [p for p in pairs if cso.AWAY_VIEW in p]
    assert len(seen) >= 2 * n and len(away) >= n and not any(results[p]['valid'] for p in away)
    rounds = [seen[:n], away[:n], seen[n:2 * n]]
    index = torch.tensor(rounds[0], dtype=torch.int32, device=gpu)
    pkg.overlap_boxes_indexed(ds, index)                             # uploads the table, loads the code objects
    need = int(hip_engine.load_library().oetr_covis_set_workspace_bytes(n))
    assert need == 64 * n
    whole = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    ws = whole[guard:guard + need]
    out = {'overlap_box1': torch.zeros(n, 4, device=gpu), 'overlap_box2': torch.zeros(n, 4, device=gpu),
           'overlap_valid': torch.zeros(n, dtype=torch.bool, device=gpu),
           'overlap_count': torch.zeros(n, dtype=torch.int32, device=gpu), 'workspace': ws}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert pkg.overlap_boxes_indexed(ds, index, out=out) is out
    assert out['workspace'] is ws
    for r, listed in enumerate(rounds):
        if r:
            index.copy_(torch.tensor(listed, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        got = host(out)
        for p, pair in enumerate(listed):
            assert_pair(got, p, results[pair], (r, pair))
        assert bool((whole[:guard] == 0xA5).all()) and bool((whole[-guard:] == 0xA5).all()), r


def test_on_a_side_stream(gpu):
    import imagematching_oetr_amd as pkg
    views, results = the_set()
    ds = depth_set(gpu, views)
    torch.cuda.synchronize()                                         # the maps went up on the current stream
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        out = pkg.mine_pairs(ds, sorted(results))
    side.synchronize()
    got = host(out)
    for p, pair in enumerate(sorted(results)):
        assert_pair(got, p, results[pair], pair)
    assert int(out['n_kept']) > 0


# ------------------------------------------------------------------ oetr_covis_select
def _select_case():
    """600 pairs (three chunks of the scan, the last one ragged): the special boxes first, then seeded integer boxes."""
    special1 = [[0, 0, 40, 10], [0, 0, 41, 10], [5, 0, 5, 10], [5, 0, 5, 10], [5, 0, 5, 90], [0, 0, 0, 0], [0, 0, 90, 10],
                [0, 0, 90, 10], [3, 4, 9, 30]]
    special2 = [[0, 0, 20, 10], [0, 0, 20, 10], [0, 0, 20, 10], [3, 0, 3, 10], [3, 0, 3, 10], [0, 0, 0, 0], [0, 0, 20, 10],
                [0, 0, 0, 0], [0, 0, 20, 10]]
    valid = [True, True, True, True, True, False, False, True, True]
    rng = np.random.default_rng(21)
    n = 600 - len(valid)
    xy = rng.integers(0, 50, (2, n, 2))
    wh = rng.integers(0, 120, (2, n, 2))                             # zero widths among them
    boxes = np.concatenate([xy, xy + wh], axis=2)
    b1 = np.concatenate([np.array(special1), boxes[0]]).astype(np.int64)
    b2 = np.concatenate([np.array(special2), boxes[1]]).astype(np.int64)
    return b1, b2, np.concatenate([np.array(valid), rng.random(n) < 0.8])


def test_select_equals_the_restatement(gpu):
    from imagematching_oetr_amd.covis_set import select_pairs
    b1, b2, valid = _select_case()
    t1, t2 = torch.from_numpy(b1.astype(np.float32)).to(gpu), torch.from_numpy(b2.astype(np.float32)).to(gpu)
    tv = torch.from_numpy(valid).to(gpu)
    want_kept, want_n, want_sd = cso.select(b1, b2, valid, 2.0)
    assert cso.scale_diff(b1[0], b2[0]) == 2.0 and 0 not in want_kept and 1 in want_kept     # exactly 2 is not kept
    assert want_sd[2] == np.inf and np.isnan(want_sd[3]) and np.isnan(want_sd[4]) and 2 in want_kept
    assert 6 not in want_kept and 7 not in want_kept and 100 < want_n < 500
    for limit in (None, 0, -3, 1, want_n - 1, want_n, want_n + 1, 600, 5000):
        res = select_pairs(t1, t2, tv, 2.0, limit)
        kept, n_kept, sd = cso.select(b1, b2, valid, 2.0, limit)
        assert res['kept'].dtype == torch.int32 and res['n_kept'].dtype == torch.int32 and res['scale_diff'].dtype == torch.float64
        assert int(res['n_kept']) == n_kept == (want_n if limit is None or limit <= 0 else min(limit, want_n)), limit
        assert np.array_equal(res['kept'].cpu().numpy(), kept), limit
        assert np.array_equal(res['scale_diff'].cpu().numpy(), sd, equal_nan=True), limit
    for thr in (0.0, 1.0, 3.5, float('inf')):
        res = select_pairs(t1, t2, tv.to(torch.uint8), thr)
        kept, n_kept, _ = cso.select(b1, b2, valid, thr)
        assert int(res['n_kept']) == n_kept and np.array_equal(res['kept'].cpu().numpy(), kept), thr
    one = select_pairs(t1[:1], t2[:1], tv[:1])                                                # a list of one
    assert int(one['n_kept']) == 0 and one['kept'].tolist() == [-1] and one['scale_diff'].tolist() == [2.0]


def test_mine_pairs_equals_the_pinned_set(gpu):
    import imagematching_oetr_amd as pkg
    for e in json.loads((REPO / 'tests' / 'covis_set_expected.json').read_text())['sets']:
        views, results = the_set(tuple(tuple(s) for s in e['sizes']), e['seed'])
        ds = depth_set(gpu, views)
        out = pkg.mine_pairs(ds, [tuple(p) for p in e['pairs']], e['min_scale_diff'])
        got = host(out)
        assert got['overlap_box1'].astype(np.int64).tolist() == e['box1'] and got['overlap_box2'].astype(np.int64).tolist() == e['box2']
        assert got['overlap_valid'].tolist() == e['valid'] and got['overlap_count'].tolist() == e['count']
        assert [repr(float(x)) for x in out['scale_diff'].cpu().numpy()] == e['scale_diff']
        n_kept = int(out['n_kept'])
        assert out['kept'][:n_kept].tolist() == e['kept'] and (out['kept'][n_kept:] == -1).all()
        cut = pkg.mine_pairs(ds, torch.tensor(e['pairs'], dtype=torch.int32, device=gpu), e['min_scale_diff'], limit=2)
        assert int(cut['n_kept']) == 2 and cut['kept'][:3].tolist() == e['kept'][:2] + [-1]


# ------------------------------------------------------------------ evaluate_indexed
def _iou_numpy(a, b):
    a, b = a.astype(np.float32), b.astype(np.float32)
    wh = np.clip(np.minimum(a[:, 2:], b[:, 2:]) - np.maximum(a[:, :2], b[:, :2]), 0, None)
    ov = wh[:, 0] * wh[:, 1]
    union = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - ov
    return ov / np.maximum(union, np.float32(1e-6))


def test_evaluate_indexed_on_a_mixed_size_set(gpu):
    """Images and depth maps of two sizes, boxes through the feature bank, ground truth by index: the recalls are
    those recomputed with numpy from ``forward_pairs_indexed``'s boxes and the restatement's ground truth."""
    import imagematching_oetr_amd as pkg
    sizes = ((160, 224), (224, 160), (160, 224), (224, 160))
    views, results = the_set(sizes, 3)
    torch.manual_seed(0)
    model = pkg.OETR(pkg.get_cfg_defaults().OETR).eval().to(gpu)
    g = torch.Generator().manual_seed(5)
    images = [torch.rand(h, w, 3, generator=g) for h, w in sizes]
    ds = depth_set(gpu, views)
    pairs = [(0, 1), (1, 0), (0, 2), (3, 1), (2, 3), (1, 2), (3, 0)]
    p1, p2 = pkg.forward_pairs_indexed(model, images, pairs, max_batch=4)          # also the warm-up
    gt1 = np.stack([results[p]['box1'] for p in pairs])
    gt2 = np.stack([results[p]['box2'] for p in pairs])
    ious = np.concatenate([_iou_numpy(gt1, p1.cpu().numpy()), _iou_numpy(gt2, p2.cpu().numpy())])
    flushes = []
    flush = model.hip_flush
    model.hip_flush = lambda: (flushes.append(1), flush())[1]
    low = np.array([0.01, 0.02, 0.05, 0.1, 0.2, 0.5])              # a random-weight model's boxes are poor: thresholds that tell
    for thrs in (np.arange(0.5, 0.96, 0.05), low):
        del flushes[:]
        res = pkg.evaluate_indexed(model, images, ds, pairs, iou_thrs=thrs, max_batch=4)
        assert len(flushes) == 1
        want = np.array([(ious >= t).sum() / float(ious.shape[0]) for t in thrs])
        print('recalls', thrs, res['recalls'], 'mean_iou', res['mean_iou'])
        assert np.array_equal(res['recalls'], want), (res['recalls'], want)
        assert res['n'] == 2 * len(pairs) and res['n_valid_pairs'] == sum(results[p]['valid'] for p in pairs) > 0
        # (the mean is compared loosely: two runs of the trunk's library convolutions need not agree to the bit)
        assert res['mean_iou'] == pytest.approx(float(np.mean(ious.astype(np.float64))), rel=1e-5)
    assert res['mean_iou'] > 0
