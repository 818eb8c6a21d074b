"""GPU checks of ``select_keypoints`` (``include/oetr_keypoint_select.h``, ``csrc/keypoint_select.hip``): every output
of the device call - keypoints, scores, descriptors, offsets, counts, over the whole capacity - equals the numpy
specification ``tests/keypoint_select_oracle.py``; floats are compared by their bits, no tolerance.

The kernels have no two-dimensional tile: the edges at which they take another path are pixel counts - a wave (64), an
NMS block (2048 pixels) and a compaction chunk (4096 pixels) - so the map sizes sit one below, at and one above those,
beside the degenerate ones."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import keypoint_select_oracle as kso  # noqa: E402
import match_assembly_oracle as mao  # noqa: E402
import nn_match_oracle as nmo  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ('keypoints', 'scores', 'descriptors', 'offsets', 'counts')
F32 = np.float32

# (H, W), (h, w): 1x1, 1xW, Hx1, 7x9 (63 pixels), one side below every r > 0, 64 and 65 pixels, 2047 / 2048 / 2049 and
# 4095 / 4096 / 4097 pixels, h or w of 1, score maps larger than h * 8 x w * 8 (taps fall outside the descriptor map)
SIZES = (((1, 1), (1, 1)), ((1, 37), (1, 5)), ((29, 1), (4, 1)), ((7, 9), (1, 2)), ((3, 40), (1, 5)), ((8, 8), (1, 1)),
         ((5, 13), (2, 1)), ((23, 89), (3, 12)), ((32, 64), (4, 8)), ((3, 683), (1, 80)), ((63, 65), (8, 9)),
         ((64, 64), (8, 8)), ((17, 241), (2, 20)), ((40, 56), (3, 4)))


def grid_scores(rng, H, W, levels=8):
    """Scores on a coarse grid of values: ties and plateaus everywhere."""
    return (rng.integers(0, levels + 1, (H, W)) / levels).astype(F32)


def distinct_scores(rng, H, W):
    return ((rng.permutation(H * W) + 1) / (H * W)).astype(F32).reshape(H, W)


def mixed_maps(seed, D=8):
    rng = np.random.default_rng(seed)
    scores = [grid_scores(rng, H, W) if i % 2 else distinct_scores(rng, H, W) for i, ((H, W), _) in enumerate(SIZES)]
    descriptors = [rng.standard_normal((D, h, w)).astype(F32) for _, (h, w) in SIZES]
    return scores, descriptors


def device(maps, gpu):
    return [torch.from_numpy(np.ascontiguousarray(m)).to(gpu) for m in maps]


def host(res):
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in OUTPUTS}


def assert_equal(got, want, tag=None):
    for k in OUTPUTS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            rows = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(1))[0]
            raise AssertionError((tag, k, len(rows), rows[:8].tolist(), g[rows[:8]].tolist(), w[rows[:8]].tolist()))


def run(pkg, gpu, scores, descriptors, **params):
    return host(pkg.select_keypoints(pkg.keypoint_map_table(device(scores, gpu), device(descriptors, gpu)), **params))


@pytest.fixture(scope='module')
def mixed():
    """The mixed-size maps: made once, shared, never modified."""
    return mixed_maps(21)


@pytest.mark.parametrize('r', (0, 1, 4, 8))
def test_mixed_sizes_in_one_call_at_every_radius(gpu, mixed, r):
    import imagematching_oetr_amd as pkg
    scores, descriptors = mixed
    params = dict(nms_radius=r, threshold=0.005, remove_borders=0, max_keypoints=48, cell=8)
    want = kso.select_call(scores, descriptors, **params)
    assert_equal(run(pkg, gpu, scores, descriptors, **params), want, r)
    # both selection branches ran
    kept, cand = want['counts'][:, 1], want['counts'][:, 0]
    assert (cand > 48).any() and ((cand <= 48) & (cand > 0)).any() and kept.max() == 48


@pytest.mark.parametrize('border', (0, 4, 20))
def test_borders(gpu, mixed, border):
    import imagematching_oetr_amd as pkg
    scores, descriptors = mixed
    params = dict(nms_radius=2, threshold=0.25, remove_borders=border, max_keypoints=30, cell=8)
    want = kso.select_call(scores, descriptors, **params)
    assert_equal(run(pkg, gpu, scores, descriptors, **params), want, border)
    tall = [b for b, ((H, W), _) in enumerate(SIZES) if 2 * border >= min(H, W)]
    assert border == 0 or (tall and (want['counts'][tall] == 0).all())     # 2 * border >= H: no keypoints
    assert want['counts'][:, 1].sum() > 0


def test_special_scores(gpu):
    import imagematching_oetr_amd as pkg
    rng = np.random.default_rng(8)
    at_threshold = grid_scores(rng, 20, 30, 4)                       # values k / 4: 0.25 is met exactly, and is not kept
    zeros = np.zeros((12, 70), F32)
    wild = grid_scores(rng, 33, 35)
    wild[rng.integers(0, 33, 40), rng.integers(0, 35, 40)] = np.nan
    wild[rng.integers(0, 33, 12), rng.integers(0, 35, 12)] = np.inf
    wild[rng.integers(0, 33, 25), rng.integers(0, 35, 25)] = -np.inf
    all_nan = np.full((6, 6), np.nan, F32)
    negative = -grid_scores(rng, 9, 9) - F32(0.5)
    scores = [at_threshold, zeros, wild, all_nan, negative]
    descriptors = [rng.standard_normal((12, 3, 5)).astype(F32) for _ in scores]
    for r, k in ((0, 4096), (2, 4096), (2, 20)):
        params = dict(nms_radius=r, threshold=0.25, remove_borders=0, max_keypoints=k, cell=8)
        want = kso.select_call(scores, descriptors, **params)
        assert_equal(run(pkg, gpu, scores, descriptors, **params), want, (r, k))
        assert want['counts'][1].tolist() == [0, 0] and want['counts'][3].tolist() == [0, 0] and want['counts'][4].tolist() == [0, 0]
        n0 = want['offsets'][1]
        assert n0 > 0 and (want['scores'][:n0] > 0.25).all() and (at_threshold == 0.25).sum() > 20
        assert np.isinf(want['scores'][want['offsets'][2]:want['offsets'][3]]).any()


@pytest.mark.parametrize('k', (1, 100, 4096))
def test_the_cut_at_k_minus_one_k_and_k_plus_one_candidates(gpu, k):
    import imagematching_oetr_amd as pkg
    rng = np.random.default_rng(k)
    H, W = 80, 90                                                    # 7200 pixels: more than 4096 candidates at r = 0
    scores = []
    for n in (k - 1, k, k + 1):
        S = np.zeros(H * W, F32)
        S[rng.choice(H * W, n, replace=False)] = (rng.integers(5, 9, n) / 8).astype(F32)   # four values: ties at the cut
        scores.append(S.reshape(H, W))
    scores.append((rng.integers(4, 9, (H, W)) / 8).astype(F32))      # 4/5 of 7200 pixels are candidates: ties across the cut
    descriptors = [rng.standard_normal((4, 10, 12)).astype(F32) for _ in scores]
    params = dict(nms_radius=0, threshold=0.5, remove_borders=0, max_keypoints=k, cell=8)
    want = kso.select_call(scores, descriptors, **params)
    assert want['counts'][:3].tolist() == [[k - 1, k - 1], [k, k], [k + 1, k]] and want['counts'][3, 0] > max(k, 1000)
    assert want['counts'][3, 1] == k
    assert_equal(run(pkg, gpu, scores, descriptors, **params), want, k)


@pytest.mark.parametrize('D', (4, 68, 256, 512))
def test_descriptor_widths_and_layouts(gpu, D):
    import imagematching_oetr_amd as pkg
    rng = np.random.default_rng(D)
    shapes = (((40, 56), (5, 7)), ((50, 70), (5, 7)), ((24, 31), (1, 4)))      # the second: taps outside the map
    scores = [distinct_scores(rng, H, W) for (H, W), _ in shapes]
    descriptors = [rng.standard_normal((D, h, w)).astype(F32) for _, (h, w) in shapes]
    params = dict(nms_radius=2, threshold=0.3, remove_borders=0, max_keypoints=40, cell=8)
    want = kso.select_call(scores, descriptors, **params)
    nchw = device(descriptors, gpu)
    last = [d.permute(1, 2, 0).contiguous().permute(2, 0, 1) for d in nchw]     # channels-last storage, [D,h,w] view
    assert all(d.stride(0) == 1 for d in last) and all(d.is_contiguous() for d in nchw)
    s = device(scores, gpu)
    assert_equal(host(pkg.select_keypoints(pkg.keypoint_map_table(s, nchw), **params)), want, ('NCHW', D))
    table = pkg.keypoint_map_table(s, last)
    assert [m.data_ptr() for m in table.maps[1::2]] == [d.data_ptr() for d in last]      # no copy
    assert_equal(host(pkg.select_keypoints(table, **params)), want, ('channels-last', D))
    # one batched tensor in torch's channels_last memory format goes in the same way
    same = [rng.standard_normal((D, 5, 7)).astype(F32) for _ in range(2)]
    batch = torch.from_numpy(np.stack(same)).to(gpu).contiguous(memory_format=torch.channels_last)
    want = kso.select_call(scores[:2], same, **params)
    assert_equal(host(pkg.select_keypoints(pkg.keypoint_map_table(s[:2], batch), **params)), want, ('batched', D))


def test_more_maps_than_one_grid_dimension(gpu):
    import imagematching_oetr_amd as pkg
    rng = np.random.default_rng(3)
    n, kinds, k = 65538, 7, 2
    S = np.stack([grid_scores(rng, 3, 3, 4) for _ in range(kinds)])
    S[0], S[1, 1, 1] = 0, np.nan
    F = rng.standard_normal((kinds, 4, 1, 1)).astype(F32)
    which = np.arange(n) % kinds
    params = dict(nms_radius=1, threshold=0.2, remove_borders=0, max_keypoints=k, cell=8)
    images = [kso.select_image(S[i], F[i], **params) for i in range(kinds)]
    want = kso.join([images[i] for i in which], k, 4)
    assert 0 < want['offsets'][-1] < n * k
    res = pkg.select_keypoints(pkg.keypoint_map_table(torch.from_numpy(S[which]).to(gpu), torch.from_numpy(F[which]).to(gpu)),
                               **params)
    assert_equal(host(res), want, '65538 maps')


def test_every_call_writes_its_whole_capacity_and_nothing_else(gpu, mixed):
    import imagematching_oetr_amd as pkg
    scores, descriptors = mixed
    table = pkg.keypoint_map_table(device(scores, gpu), device(descriptors, gpu))
    n, k, D, guard = len(scores), 48, 8, 64
    rows = n * k
    need = pkg.load_library().oetr_keypoint_select_workspace_bytes(table.total_pixels, n, k)
    params = dict(nms_radius=4, threshold=0.005, remove_borders=0, max_keypoints=k, cell=8)
    want = kso.select_call(scores, descriptors, **params)
    assert want['offsets'][-1] < rows                                # there is a tail to write
    shapes = dict(keypoints=(rows, 2), scores=(rows,), descriptors=(rows, D), offsets=(n + 1,), counts=(n, 2))
    dtypes = dict(offsets=torch.int32, counts=torch.int32)
    for sentinel in (77, -3):
        whole, out = {}, {}
        for key, shape in shapes.items():
            whole[key] = torch.full((shape[0] + 2 * guard,) + shape[1:], sentinel, dtype=dtypes.get(key, torch.float32), device=gpu)
            out[key] = whole[key][guard:guard + shape[0]]
        whole['workspace'] = torch.full((need + 512,), 0x5a, dtype=torch.uint8, device=gpu)
        out['workspace'] = whole['workspace'][256:256 + need]
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        assert pkg.select_keypoints(table, out=out, **params) is out
        assert torch.cuda.memory_allocated() == before                # nothing allocated with out=
        assert_equal(host(out), want, sentinel)                       # every row of the capacity, the tail included
        for key, shape in shapes.items():
            assert (whole[key][:guard] == sentinel).all() and (whole[key][guard + shape[0]:] == sentinel).all(), key
        assert (whole['workspace'][:256] == 0x5a).all() and (whole['workspace'][256 + need:] == 0x5a).all()
    total = want['offsets'][-1]
    assert (want['keypoints'][total:] == -1).all() and np.isnan(want['scores'][total:]).all()
    with pytest.raises(ValueError, match='other sizes'):
        pkg.select_keypoints(table, out=out, **dict(params, max_keypoints=47))


def test_two_calls_give_equal_bits_and_a_graph_replays_on_changed_inputs(gpu, mixed):
    import imagematching_oetr_amd as pkg
    scores, descriptors = mixed
    s, d = device(scores, gpu), device(descriptors, gpu)
    table = pkg.keypoint_map_table(s, d)
    params = dict(nms_radius=4, threshold=0.005, remove_borders=1, max_keypoints=48, cell=8)
    first, again = host(pkg.select_keypoints(table, **params)), host(pkg.select_keypoints(table, **params))
    assert_equal(again, first, 'two eager calls')
    assert_equal(first, kso.select_call(scores, descriptors, **params), 'specification')
    out = pkg.select_keypoints(table, **params)                      # allocates the outputs and the workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.select_keypoints(table, out=out, **params)
        with pytest.raises(ValueError, match='inside a graph capture'):          # host maps: refused, nothing enqueued
            pkg.keypoint_map_table([torch.from_numpy(scores[0])], [torch.from_numpy(descriptors[0])])
    graph.replay()
    assert_equal(host(captured), first, 'replay')
    other_scores, other_descriptors = mixed_maps(22)
    for t, a in zip(s + d, other_scores + other_descriptors):
        t.copy_(torch.from_numpy(a))
    want = kso.select_call(other_scores, other_descriptors, **params)
    for replay in range(2):
        graph.replay()
        assert_equal(host(captured), want, ('replay on other maps', replay))
    assert not np.array_equal(want['counts'], first['counts'])


def test_the_result_feeds_the_matcher_and_the_assembly_as_it_is(gpu):
    import imagematching_oetr_amd as pkg
    rng = np.random.default_rng(31)
    P, k, D = 3, 24, 16
    sides = []
    for side in range(2):
        scores = [distinct_scores(rng, 30 + 3 * p, 41 - 2 * p) for p in range(P)]
        scores[1] = grid_scores(rng, 9, 9) * F32(side)               # side 0 of pair 1 has no keypoints at all
        descriptors = [rng.standard_normal((D, 5, 6)).astype(F32) for _ in range(P)]
        params = dict(nms_radius=3, threshold=0.3, remove_borders=2, max_keypoints=k, cell=8)
        res = pkg.select_keypoints(pkg.keypoint_map_table(device(scores, gpu), device(descriptors, gpu)), **params)
        spec = kso.select_call(scores, descriptors, **params)
        assert_equal(host(res), spec, ('side', side))
        sides.append((res, spec))
    (res0, spec0), (res1, spec1) = sides
    assert spec0['counts'][1, 1] == 0 and spec0['counts'][0, 1] == k and 0 < spec1['counts'][1, 1] < k
    matched = pkg.match_descriptors(res0['descriptors'], res1['descriptors'], offsets0=res0['offsets'],
                                    offsets1=res1['offsets'], max_k0=k, max_k1=k)
    off0, off1 = spec0['offsets'], spec1['offsets']
    sims = [nmo.similarity(spec0['descriptors'][off0[p]:off0[p + 1]], spec1['descriptors'][off1[p]:off1[p + 1]]) for p in range(P)]
    want = nmo.match_call(sims, P * k, P * k, off0, off1, max_k0=k, max_k1=k)
    for key in ('matches0', 'matching_scores0', 'matches1', 'counts'):
        assert matched[key].cpu().numpy().tobytes() == want[key].tobytes(), key
    assert (want['matches0'] > -1).sum() > 10
    geometry = mao.make_call(5, tuple((int(off0[p + 1] - off0[p]), int(off1[p + 1] - off1[p]), 'none', 1) for p in range(P)))
    records = torch.from_numpy(np.ascontiguousarray(geometry['info']).view(np.uint8).reshape(P, -1).copy()).to(gpu)
    lists = pkg.assemble_matches(records, torch.from_numpy(geometry['scales']).to(gpu), res0['keypoints'], res1['keypoints'],
                                 matched['matches0'], matched['matching_scores0'], offsets0=res0['offsets'],
                                 offsets1=res1['offsets'])
    asm = mao.assemble(geometry['info'], geometry['scales'], spec0['keypoints'], spec1['keypoints'], off0, off1,
                       want['matches0'], want['matching_scores0'])
    assert asm['offsets'][-1] == (want['matches0'] > -1).sum()
    for key, w in asm.items():
        assert mao.equal_bits(lists[key].cpu().numpy(), w), key


def test_the_plug_in_returns_the_references_shapes(gpu):
    from imagematching_oetr_amd.dloc_extractor import DenseExtractor

    class Net(torch.nn.Module):
        """Two layers: a score head at full resolution and a descriptor head at one eighth."""

        def __init__(self):
            super().__init__()
            self.score = torch.nn.Conv2d(1, 1, 3, padding=1)
            self.desc = torch.nn.Conv2d(1, 32, 8, stride=8)

        def forward(self, image):
            return torch.sigmoid(self.score(image))[:, 0], self.desc(image)

    torch.manual_seed(4)
    net = Net().to(gpu).eval()
    image = torch.rand(3, 1, 48, 64, device=gpu)
    with torch.no_grad():
        out = DenseExtractor({'max_keypoints': 50, 'nms_radius': 3}, net=net)({'image': image})
        scores, descriptors = net(image)
    assert set(out) == {'keypoints', 'scores', 'descriptors'} and all(len(out[key]) == 3 for key in out)
    want = kso.select_call(list(scores.cpu().numpy()), list(descriptors.cpu().numpy()), nms_radius=3, threshold=0.005,
                           remove_borders=4, max_keypoints=50, cell=8)
    for b in range(3):
        lo, hi = want['offsets'][b], want['offsets'][b + 1]
        K = hi - lo
        assert 0 < K <= 50
        assert tuple(out['keypoints'][b].shape) == (K, 2) and tuple(out['scores'][b].shape) == (K,)
        assert tuple(out['descriptors'][b].shape) == (32, K) and out['descriptors'][b].dtype == torch.float32
        assert out['keypoints'][b].cpu().numpy().tobytes() == want['keypoints'][lo:hi].tobytes()
        assert out['scores'][b].cpu().numpy().tobytes() == want['scores'][lo:hi].tobytes()
        assert out['descriptors'][b].t().contiguous().cpu().numpy().tobytes() == want['descriptors'][lo:hi].tobytes()
