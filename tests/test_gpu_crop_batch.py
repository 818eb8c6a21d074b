"""GPU tests of the batched crop call (``oetr_overlap_crop_batch``, ``crop_batch.py``): pair k of a call
must be what the per-pair ``overlap_crop`` gives for that pair alone - every field of the geometry record
and every pixel, bit for bit - at the smallest shapes at which the kernels can go wrong (1-channel images
of 40-200 px, sizes off the 64 x 16 tile, mixed sizes inside one call)."""
import random

import numpy as np
import pytest
import torch

import imagematching_oetr_amd as pkg
from oracle import crop_oracle as cro
from tests.test_crop_cpu import load_cases

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
PIX_TOL = 2e-6      # as tests/test_gpu_pipeline.py: crops live in [0,1]; same algorithm, fp32, another contraction


def info_fields(g):
    """Every field of one ``oetr_crop_info`` as plain Python values."""
    two = lambda a: [int(a[0]), int(a[1])]
    return dict(valid=int(g.valid), box=[[int(v) for v in g.box[i]] for i in (0, 1)],
                crop_w=two(g.crop_w), crop_h=two(g.crop_h), new_w=two(g.new_w), new_h=two(g.new_h),
                out_w=two(g.out_w), out_h=two(g.out_h),
                ratio=[[float(v) for v in g.ratio[i]] for i in (0, 1)],
                sbox=[[float(v) for v in g.sbox[i]] for i in (0, 1)])


def image(hw, channels=1):
    """The fuzz test's image of a size (same seed recipe), any channel count."""
    return torch.rand(1, channels, *hw, generator=torch.Generator().manual_seed(hw[0] * 1000 + hw[1]))


def fuzz_cases():
    """The 60 cases of ``test_crop_geometry_fuzz_is_bit_exact_vs_oracle`` (tests/test_gpu_pipeline.py),
    restated: the same generator, seed and order of draws."""
    rng = random.Random(11)
    cases = []
    for _ in range(60):
        hw0 = (rng.randrange(40, 200), rng.randrange(40, 200))
        hw1 = (rng.randrange(40, 200), rng.randrange(40, 200))
        sc0 = (rng.choice([1.0, 0.75, 0.3, 1.6]), rng.choice([1.0, 0.6, 0.25, 1.3]))
        sc1 = (rng.choice([1.0, 0.75, 0.3, 1.6]), rng.choice([1.0, 0.6, 0.25, 1.3]))

        def box(hw, sc):
            w, h = hw[1] / sc[0], hw[0] / sc[1]          # OETR-frame size that maps onto the image
            x1, y1 = rng.uniform(0, w * 0.7), rng.uniform(0, h * 0.7)
            return torch.tensor([x1, y1, x1 + rng.uniform(0.5, w * 0.6), y1 + rng.uniform(0.5, h * 0.6)])
        b0, b1 = box(hw0, sc0), box(hw1, sc1)
        keep, div, pp = rng.random() < 0.7, rng.choice([1, 1, 8]), rng.random() < 0.3
        cases.append(dict(hw0=hw0, hw1=hw1, sc0=sc0, sc1=sc1, b0=b0, b1=b1, mode=(keep, div, pp)))
    return cases


def check_call(gpu, pairs, mode, expect_valid=None):
    """One batched call over ``pairs`` (dicts with device images ``im0`` / ``im1``, boxes ``b0`` / ``b1`` [4]
    and scales ``sc0`` / ``sc1``) against the per-pair call of every pair.  Returns the batch."""
    keep, div, pp = mode
    table = pkg.crop_pair_table([p['im0'] for p in pairs], [p['im1'] for p in pairs],
                                [p['sc0'] for p in pairs], [p['sc1'] for p in pairs])
    box0 = torch.stack([p['b0'] for p in pairs]).to(gpu)
    box1 = torch.stack([p['b1'] for p in pairs]).to(gpu)
    batch = pkg.overlap_crop_batch(table, box0, box1, keep_aspect=keep, size_divisor=div, pragueparks=pp)
    assert len(batch) == len(pairs) and len(batch.geometry()) == len(pairs)
    for k, p in enumerate(pairs):
        one = pkg.overlap_crop(p['im0'], p['im1'], p['b0'].to(gpu), p['b1'].to(gpu), p['sc0'], p['sc1'], keep, div, pp)
        want, got = info_fields(one.geometry()), info_fields(batch.geometry()[k])
        assert got == want, (k, got, want)
        assert batch.valid[k] == want['valid']
        if expect_valid is not None:
            assert want['valid'] == expect_valid[k], (k, want['valid'])
        if want['valid'] < 0:
            with pytest.raises(pkg.OetrError):
                batch.crop(k, 0)
            continue
        for i in (0, 1):
            assert tuple(batch.crop(k, i).shape) == tuple(one.crop(i).shape), (k, i)
            assert torch.equal(batch.crop(k, i), one.crop(i)), (k, i)
            assert torch.equal(batch.bbox(k, i), one.bbox(i)) and batch.ratio(k, i) == one.ratio(i)
    return batch


def test_fuzz_calls_equal_the_per_pair_path_bit_for_bit(gpu):
    groups = {}
    for c in fuzz_cases():
        groups.setdefault(c['mode'], []).append(c)
    cache, sizes, total = {}, [], 0

    def dev_image(hw):
        if hw not in cache:
            cache[hw] = image(hw).to(gpu)
        return cache[hw]
    order = (8, 5, 1)
    for mode, cases in groups.items():
        at, turn = 0, 0
        while at < len(cases):
            chunk = cases[at:at + order[turn % 3]]
            pairs = [dict(im0=dev_image(c['hw0']), im1=dev_image(c['hw1']), b0=c['b0'], b1=c['b1'],
                          sc0=c['sc0'], sc1=c['sc1']) for c in chunk]
            check_call(gpu, pairs, mode)
            sizes.append(len(chunk))
            total += len(chunk)
            at, turn = at + len(chunk), turn + 1
    assert total == 60 and {1, 5, 8} <= set(sizes), sizes
    assert {m[1] for m in groups} == {1, 8}       # both launch counts ran


def test_three_channels_and_one_image_in_four_pairs(gpu):
    cases = fuzz_cases()
    # colour: the first three fuzz cases' boxes and sizes, 3-channel images, both divisors
    for div in (1, 8):
        pairs = [dict(im0=image(c['hw0'], 3).to(gpu), im1=image(c['hw1'], 3).to(gpu), b0=c['b0'], b1=c['b1'],
                      sc0=c['sc0'], sc1=c['sc1']) for c in cases[:3]]
        batch = check_call(gpu, pairs, (True, div, False))
        assert batch.crop(0, 0).shape[1] == 3
    # one image tensor as side 0 of four pairs (and once as side 1), four different boxes
    a = image((120, 150)).to(gpu)
    others = [image(hw).to(gpu) for hw in ((90, 70), (150, 181), (64, 64))]
    boxes = [torch.tensor(b) for b in ([10.0, 12.0, 100.0, 80.0], [0.0, 0.0, 149.0, 119.0],
                                        [70.5, 30.25, 140.0, 60.0], [33.0, 64.0, 97.0, 118.0])]
    pairs = [dict(im0=a, im1=([a] + others)[k], b0=boxes[k], b1=torch.tensor([5.0, 6.0, 60.0, 58.0]),
                  sc0=(1.0, 1.0), sc1=(1.0, 1.0)) for k in range(4)]
    batch = check_call(gpu, pairs, (True, 8, False), expect_valid=[1, 1, 1, 1])
    assert batch.crop(0, 0).data_ptr() != batch.crop(1, 0).data_ptr()


def test_mixed_outcomes_in_one_call(gpu):
    """A cropping pair, a gate failure and a degenerate box (the ``outside`` box of
    ``test_degenerate_crop_is_reported_not_passed_through``) side by side."""
    im = torch.rand(1, 1, 64, 64, generator=torch.Generator().manual_seed(1)).to(gpu)
    other = image((50, 77)).to(gpu)
    inside = torch.tensor([5.0, 5.0, 60.0, 60.0])
    outside = torch.tensor([70.0, 10.0, 100.0, 50.0])         # x1 beyond the 64-px width
    thin = torch.tensor([10.0, 10.0, 11.9, 50.0])             # 1 px wide: the gate fails
    one = (1.0, 1.0)
    pairs = [dict(im0=im, im1=other, b0=inside, b1=torch.tensor([3.0, 4.0, 70.0, 45.0]), sc0=one, sc1=one),
             dict(im0=im, im1=other, b0=thin, b1=inside, sc0=one, sc1=one),
             dict(im0=im, im1=im, b0=outside, b1=inside, sc0=one, sc1=one)]
    for div in (1, 8):
        batch = check_call(gpu, pairs, (True, div, False), expect_valid=[1, 0, -1])
        assert batch.valid == [1, 0, -1]
        assert torch.equal(batch.crop(1, 0), im) and torch.equal(batch.crop(1, 1), other)     # pass-through, bit for bit
        with pytest.raises(pkg.OetrError):
            batch.crop(2, 0)
        with pytest.raises(pkg.OetrError):
            batch.crop(2, 1)
        assert batch.bbox(1, 0).tolist() == [[0.0, 0.0, 64.0, 64.0]] and batch.ratio(1, 1) == [[1.0, 1.0]]


def test_edges(gpu):
    one = (1.0, 1.0)
    full = lambda hw: torch.tensor([0.0, 0.0, float(hw[1]), float(hw[0])])
    # a 2 x 2-px crop: every tap of every output pixel is clamped to the border
    im0, im1 = image((48, 56)).to(gpu), image((41, 47)).to(gpu)
    tiny = torch.tensor([10.0, 10.0, 12.0, 12.0])
    for mode in ((True, 1, False), (False, 8, False)):
        b = check_call(gpu, [dict(im0=im0, im1=im1, b0=tiny, b1=tiny, sc0=one, sc1=one)], mode, expect_valid=[1])
        assert list(b.geometry()[0].crop_w) == [2, 2] and list(b.geometry()[0].crop_h) == [2, 2]
    # output widths of 63, 64 and 65: one short of, exactly and one past a 64-wide tile (without the aspect
    # rule the output takes the size of the larger image), in ONE call; then rounded up to 64 / 64 / 72
    pairs = []
    for w, h in ((63, 40), (64, 17), (65, 33)):
        big, small = image((h, w)).to(gpu), image((h - 3, w - 5)).to(gpu)
        pairs.append(dict(im0=big, im1=small, b0=torch.tensor([2.0, 3.0, w - 4.0, h - 2.0]),
                          b1=torch.tensor([1.0, 1.0, w - 20.0, h - 6.0]), sc0=one, sc1=one))
    b = check_call(gpu, pairs, (False, 1, False), expect_valid=[1, 1, 1])
    assert [int(g.out_w[0]) for g in b.geometry()] == [63, 64, 65] == [int(g.out_w[1]) for g in b.geometry()]
    assert [int(g.out_h[0]) for g in b.geometry()] == [40, 17, 33]
    b = check_call(gpu, pairs, (False, 8, False), expect_valid=[1, 1, 1])
    assert [int(g.out_w[0]) for g in b.geometry()] == [64, 64, 72]
    # an output one pixel high: a 190 x 2 strip of the smaller image under the aspect rule
    wide, strip_src = image((40, 120)).to(gpu), image((20, 200)).to(gpu)
    b = check_call(gpu, [dict(im0=wide, im1=strip_src, b0=torch.tensor([4.0, 4.0, 100.0, 36.0]),
                              b1=torch.tensor([5.0, 9.0, 195.0, 11.0]), sc0=one, sc1=one)],
                   (True, 1, False), expect_valid=[1])
    assert int(b.geometry()[0].out_h[1]) == 1 and int(b.geometry()[0].out_w[1]) == 120
    # the last pair of a call has larger images than the first: its tiles lie beyond the first pair's sizes
    small0, small1 = image((48, 56)).to(gpu), image((41, 47)).to(gpu)
    big0, big1 = image((150, 190)).to(gpu), image((199, 131)).to(gpu)
    pairs = [dict(im0=small0, im1=small1, b0=full((40, 50)), b1=full((30, 40)), sc0=one, sc1=one),
             dict(im0=big0, im1=big1, b0=full((150, 190)), b1=torch.tensor([3.0, 7.0, 120.0, 190.0]), sc0=one, sc1=one)]
    for div in (1, 8):
        check_call(gpu, pairs, (True, div, False), expect_valid=[1, 1])


def test_goldens(gpu, golden_dir):
    """The eight cases of tests/golden/crop.npz, grouped into calls by mode and channels: geometry equal
    to the golden, pixels within PIX_TOL of the oracle (and of the golden's stored crops)."""
    groups = {}
    for ci, c, im0, im1 in load_cases(golden_dir):
        key = (bool(c['keep_aspect']), int(c['size_divisor']), bool(c['pragueparks']), int(c['channels']))
        groups.setdefault(key, []).append((ci, c, im0, im1))
    assert sum(len(v) for v in groups.values()) == 8
    for (keep, div, pp, _), members in groups.items():
        table = pkg.crop_pair_table([m[2].to(gpu) for m in members], [m[3].to(gpu) for m in members],
                                    [tuple(m[1]['scales0']) for m in members], [tuple(m[1]['scales1']) for m in members])
        box0 = torch.stack([torch.from_numpy(m[1]['box0']).reshape(-1, 4)[0] for m in members]).float().to(gpu)
        box1 = torch.stack([torch.from_numpy(m[1]['box1']).reshape(-1, 4)[0] for m in members]).float().to(gpu)
        batch = pkg.overlap_crop_batch(table, box0, box1, keep, div, pp)
        for k, (ci, c, im0, im1) in enumerate(members):
            assert batch.valid[k] == int(bool(c['valid'])), ci
            ref = cro.overlap_crop(im0, im1, torch.from_numpy(c['box0']), torch.from_numpy(c['box1']),
                                   tuple(c['scales0']), tuple(c['scales1']), keep, div, pp)
            for i, s in ((0, '0'), (1, '1')):
                assert np.array_equal(batch.bbox(k, i).numpy().reshape(-1), c['bbox' + s]), (ci, i)
                assert np.array_equal(np.float32(batch.ratio(k, i)).astype(np.float64).reshape(-1), c['ratio' + s]), (ci, i)
                crop = batch.crop(k, i).cpu()
                assert tuple(crop.shape) == tuple(c['out_shape' + s]), (ci, i)
                assert float((crop - ref['crop' + s]).abs().max()) <= PIX_TOL, (ci, i)
                if 'crop' + s in c:
                    assert float((crop - torch.from_numpy(c['crop' + s])).abs().max()) <= PIX_TOL, (ci, i)
            if not batch.valid[k]:
                assert torch.equal(batch.crop(k, 0).cpu(), im0) and torch.equal(batch.crop(k, 1).cpu(), im1), ci


def test_capture_and_reuse_of_a_result(gpu):
    """The call is enqueue-only: captured into a graph and replayed after the boxes were overwritten it
    equals a fresh call; and written into an earlier result it allocates nothing."""
    ims0 = [image(hw, 3).to(gpu) for hw in ((96, 128), (80, 112), (57, 93), (96, 128))]
    ims1 = [image(hw, 3).to(gpu) for hw in ((80, 112), (96, 128), (120, 64), (61, 77))]
    table = pkg.crop_pair_table(ims0, ims1, [(1.0, 1.0)] * 4, [(1.0, 0.75)] * 4)
    b0 = torch.tensor([[10.0, 12.0, 100.0, 80.0], [5.0, 6.0, 90.0, 70.0], [0.0, 0.0, 93.0, 57.0], [30.0, 30.0, 60.0, 90.0]], device=gpu)
    b1 = torch.tensor([[5.0, 6.0, 90.0, 70.0], [10.0, 12.0, 100.0, 80.0], [8.0, 40.0, 50.0, 150.0], [2.0, 3.0, 70.0, 70.0]], device=gpu)
    held = pkg.overlap_crop_batch(table, b0, b1, True, 8)
    before = held.crop(0, 0).clone()
    torch.cuda.synchronize()
    # re-use: same object, same buffers, no allocation
    ptrs = (held._out.data_ptr(), held._tmp.data_ptr(), held.info.data_ptr())
    allocated = torch.cuda.memory_allocated(gpu)
    again = pkg.overlap_crop_batch(table, b0, b1, True, 8, out=held)
    assert again is held and (held._out.data_ptr(), held._tmp.data_ptr(), held.info.data_ptr()) == ptrs
    assert torch.cuda.memory_allocated(gpu) == allocated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.overlap_crop_batch(table, b0, b1, True, 8, out=held)
    b0.copy_(torch.tensor([[20.0, 12.0, 100.0, 80.0], [15.0, 6.0, 90.0, 60.0], [0.0, 10.0, 93.0, 57.0], [30.0, 35.0, 70.0, 90.0]]))
    graph.replay()
    torch.cuda.synchronize()
    captured.geometry(refresh=True)
    fresh = pkg.overlap_crop_batch(table, b0, b1, True, 8)
    assert captured.valid == fresh.valid == [1, 1, 1, 1]
    for k in range(4):
        assert info_fields(captured.geometry()[k]) == info_fields(fresh.geometry()[k])
        for i in (0, 1):
            assert torch.equal(captured.crop(k, i), fresh.crop(k, i)), (k, i)
    assert not torch.equal(fresh.crop(0, 0), before)       # the replay saw the new boxes
    with pytest.raises(ValueError):
        pkg.overlap_crop_batch(table, b0, b1, True, 1, out=held)      # another mode: not this result's buffers


class FixedBoxes(torch.nn.Module):
    """Stand-in for the model: ``forward_dummy`` returns fixed boxes (row j for the j-th pair of a batch)."""
    BOX0 = torch.tensor([[10.0, 12.0, 100.0, 90.0], [0.0, 0.0, 128.0, 128.0], [40.5, 8.25, 90.0, 120.0]])
    BOX1 = torch.tensor([[5.0, 8.0, 120.0, 110.0], [30.0, 20.0, 31.5, 100.0], [0.0, 64.0, 64.0, 128.0]])

    def __init__(self, device):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=device))

    def forward_dummy(self, im0, im1):
        n = im0.shape[0]
        return self.BOX0[:n].to(im0.device).clone(), self.BOX1[:n].to(im0.device).clone()


def test_crop_pairs_equals_the_per_pair_loop(gpu):
    rng = np.random.default_rng(4)
    sizes = [((70, 90), (60, 100)), ((50, 64), (96, 80)), ((64, 64), (33, 47)), ((90, 70), (70, 90)), ((45, 150), (80, 80)),
             ((64, 96), (64, 96)), ((40, 41), (99, 98))]
    raw = [tuple(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in pair) for pair in sizes]
    res = pkg.forward_pairs_raw(FixedBoxes(gpu), raw, resize=(128,), grayscale=True, align='disk', max_batch=3)
    for mode in ((True, 1, False), (True, 8, False)):
        chunks = pkg.crop_pairs(res, keep_aspect=mode[0], size_divisor=mode[1], pragueparks=mode[2], max_batch=3)
        assert [len(c) for c in chunks] == [3, 3, 1]
        valids = []
        for i in range(len(raw)):
            one = pkg.overlap_crop(res['inp0'][i], res['inp1'][i], res['box0'][i], res['box1'][i],
                                   res['overlap_scales0'][i], res['overlap_scales1'][i], *mode)
            batch, k = chunks[i // 3], i % 3
            assert info_fields(batch.geometry()[k]) == info_fields(one.geometry()), i
            valids.append(batch.valid[k])
            for side in (0, 1):
                assert torch.equal(batch.crop(k, side), one.crop(side)), (i, side)
            kp = np.float32([[0.0, 0.0], [7.5, 3.25]])
            assert np.array_equal(batch.to_origin(k, 0, kp, res['scales0'][i]),
                                  pkg.keypoints_to_origin(kp, torch.tensor(one.ratio(0)), one.bbox(0)[0], res['scales0'][i]))
        assert 0 in valids and 1 in valids       # the 1.5-px box fails the gate where its scale leaves it under 2 px
