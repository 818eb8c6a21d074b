"""GPU tests of the feature bank (``include/oetr_bank.h``, ``imagematching_oetr_amd/bank.py``,
``pipeline.forward_pairs_indexed``): the gather kernel is an exact copy that never leaves its
buffers and never follows a bad index; ``oetr_forward_bank`` is the token-resident forward on the
gathered rows, bit for bit, eagerly and replayed from a HIP graph; the module route equals
``boxes_from_backbone`` on the same trunk output bit for bit and ``forward_dummy`` end to end within
the project's tolerance for two trunk runs; the range guards and the bank's life-cycle rules hold."""
import math

import pytest
import torch

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd import hip_engine
from oracle import oetr_oracle as orc

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BOX_TOL = 5e-2      # px: the project's tolerance for two runs of the torch / MIOpen trunk (test_gpu_pipeline.py)


def make_model(gpu, seed=6):
    torch.manual_seed(0)
    model = pkg.OETR(pkg.get_cfg_defaults().OETR).eval()
    sd = model.state_dict()
    sd.update(orc.make_hot_weights(seed, sharpen=True))
    model.load_state_dict(sd, strict=True)
    return model.to(gpu)


def feature_rows(seed, images, hf, wf, gpu):
    """Oracle features [images,256,hf,wf] as a bank [images, hf*wf, 256]."""
    return orc.make_features(seed, images, hf, wf).flatten(2).permute(0, 2, 1).contiguous().to(gpu)


def dev_idx(values, gpu):
    return torch.tensor(values, dtype=torch.int32, device=gpu)


class Guarded:
    """tokens1 / tokens2 as row ranges of ONE buffer with a sentinel row directly before and after each."""
    SENTINEL = -12345.5

    def __init__(self, n, L1, L2, gpu):
        self.buf = torch.full((n * (L1 + L2) + 3, 256), self.SENTINEL, device=gpu)
        self.tokens1 = self.buf[1:1 + n * L1]
        self.tokens2 = self.buf[2 + n * L1:2 + n * (L1 + L2)]
        self.guards = (0, 1 + n * L1, 2 + n * (L1 + L2))

    def intact(self):
        return all(bool((self.buf[r] == self.SENTINEL).all()) for r in self.guards)


@pytest.mark.parametrize('n', [1, 13])
@pytest.mark.parametrize('grids', [((8, 10), (5, 7)), ((20, 20), (20, 20))])
def test_gather_is_an_exact_copy_inside_its_buffers(gpu, n, grids):
    eng = pkg.HotPathEngine(orc.make_hot_weights(7, sharpen=True), device=gpu)
    (h1, w1), (h2, w2) = grids
    L1, L2 = h1 * w1, h2 * w2
    g = torch.Generator().manual_seed(n)
    bank1 = torch.randn(6, L1, 256, generator=g).to(gpu)
    bank2 = torch.randn(9, L2, 256, generator=g).to(gpu)
    i1 = torch.randint(6, (n,), generator=g).tolist()          # with repeats
    i2 = torch.randint(9, (n,), generator=g).tolist()
    out = Guarded(n, L1, L2, gpu)
    eng.bank_gather(bank1, dev_idx(i1, gpu), bank2, dev_idx(i2, gpu), out.tokens1, out.tokens2)
    assert torch.equal(out.tokens1, bank1[i1].reshape(-1, 256)) and torch.equal(out.tokens2, bank2[i2].reshape(-1, 256))
    assert out.intact()
    if L1 == L2:                                               # one bank on both sides, host-side indices
        i2 = [i % 6 for i in i2]
        out = Guarded(n, L1, L2, gpu)
        eng.bank_gather(bank1, i1, bank1, i2, out.tokens1, out.tokens2)
        assert torch.equal(out.tokens1, bank1[i1].reshape(-1, 256)) and torch.equal(out.tokens2, bank1[i2].reshape(-1, 256))
        assert out.intact()
    with pytest.raises(IndexError):                            # host-side indices are checked on the host
        eng.bank_gather(bank1, [6] * n, bank2, i2, out.tokens1, out.tokens2)
    with pytest.raises(ValueError):
        eng.bank_gather(bank1, dev_idx(i1, gpu), bank2, dev_idx(i2, gpu), out.tokens1[:-1], out.tokens2)


def test_gather_of_more_pairs_than_one_grid_holds(gpu):
    """2 x pairs is the launch's y extent; beyond 65535 the call goes out as several launches."""
    eng = pkg.HotPathEngine(orc.make_hot_weights(7, sharpen=True), device=gpu)
    n, L1, L2 = 40000, 2, 1
    g = torch.Generator().manual_seed(5)
    bank1, bank2 = torch.randn(7, L1, 256, generator=g).to(gpu), torch.randn(3, L2, 256, generator=g).to(gpu)
    i1, i2 = torch.randint(7, (n,), generator=g).to(gpu), torch.randint(3, (n,), generator=g).to(gpu)
    out = Guarded(n, L1, L2, gpu)
    eng.bank_gather(bank1, i1.int(), bank2, i2.int(), out.tokens1, out.tokens2)
    assert torch.equal(out.tokens1, bank1[i1].reshape(-1, 256)) and torch.equal(out.tokens2, bank2[i2].reshape(-1, 256))
    assert out.intact()


def test_index_outside_the_bank_is_clamped_and_flagged(gpu):
    """A missing clamp would still read memory that exists: the bank tensor holds 4 images, the call
    declares 2, the index is 3."""
    eng = pkg.HotPathEngine(orc.make_hot_weights(7, sharpen=True), device=gpu)
    L1, L2 = 80, 35
    g = torch.Generator().manual_seed(2)
    bank1, bank2 = torch.randn(4, L1, 256, generator=g).to(gpu), torch.randn(4, L2, 256, generator=g).to(gpu)
    word = torch.zeros(4, dtype=torch.int32, device=gpu)
    out = Guarded(3, L1, L2, gpu)
    eng.bank_gather(bank1, dev_idx([0, 3, 1], gpu), bank2, dev_idx([1, 0, -2], gpu), out.tokens1, out.tokens2,
                    status_word=word, images=(2, 2))
    assert word.tolist() == [hip_engine.FLAG_INDEX, 0, 0, 0]
    assert torch.equal(out.tokens1, bank1[[0, 1, 1]].reshape(-1, 256))       # clamped, never followed
    assert torch.equal(out.tokens2, bank2[[1, 0, 0]].reshape(-1, 256))
    assert out.intact()
    word.zero_()
    eng.bank_gather(bank1, dev_idx([0, 1, 1], gpu), bank2, dev_idx([1, 0, 0], gpu), out.tokens1, out.tokens2,
                    status_word=word, images=(2, 2))
    assert word.tolist() == [0, 0, 0, 0] and out.intact()
    # through the forward entry the bit travels in the published word (and is no FLAG_INVALID matter)
    rows = feature_rows(70, 4, 8, 10, gpu)
    bufs = eng.token_buffers(2, 8, 10, 8, 10)
    eng.load_pos_tokens(bufs, orc.position_table(8, 10).to(gpu), orc.position_table(8, 10).to(gpu))
    _, ticket = eng.forward_bank(rows[:2], dev_idx([0, 3], gpu), rows[:2], dev_idx([1, 0], gpu), 8, 10, 8, 10,
                                 (256, 320), (256, 320), publish=True)
    assert ticket.value() == hip_engine.FLAG_INDEX and not ticket.value() & hip_engine.FLAG_INVALID
    _, ticket = eng.forward_bank(rows[:2], dev_idx([0, 1], gpu), rows[:2], dev_idx([1, 0], gpu), 8, 10, 8, 10,
                                 (256, 320), (256, 320), publish=True)
    assert ticket.value() == 0
    with pytest.raises(IndexError):
        eng.forward_bank(rows[:2], [0, 2], rows[:2], [1, 0], 8, 10, 8, 10, (256, 320), (256, 320))


@pytest.mark.parametrize('precision,enc_tile,attention', [
    ('f32_split_f16', 32, 'linear'), ('f32_split_f16', 64, 'linear'), ('f32', None, 'linear'),
    ('f32_split_f16', None, 'full')])
def test_forward_bank_is_forward_tokens_on_the_gathered_rows(gpu, precision, enc_tile, attention):
    eng = pkg.HotPathEngine(orc.make_hot_weights(7, sharpen=True), device=gpu, precision=precision,
                            enc_tile=enc_tile, attention=attention)
    for (h1, w1), (h2, w2), hw1, hw2, i1, i2, shared in (
            ((8, 10), (5, 7), (256, 320), (160, 224), [4, 0, 0], [1, 2, 1], False),
            ((20, 20), (20, 20), (640, 640), (640, 640), [0, 3, 3, 1, 4, 2, 0, 4], [1, 3, 0, 0, 2, 4, 4, 3], True)):
        n = len(i1)
        bank1 = feature_rows(70, 5, h1, w1, gpu)
        bank2 = bank1 if shared else feature_rows(71, 3, h2, w2, gpu)
        p1, p2 = orc.position_table(h1, w1).to(gpu), orc.position_table(h2, w2).to(gpu)
        bufs = eng.token_buffers(n, h1, w1, h2, w2)
        eng.load_pos_tokens(bufs, p1, p2)
        bufs['tokens1'].copy_(bank1[i1].reshape(-1, 256))
        bufs['tokens2'].copy_(bank2[i2].reshape(-1, 256))
        want, ticket = eng.forward_tokens(n, h1, w1, h2, w2, hw1, hw2, publish=True)
        assert ticket.value() == 0
        bufs['tokens'].fill_(float('nan'))                       # nothing of the copy may survive
        got, ticket = eng.forward_bank(bank1, dev_idx(i1, gpu), bank2, dev_idx(i2, gpu), h1, w1, h2, w2, hw1, hw2,
                                       publish=True)
        assert ticket.value() == 0
        assert torch.isfinite(want[0]).all() and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        plain = eng.forward_bank(bank1, i1, bank2, i2, h1, w1, h2, w2, hw1, hw2)      # host indices, no publication
        assert torch.equal(plain[0], want[0]) and torch.equal(plain[1], want[1])
        assert eng.query_flags() == 0
    with pytest.raises(ValueError):
        eng.forward_bank(bank1, i1, bank2, i2, 8, 10, 8, 10, (256, 320), (256, 320))     # banks of another grid


def test_forward_bank_replays_from_a_hip_graph_with_new_indices(gpu):
    """Enqueue-only with the default settings: the indices are device memory, a replay gathers by
    what they hold THEN."""
    eng = pkg.HotPathEngine(orc.make_hot_weights(7, sharpen=True), device=gpu)
    bank1, bank2 = feature_rows(70, 5, 8, 10, gpu), feature_rows(71, 4, 5, 7, gpu)
    p1, p2 = orc.position_table(8, 10).to(gpu), orc.position_table(5, 7).to(gpu)
    i1, i2 = dev_idx([0, 1, 2], gpu), dev_idx([3, 2, 1], gpu)

    def step(publish):
        bufs = eng.token_buffers(3, 8, 10, 5, 7)
        eng.load_pos_tokens(bufs, p1, p2)
        return eng.forward_bank(bank1, i1, bank2, i2, 8, 10, 5, 7, (256, 320), (160, 224), publish=publish)
    first = tuple(b.clone() for b in step(False))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        boxes, ticket = step(True)
    graph.replay()
    torch.cuda.synchronize()
    assert ticket.value() == 0 and torch.equal(boxes[0], first[0]) and torch.equal(boxes[1], first[1])
    i1.copy_(dev_idx([4, 4, 0], gpu))
    i2.copy_(dev_idx([0, 1, 3], gpu))
    graph.replay()
    torch.cuda.synchronize()
    fresh = step(False)
    assert ticket.value() == 0 and torch.equal(boxes[0], fresh[0]) and torch.equal(boxes[1], fresh[1])
    assert not torch.equal(fresh[0], first[0])
    ticket.release()


def test_boxes_from_bank_equals_boxes_from_backbone_on_one_trunk_output(gpu):
    """The neck and the hot path are batch-invariant bit for bit, so rows stored once per image and
    gathered by index give the boxes of the pair-wise route on the same trunk output."""
    model = make_model(gpu)
    g = torch.Generator().manual_seed(21)
    bb_a = model.backbone(torch.rand(6, 320, 320, 3, generator=g).to(gpu))
    bb_b = model.backbone(torch.rand(3, 256, 384, 3, generator=g).to(gpu))
    bank_a, bank_b = model.feature_bank((320, 320), 8), model.feature_bank((256, 384), 3)
    assert bank_a.add_backbone(bb_a[:4]) == [0, 1, 2, 3] and bank_a.add_backbone(bb_a[4:]) == [4, 5]
    assert bank_b.add_backbone(bb_b) == [0, 1, 2] and len(bank_a) == 6 and bank_a.grid == (10, 10)
    for b1, bb1, b2, bb2, i1, i2 in ((bank_a, bb_a, bank_a, bb_a, [0, 2, 2, 5], [1, 0, 2, 3]),
                                     (bank_a, bb_a, bank_b, bb_b, [5, 0, 3], [2, 2, 0]),
                                     (bank_b, bb_b, bank_a, bb_a, [1], [4])):
        got = model.boxes_from_bank(b1, i1, b2, i2)
        assert (model.h1, model.w1, model.h2, model.w2) == b1.image_hw + b2.image_hw
        want = model.boxes_from_backbone(bb1[i1].contiguous(), bb2[i2].contiguous(), b1.image_hw, b2.image_hw)
        model.hip_flush()
        assert torch.isfinite(want[0]).all()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (i1, i2)
    with pytest.raises(IndexError):
        model.boxes_from_bank(bank_a, [0, 6], bank_a, [0, 0])       # 6 filled slots of 8
    with pytest.raises(IndexError):
        model.boxes_from_bank(bank_a, [0], bank_b, [-1])


@pytest.mark.parametrize('streams', [1, 3])
def test_forward_pairs_indexed_equals_forward_dummy_per_pair(gpu, streams):
    model = make_model(gpu, seed=5)
    model.hip_streams = streams
    g = torch.Generator().manual_seed(9)
    sizes = [(320, 320), (320, 448), (256, 320)]
    which = [0, 1, 0, 2, 0, 1, 0, 2, 0, 1, 0, 0]                      # 12 images: 6 + 3 + 2 referenced, one not
    images = [torch.rand(*sizes[k], 3, generator=g) if i % 2 else torch.rand(1, *sizes[k], 3, generator=g)
              for i, k in enumerate(which)]
    pair_index = [(int(a), int(b)) for a, b in torch.randint(11, (28, 2), generator=g).tolist()] + [(4, 4), (0, 1)]
    calls = []
    hook = model.backbone.register_forward_hook(lambda m, inp, out: calls.append(int(out.shape[0])))
    b0, b1 = pkg.forward_pairs_indexed(model, images, pair_index, max_batch=4, trunk_batch=3)
    hook.remove()
    used = {m for p in pair_index for m in p}
    per_size = [sum(1 for m in used if which[m] == k) for k in range(3)]
    assert len(calls) == sum(math.ceil(c / 3) for c in per_size) and sum(calls) == len(used)
    assert b0.shape == (30, 4) and b0.device.type == 'cuda'
    model.hip_streams = 1
    b4 = lambda t: (t if t.dim() == 4 else t[None]).to(gpu)
    for k, (i, j) in enumerate(pair_index):
        e0, e1 = model.forward_dummy(b4(images[i]), b4(images[j]))
        model.hip_flush()
        err = max(float((b0[k] - e0[0]).abs().max()), float((b1[k] - e1[0]).abs().max()))
        assert err <= BOX_TOL, (k, i, j, err)


def test_range_guards_of_the_bank_route(gpu):
    model = make_model(gpu)
    g = torch.Generator().manual_seed(23)
    bb = model.backbone(torch.rand(6, 320, 320, 3, generator=g).to(gpu))
    bank = model.feature_bank((320, 320), 6)
    bank.add_backbone(bb)
    batch_a, batch_b = ([0, 1], [3, 4]), ([2, 5], [0, 2])
    settled = model.boxes_from_bank(bank, batch_a[0], bank, batch_a[1])
    model.hip_flush()
    clean_a = tuple(b.clone() for b in settled)
    bank.rows[5].mul_(1e6 / float(bank.rows[5].abs().max()))          # one slot beyond the f16 range (largest value 1e6)
    first = model.boxes_from_bank(bank, batch_a[0], bank, batch_a[1])
    bad = model.boxes_from_bank(bank, batch_b[0], bank, batch_b[1])
    last = model.boxes_from_bank(bank, batch_a[0], bank, batch_a[1])
    model.hip_flush()
    for boxes in (first, last):                             # the other batches are unchanged
        assert torch.equal(boxes[0], clean_a[0]) and torch.equal(boxes[1], clean_a[1])
    hf, wf = bank.grid
    nchw = lambda idx: bank.rows[idx].permute(0, 2, 1).reshape(len(idx), 256, hf, wf).contiguous()
    f1, f2 = nchw(batch_b[0]), nchw(batch_b[1])
    want = model.exact_engine().forward(f1, f2, model.pos_encoding(f1), model.pos_encoding(f2), (320, 320), (320, 320))
    assert torch.isfinite(bad[0]).all() and torch.isfinite(bad[1]).all()
    assert torch.equal(bad[0], want[0]) and torch.equal(bad[1], want[1])
    model.hip_on_overflow = 'raise'
    model.boxes_from_bank(bank, batch_b[0], bank, batch_b[1])          # enqueue-only ...
    with pytest.raises(pkg.OetrRangeError):
        model.hip_flush()                                              # ... reported here
    # an out-of-range TRUNK output: the neck's guard is read in add_backbone
    other = model.feature_bank((320, 320), 4)
    with pytest.raises(pkg.OetrRangeError):
        other.add_backbone(bb[:2] * 1e6)
    assert len(other) == 0
    model.hip_on_overflow = 'f32'
    assert other.add_backbone(bb[:2] * 1e6) == [0, 1]
    want = model._neck_torch(bb[:2] * 1e6).flatten(2).transpose(1, 2)
    # The torch-neck route, stored transposed.  Two runs of the same fp32 torch / MIOpen modules are not
    # bit-stable; dot products of up to 4096 fp32 terms in another order differ by far less than
    # 4096 x 2^-24 = 2.4e-4 of the largest magnitude (the HIP neck's overflowed result is not finite).
    assert torch.isfinite(other.rows).all()
    assert float((other.rows - want).abs().max()) <= 2.4e-4 * float(want.abs().max())
    assert other.add_backbone(bb[2:4]) == [2, 3]                       # in range again: the HIP neck
    assert torch.equal(other.rows[2:], bank.rows[2:4])


def test_bank_life_cycle(gpu):
    model = make_model(gpu)
    g = torch.Generator().manual_seed(24)
    images = torch.rand(3, 256, 320, 3, generator=g)
    bank = model.feature_bank((256, 320), 4)
    assert bank.add(images) == [0, 1, 2]                    # host images are moved to the model's device
    with pytest.raises(RuntimeError, match='full'):
        bank.add(images[:2])
    with pytest.raises(ValueError):
        bank.add(torch.rand(1, 320, 320, 3))                # one bank = one image size
    assert len(bank) == 3
    model.train()
    with pytest.raises(RuntimeError, match='eval'):
        bank.add(images[:1])
    model.eval()
    boxes = tuple(b.clone() for b in model.boxes_from_bank(bank, [0, 1], bank, [2, 2]))
    model.load_state_dict(model.state_dict())
    with pytest.raises(RuntimeError, match='stale'):
        model.boxes_from_bank(bank, [0, 1], bank, [2, 2])
    with pytest.raises(RuntimeError, match='stale'):
        bank.add(images[:1])
    bank.clear()
    assert len(bank) == 0 and bank.add(images[1:]) == [0, 1] and bank.add(images[:1]) == [2]
    again = model.boxes_from_bank(bank, [2, 0], bank, [1, 1])
    model.hip_flush()
    assert float((again[0] - boxes[0]).abs().max()) <= BOX_TOL and float((again[1] - boxes[1]).abs().max()) <= BOX_TOL
    with pytest.raises(ValueError):
        model.boxes_from_bank(bank, [0], make_model(gpu).feature_bank((256, 320), 1), [0])
