"""CPU-only checks of the feature-bank extension (``include/oetr_bank.h``,
``imagematching_oetr_amd/bank.py``, ``pipeline.forward_pairs_indexed``): the header, the export
list and the built library agree; host-side argument validation of both entry points works without
a GPU and enqueues nothing; there is no CPU route; the indexed front-end's host logic on a stub."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd import hip_engine
from imagematching_oetr_amd.pipeline import forward_pairs_indexed, plan_indexed

REPO = Path(__file__).resolve().parents[1]
BAD_ARG, BAD_SHAPE = 1, 2


def header_functions(name):
    text = (REPO / 'include' / name).read_text()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(oetr_[a-z_0-9]+)\s*\(', text)))


def test_bank_header_exports_and_library_agree():
    lib = pkg.load_library()
    names = header_functions('oetr_bank.h')
    assert len(names) == 3, names
    assert set(names) == set(hip_engine.BANK_EXPORTS)
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/oetr_bank.h but not exported'
    assert lib.oetr_bank_abi_version() == hip_engine.BANK_ABI_VERSION == 1
    # the extension stays out of the base header, its export list and its version
    assert len(header_functions('oetr_hip.h')) == 53
    assert not set(hip_engine.BANK_EXPORTS) & set(hip_engine.EXPORTS)
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    text = (REPO / 'include' / 'oetr_bank.h').read_text()
    assert re.search(r'#define\s+OETR_BANK_ABI_VERSION\s+1\b', text)
    assert re.search(r'#define\s+OETR_FLAG_INDEX\s+4u\b', text)
    assert hip_engine.FLAG_INDEX == 4
    assert hip_engine.FLAG_INVALID == hip_engine.FLAG_F16_RANGE | hip_engine.FLAG_EXCHANGE   # an index error is no re-run matter


def _fake(n_bytes=64):
    """Host memory standing in for a device buffer: validation must refuse the call before
    anything could touch it."""
    buf = ctypes.create_string_buffer(n_bytes)
    return buf, ctypes.addressof(buf)


def test_bank_gather_argument_errors_need_no_gpu():
    lib = pkg.load_library()
    keep, p = _fake()

    def call(bank1=p, k1=4, idx1=p, bank2=p, k2=4, idx2=p, n=2, L1=80, L2=35, t1=p, t2=p):
        return lib.oetr_bank_gather(bank1, k1, idx1, bank2, k2, idx2, n, L1, L2, t1, t2, None, None)

    for kw in (dict(bank1=None), dict(bank2=None), dict(idx1=None), dict(idx2=None), dict(t1=None),
               dict(t2=None), dict(n=0), dict(n=-3), dict(k1=0), dict(k2=-1)):
        assert call(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_bank_gather'), kw
    for kw in (dict(L1=0), dict(L2=-5), dict(L1=10001), dict(L2=10001), dict(n=1 << 20, L1=10000, L2=10000)):
        assert call(**kw) == BAD_SHAPE, kw
        assert len(lib.oetr_last_error()) > 0, kw
    del keep


def test_forward_bank_argument_errors_need_no_gpu():
    lib = pkg.load_library()
    keep, p = _fake()

    def call(h=p, bank1=p, k1=4, idx1=p, bank2=p, k2=4, idx2=p, n=2, grids=(8, 10, 5, 7),
             imgs=(256, 320, 160, 224), ws=p, ws_bytes=1 << 30, box1=p, box2=p):
        return lib.oetr_forward_bank(h, bank1, k1, idx1, bank2, k2, idx2, n, *grids, *imgs, ws, ws_bytes,
                                     box1, box2, None, None)

    for kw in (dict(h=None), dict(box1=None), dict(box2=None), dict(bank1=None), dict(bank2=None),
               dict(idx1=None), dict(idx2=None), dict(n=0), dict(k1=0), dict(k2=0)):
        assert call(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_forward_bank'), kw
    for kw in (dict(grids=(0, 10, 5, 7)), dict(grids=(8, 10, 101, 100)), dict(grids=(8, 10, 5, -7)),
               dict(imgs=(4, 320, 160, 224)), dict(imgs=(256, 0, 160, 224))):
        assert call(**kw) == BAD_SHAPE, kw
        assert len(lib.oetr_last_error()) > 0, kw
    del keep


def test_feature_bank_has_no_cpu_route():
    model = pkg.OETR(pkg.get_cfg_defaults().OETR).eval()
    with pytest.raises(RuntimeError, match='GPU'):
        model.feature_bank((64, 64), 4)


# ------------------------------------------------ forward_pairs_indexed on a stub model
SIZES = [(64, 64), (64, 128), (48, 64)]


def _boxes(image1, image2):
    """Boxes that depend on the pixels of the two images only (tests/test_pipeline_cpu.StubModel)."""
    m1 = image1.reshape(image1.shape[0], -1).mean(1, keepdim=True)
    m2 = image2.reshape(image2.shape[0], -1).mean(1, keepdim=True)
    k = torch.arange(4, dtype=torch.float32)
    return m1 * image1.shape[2] + k, m2 * image2.shape[1] - k


class StubBank:
    def __init__(self, model, image_hw, capacity):
        self.model, self.image_hw, self.capacity, self.images = model, tuple(image_hw), capacity, []

    def __len__(self):
        return len(self.images)

    def add(self, images):
        assert tuple(images.shape[1:]) == self.image_hw + (3,)
        assert len(self.images) + images.shape[0] <= self.capacity
        self.model.adds.append(int(images.shape[0]))
        first = len(self.images)
        self.images += [im.clone() for im in images]
        self.model.added += [float(im.mean()) for im in images]
        return list(range(first, first + images.shape[0]))


class StubModel:
    """``feature_bank`` / ``boxes_from_bank`` with the module's contract; a batch's boxes are garbage
    until ``hip_flush()`` settles them in place (what OETR does under hip_defer_check)."""

    def __init__(self):
        self.adds, self.added, self.batches, self._pending = [], [], [], None

    def hip_flush(self):
        if self._pending is not None:
            for t, good in self._pending:
                t.copy_(good)
            self._pending = None

    def feature_bank(self, image_hw, capacity):
        return StubBank(self, image_hw, capacity)

    def boxes_from_bank(self, bank1, idx1, bank2, idx2):
        assert len(idx1) == len(idx2) > 0
        self.hip_flush()
        self.batches.append(len(idx1))
        good = _boxes(torch.stack([bank1.images[i] for i in idx1]), torch.stack([bank2.images[i] for i in idx2]))
        out = tuple(torch.full_like(t, 7.0e4) for t in good)
        self._pending = list(zip(out, good))
        return out


def make_images(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        h, w = SIZES[(i * 5 + i // 4) % 3]
        out.append(torch.rand(1, h, w, 3, generator=g) if i % 2 else torch.rand(h, w, 3, generator=g))
    return out


def make_pair_index(n_images, n_pairs, skip, seed=1):
    g = torch.Generator().manual_seed(seed)
    live = [i for i in range(n_images) if i not in skip]
    pick = lambda: live[int(torch.randint(len(live), (1,), generator=g))]
    pairs = [(pick(), pick()) for _ in range(n_pairs - 2)]
    return pairs + [(live[0], live[0]), (live[3], live[3])]       # (i, i) is a legal pair


def per_pair_loop(images, pair_index):
    b4 = lambda t: t if t.dim() == 4 else t[None]
    out = [_boxes(b4(images[i]), b4(images[j])) for i, j in pair_index]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


@pytest.mark.parametrize('max_batch,trunk_batch', [(1, 1), (3, 4), (8, 16), (64, 2)])
def test_forward_pairs_indexed_equals_the_per_pair_loop(max_batch, trunk_batch):
    images = make_images(17)
    skip = {2, 9}                                    # never referenced: must never be added
    pair_index = make_pair_index(len(images), 41, skip)
    used = {m for p in pair_index for m in p}
    model = StubModel()
    b0, b1 = forward_pairs_indexed(model, images, pair_index, max_batch=max_batch, trunk_batch=trunk_batch)
    e0, e1 = per_pair_loop(images, pair_index)
    assert b0.shape == (41, 4) and torch.equal(b0, e0) and torch.equal(b1, e1)
    # every referenced image exactly once, unreferenced ones never
    assert sorted(model.added) == sorted(float(images[m].mean()) for m in used)
    assert sum(model.adds) == len(used) and all(1 <= a <= trunk_batch for a in model.adds)
    assert all(1 <= b <= max_batch for b in model.batches) and sum(model.batches) == len(pair_index)
    if max_batch >= 8:
        assert max(model.batches) >= 4               # buckets really are batched


def test_plan_indexed_is_a_pure_plan():
    shapes = [SIZES[i % 3] for i in range(9)]
    pair_index = [(0, 3), (1, 1), (3, 0), (0, 6), (4, 8), (6, 0), (1, 4)]
    banks, batches = plan_indexed(shapes, pair_index, 2)
    assert banks == {SIZES[0]: [0, 3, 6], SIZES[1]: [1, 4], SIZES[2]: [8]}      # first-referenced order; 2, 5, 7 unused
    assert batches == [((SIZES[0], SIZES[0]), [0, 2]), ((SIZES[0], SIZES[0]), [3, 5]),
                       ((SIZES[1], SIZES[1]), [1, 6]), ((SIZES[1], SIZES[2]), [4])]
    with pytest.raises(ValueError):
        plan_indexed(shapes, pair_index, 0)


def test_forward_pairs_indexed_edge_cases():
    images = make_images(6)
    for bad in ([(0, 6)], [(1, 2), (-1, 0)]):
        model = StubModel()
        with pytest.raises(IndexError):
            forward_pairs_indexed(model, images, bad)
        assert not model.adds and not model.batches           # refused before any model call
    z0, z1 = forward_pairs_indexed(StubModel(), images, [])
    assert z0.shape == (0, 4) and z1.shape == (0, 4)
    with pytest.raises(ValueError):
        forward_pairs_indexed(StubModel(), [torch.rand(2, 8, 8, 3)], [(0, 0)])
