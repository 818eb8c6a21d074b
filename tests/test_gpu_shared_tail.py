"""The shared ragged tail of the 64-row encoder (``oetr_set_tail_share``): where both images of the pairs end in a token
tile of 1..16 rows, one workgroup runs the two tails as rows 0.. and 16.. of one 32-row MFMA tile.  The arithmetic of
every output element is unchanged - same products, same k-slots, exact zeros elsewhere - so the check is BIT identity
between ``set_tail_share(0)`` and the automatic setting in one build, on every stage ``forward(stages=True)`` and
``feature_correlation`` return, with and without masks, in both two-plane precisions and both tail modes; the launch's
grid shows which path ran (one workgroup per pair fewer where the shape allows sharing, the full grid where it must
fall back).  Boxes are held to the oracle within test_gpu_parity's tolerance as everywhere else.
"""
import pytest
import torch

from oracle import oetr_oracle as orc
from tests.test_gpu_parity import TOL, maxerr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PRECISIONS = ('f32_split_f16', 'f32_split_qk16')
TAIL_MODES = (1, 2)   # P form, direct
# (id, pairs, grid 1, grid 2, shared) - image size = 32 x grid; L % 64 of the two images in the comment
CASES = [
    ('shared_only', 1, (3, 3), (3, 3), True),          # 9 | 9: no full tile, the shared workgroup is the pair's only one
    ('flagship_pattern', 2, (20, 20), (20, 20), True),  # 16 | 16: 400 tokens, the benchmark's tile pattern
    ('unequal_tails', 2, (5, 16), (8, 9), True),        # 16 | 8: L = 80 / 72
    ('one_row_tail', 1, (5, 13), (20, 20), True),       # 1 | 16: L = 65 / 400, 2 tiles against 7
    ('fallback_tail36', 1, (10, 10), (20, 20), False),  # 36 | 16
    ('fallback_tail17', 1, (9, 9), (20, 20), False),    # 17 | 16
    ('fallback_tail0', 1, (8, 8), (20, 20), False),     # 0 | 16
]


def tiles(grid):
    return (grid[0] * grid[1] + 63) // 64


@pytest.fixture(scope='module')
def weights():
    return orc.make_hot_weights(7, sharpen=True)


@pytest.fixture(scope='module')
def engines(weights, gpu):
    import imagematching_oetr_amd as pkg
    return {p: pkg.HotPathEngine(weights, device=gpu, precision=p, enc_tile=64) for p in PRECISIONS}


class Case:
    def __init__(self, cid, n, g1, g2, shared, weights):
        self.id, self.n, self.g1, self.g2, self.shared = cid, n, g1, g2, shared
        seed = 100 + [c[0] for c in CASES].index(cid)
        self.f1, self.f2 = orc.make_features(seed, n, *g1), orc.make_features(seed + 50, n, *g2)
        self.p1, self.p2 = orc.position_table(*g1), orc.position_table(*g2)
        self.hw1, self.hw2 = (32 * g1[0], 32 * g1[1]), (32 * g2[0], 32 * g2[1])
        # random masks whose last token is valid (a valid last row: the tail tile's mask is not all zero)
        g = torch.Generator().manual_seed(seed + 7)
        self.m1 = (torch.rand(n, *g1, generator=g) >= 0.25).float()
        self.m2 = (torch.rand(n, *g2, generator=g) >= 0.25).float()
        self.m1[:, -1, -1] = 1.0
        self.m2[:, -1, -1] = 1.0
        self.ref = {
            False: orc.hot_path(self.f1, self.f2, weights, self.hw1, self.hw2),
            True: orc.hot_path(self.f1, self.f2, weights, self.hw1, self.hw2, mask1=self.m1, mask2=self.m2)}
        self.grid_full = n * (tiles(g1) + tiles(g2))

    def run(self, eng, dev, masked):
        mk = dict(mask1=self.m1.to(dev), mask2=self.m2.to(dev)) if masked else {}
        args = (self.f1.to(dev), self.f2.to(dev), self.p1.to(dev), self.p2.to(dev))
        out = dict(eng.forward(*args, self.hw1, self.hw2, stages=True, **mk))
        grid = eng.debug_encoder_grid()
        fc = eng.feature_correlation(*args, **mk)
        assert eng.debug_encoder_grid() == grid
        for k, t in zip(('fc_hs1', 'fc_hs2', 'fc_memory1', 'fc_memory2'), fc):
            out[k] = t
        torch.cuda.synchronize()
        return out, grid


@pytest.fixture(scope='module')
def cases(weights):
    made = {}

    def get(cid):
        if cid not in made:
            made[cid] = Case(*next(c for c in CASES if c[0] == cid), weights)
        return made[cid]
    return get


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_shared_tail_is_bit_identical(cid, precision, cases, engines, gpu):
    c, eng = cases(cid), engines[precision]
    try:
        for tail in TAIL_MODES:
            eng.set_tail_mode(tail)
            for masked in (False, True):
                note = (cid, precision, tail, masked)
                eng.set_tail_share(0)
                off, grid_off = c.run(eng, gpu, masked)
                eng.set_tail_share(-1)
                auto, grid_auto = c.run(eng, gpu, masked)
                assert eng.query_flags() == 0, note
                # which path ran: one workgroup per pair fewer where both tails are 1..16 rows, else the fallback
                assert grid_off == c.grid_full, (note, grid_off)
                assert grid_auto == c.grid_full - (c.n if c.shared else 0), (note, grid_auto)
                assert sorted(off) == sorted(auto)
                for k in sorted(off):
                    assert torch.equal(off[k], auto[k]), (note, k, maxerr(off[k], auto[k]))
                for s, r in zip(('1', '2'), c.ref[masked]):
                    e = maxerr(auto['box' + s], r)
                    print(f'{note} box{s} max err vs oracle {e:.3e} px')
                    assert e <= TOL['box'], (note, s, e)
    finally:
        eng.set_tail_mode(0)
        eng.set_tail_share(-1)


def test_setter_refuses_other_values(engines):
    eng = engines[PRECISIONS[0]]
    for bad in (1, 2, -2):
        with pytest.raises(Exception):
            eng.set_tail_share(bad)
    eng.set_tail_share(-1)
