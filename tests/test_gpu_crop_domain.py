"""GPU tests of the BOX DOMAIN of the crop step and of what a crop call writes (``oetr_overlap_crop``,
``oetr_overlap_crop_batch``; ``csrc/crop_sample.h::crop_geometry``).  The box is a float32 on the device that becomes
an address; the host cannot look at it, so the kernels are the only guard: a scaled coordinate that does not
truncate into [0, 2^31) makes the pair ``valid = -1`` - nothing read, nothing written
(``oracle/crop_oracle.py::in_domain``).  Every call here runs on buffers the test owns and has filled with a
sentinel, so "nothing written" and "the rest of a slot is not written" are checked element by element."""
import ctypes as C

import numpy as np
import pytest
import torch

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd.hip_engine import _CropInfo, _check, _stream
from oracle import crop_oracle as cro
from tests.test_crop_cpu import BOX1, DOMAIN_HW, DOMAIN_TABLE, domain_row_boxes
from tests.test_gpu_crop_batch import image, info_fields

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
PIX_TOL = 1e-5      # against the oracle: the tolerance of test_crop_geometry_fuzz_is_bit_exact_vs_oracle
# A quiet NaN with a payload, compared by BITS: a pixel computed from a guard value is a NaN of another payload
# or not a NaN at all, and no float a kernel computes from image data in [0, 1] has these bits.
SENTINEL = 0x7FC0BEEF
GUARD_ROWS = 8      # the largest |coordinate| that reaches a kernel as a moderate integer in any table here
ONE = (1.0, 1.0)


def fill_sentinel(t):
    t.view(torch.int32).fill_(SENTINEL)


def bits(t):
    return t.contiguous().view(torch.int32)


def all_sentinel(t):
    return bool((bits(t) == SENTINEL).all())


def no_sentinel(t):
    return not bool((bits(t) == SENTINEL).any())


class Guarded:
    """A contiguous ``[1, C, h, w]`` image that is a view into the middle of a larger sentinel-filled buffer, with
    ``(GUARD_ROWS + 1) * w`` floats of guard on each side.

    With the box domain in place no kernel reads outside the image at all.  The guards are the second safeguard:
    a build WITHOUT the range test would read plane 0 of a box with origin ``(x0, y0)``, ``-a <= x0, y0 < 0``, from
    index ``(y0 + yy) * w + x0 + xx >= -(a * w + a) > -(a + 1) * w`` on (``yy, xx >= 0`` are the clamped taps), and
    never past ``h * w`` of the last plane, because the taps are clamped to ``crop_h - 1`` / ``crop_w - 1`` and the
    stops to the far edge: memory this test owns, for every row with ``a <= GUARD_ROWS`` (the tables here stop at
    -8).  The huge and non-finite rows sit on coordinates where such a build's saturating conversion turns them into
    a failed gate, an empty crop or a stop clamped at the far edge (huge negatives and -inf only on starts, where
    the wrapped width fails the gate): nothing outside the image is read for them either."""

    def __init__(self, hw, channels, gpu):
        h, w = hw
        n, g = channels * h * w, (GUARD_ROWS + 1) * w
        self.buf = torch.empty(g + n + g, device=gpu)
        fill_sentinel(self.buf)
        self.cpu = image(hw, channels)
        self.image = self.buf[g:g + n].view(1, channels, h, w)
        self.image.copy_(self.cpu)
        self.guards = (self.buf[:g], self.buf[g + n:])
        assert self.image.is_contiguous() and self.intact()

    def intact(self):
        return all_sentinel(self.guards[0]) and all_sentinel(self.guards[1]) and torch.equal(self.image.cpu(), self.cpu)


def per_pair(gpu, p, mode):
    """``oetr_overlap_crop`` through the C ABI on sentinel-filled ``tmp`` / ``out1`` / ``out2`` / ``info`` of the
    test's own.  ``p``: a pair dict (``g0`` / ``g1`` :class:`Guarded`, ``b0`` / ``b1`` device ``[4]``, ``sc0`` / ``sc1``)."""
    keep, div, pp = mode
    lib = pkg.load_library()
    im0, im1 = p['g0'].image, p['g1'].image
    ch, h0, w0 = (int(v) for v in im0.shape[1:])
    h1, w1 = int(im1.shape[2]), int(im1.shape[3])
    cap = int(lib.oetr_overlap_crop_capacity(ch, h0, w0, h1, w1, div, None, None))
    assert cap > 0
    tmp, out = torch.empty(2 * cap, device=gpu), [torch.empty(cap, device=gpu) for _ in (0, 1)]
    info = torch.empty((C.sizeof(_CropInfo) + 7) // 8, dtype=torch.float64, device=gpu)
    for t in (tmp, out[0], out[1], info):
        fill_sentinel(t)
    s0, s1 = (C.c_float * 2)(*p['sc0']), (C.c_float * 2)(*p['sc1'])
    with torch.cuda.device(gpu):
        _check(lib, lib.oetr_overlap_crop(
            im0.data_ptr(), im1.data_ptr(), ch, h0, w0, h1, w1, p['b0'].data_ptr(), p['b1'].data_ptr(), s0, s1,
            int(keep), div, int(pp), tmp.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), cap, info.data_ptr(),
            _stream(gpu)), 'oetr_overlap_crop')
    torch.cuda.synchronize()
    rec = _CropInfo.from_buffer_copy(info.cpu().numpy().tobytes()[:C.sizeof(_CropInfo)])
    return dict(tmp=tmp, out=out, rec=info_fields(rec), cap=cap)


def refill(held):
    for t in (held._out, held._tmp, held.info):
        if t is not None:
            fill_sentinel(t)


def batched(gpu, pairs, mode):
    """One ``overlap_crop_batch`` call whose ``_out`` / ``_tmp`` / ``info`` were filled with the sentinel first: the
    result is built once, filled, and written into again with ``out=``.  Returns (result, box0, box1)."""
    keep, div, pp = mode
    table = pkg.crop_pair_table([p['g0'].image for p in pairs], [p['g1'].image for p in pairs],
                                [p['sc0'] for p in pairs], [p['sc1'] for p in pairs])
    box0 = torch.stack([p['b0'] for p in pairs]).contiguous()
    box1 = torch.stack([p['b1'] for p in pairs]).contiguous()
    held = pkg.overlap_crop_batch(table, box0, box1, keep, div, pp)
    torch.cuda.synchronize()
    assert (held._tmp is None) == (div == 1)          # divisor 1 is the direct form: tmp == NULL
    refill(held)
    assert pkg.overlap_crop_batch(table, box0, box1, keep, div, pp, out=held) is held
    torch.cuda.synchronize()
    return held, box0, box1


def pair(gpu, g0, g1, b0, b1, sc0=ONE, sc1=ONE):
    dev = lambda b: torch.as_tensor(b, dtype=torch.float32).to(gpu)
    return dict(g0=g0, g1=g1, b0=dev(b0), b1=dev(b1), sc0=sc0, sc1=sc1)


def oracle_record(p, mode):
    return cro.crop_record(p['g0'].image.shape[2:], p['g1'].image.shape[2:], p['b0'].cpu(), p['b1'].cpu(),
                           p['sc0'], p['sc1'], *mode)


def oracle_crops(p, mode):
    return cro.overlap_crop(p['g0'].cpu, p['g1'].cpu, p['b0'].cpu(), p['b1'].cpu(), p['sc0'], p['sc1'], *mode)


INTS = ('valid', 'box', 'crop_w', 'crop_h', 'new_w', 'new_h', 'out_w', 'out_h')
same_floats = lambda a, b, dt: np.array_equal(np.asarray(a, dtype=dt), np.asarray(b, dtype=dt), equal_nan=True)


def assert_record_is(got, want, tag):
    """A device record against the oracle's, field for field (a ratio the oracle leaves unspecified - the division
    by zero of an empty crop inside the domain - is not compared)."""
    for k in INTS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    if want['ratio'] is not None:
        assert got['ratio'] == want['ratio'], (tag, got['ratio'], want['ratio'])
    assert same_floats(got['sbox'], want['sbox'], np.float32), (tag, got['sbox'], want['sbox'])


def assert_same_record(a, b, tag):
    """Two device records, every field (NaN equals NaN)."""
    for k in INTS:
        assert a[k] == b[k], (tag, k, a[k], b[k])
    assert same_floats(a['ratio'], b['ratio'], np.float64) and same_floats(a['sbox'], b['sbox'], np.float32), (tag, a, b)


def check_pair(gpu, held, k, p, mode, channels, want_valid=None, pixels=True):
    """Pair ``k`` of a sentinel-prefilled batched call and the per-pair call of the same pair on sentinel-prefilled
    buffers: records equal to the oracle and to each other; for ``valid = -1`` every element of both output slots
    and both ``tmp`` slots still the sentinel, in both entries; otherwise exactly the crop's extent written - equal
    bit for bit between the entries, within PIX_TOL of the oracle (bit for bit the image for a pass-through) - and
    every float after it still the sentinel."""
    one = per_pair(gpu, p, mode)
    want = oracle_record(p, mode)
    got = info_fields(held.geometry()[k])
    assert_record_is(got, want, ('batched', k))
    assert_record_is(one['rec'], want, ('per pair', k))
    assert_same_record(got, one['rec'], k)
    if want_valid is not None:
        assert want['valid'] == want_valid, (k, want['valid'], want_valid)
    if want['valid'] < 0:
        assert all_sentinel(held._out[k]) and (held._tmp is None or all_sentinel(held._tmp[k])), k
        assert all_sentinel(one['tmp']) and all_sentinel(one['out'][0]) and all_sentinel(one['out'][1]), k
        with pytest.raises(pkg.OetrError):
            held.crop(k, 0)
        return one
    ref = oracle_crops(p, mode) if pixels and want['valid'] == 1 else None
    for i, g in enumerate((p['g0'], p['g1'])):
        n = channels * want['out_h'][i] * want['out_w'][i]
        assert 0 < n <= one['cap']
        for name, slot in (('batched', held._out[k, i]), ('per pair', one['out'][i])):
            assert no_sentinel(slot[:n]), (name, k, i)
            assert all_sentinel(slot[n:]), (name, k, i)
        assert torch.equal(held._out[k, i, :n], one['out'][i][:n]), (k, i)
        assert tuple(held.crop(k, i).shape) == (1, channels, want['out_h'][i], want['out_w'][i])
        if want['valid'] == 0:
            assert n == g.image.numel() and torch.equal(held.crop(k, i), g.image), (k, i)
            assert all_sentinel(one['tmp']) and (held._tmp is None or all_sentinel(held._tmp[k])), (k, i)
        elif ref is not None:
            err = float((held.crop(k, i).cpu() - ref['crop' + '01'[i]]).abs().max())
            assert err <= PIX_TOL, (k, i, err)
    return one


@pytest.mark.parametrize('channels', [1, 3])
@pytest.mark.parametrize('divisor', [1, 8])
def test_domain_table_on_the_device(gpu, channels, divisor):
    """Every row of the CPU table (tests/test_crop_cpu.py::DOMAIN_TABLE) as one pair of ONE batched call and as a
    per-pair call."""
    mode = (True, divisor, False)
    g0, g1 = Guarded(DOMAIN_HW[0], channels, gpu), Guarded(DOMAIN_HW[1], channels, gpu)
    pairs = [pair(gpu, g0, g1, *domain_row_boxes(row), row['sc0'], row['sc1']) for row in DOMAIN_TABLE]
    held, _, _ = batched(gpu, pairs, mode)
    assert held.valid == [row['valid'] for row in DOMAIN_TABLE]
    for k, (row, p) in enumerate(zip(DOMAIN_TABLE, pairs)):
        check_pair(gpu, held, k, p, mode, channels, want_valid=row['valid'])
    assert g0.intact() and g1.intact()


def test_a_call_of_mixed_outcomes(gpu):
    """Seven pairs in one call: 2 and 5 outside the domain (a negative origin, a NaN), 3 a failed gate, the rest
    crop.  The in-domain pairs equal - records, and every bit of their out and tmp slots - the same call made
    without pairs 2 and 5."""
    nan = float('nan')
    for channels, divisor in ((1, 1), (3, 8)):
        mode = (True, divisor, False)
        g0, g1 = Guarded((48, 56), channels, gpu), Guarded((41, 47), channels, gpu)
        pairs = [pair(gpu, g0, g1, [5.0, 6.0, 50.0, 40.0], BOX1),
                 pair(gpu, g1, g0, [2.0, 3.0, 44.0, 38.0], [10.0, 8.0, 52.0, 44.0]),
                 pair(gpu, g0, g1, [-5.0, -3.0, 40.0, 30.0], BOX1),
                 pair(gpu, g0, g1, [10.0, 10.0, 11.9, 40.0], BOX1),
                 pair(gpu, g0, g1, [0.0, 0.0, 56.0, 48.0], [0.0, 0.0, 47.0, 41.0]),
                 pair(gpu, g1, g0, [2.0, 3.0, nan, 38.0], [10.0, 8.0, 52.0, 44.0]),
                 pair(gpu, g0, g1, [10.0, 12.0, 70.0, 70.0], BOX1, sc0=(0.75, 0.6))]
        held, _, _ = batched(gpu, pairs, mode)
        assert held.valid == [1, 1, -1, 0, 1, -1, 1]
        for k, p in enumerate(pairs):
            check_pair(gpu, held, k, p, mode, channels)
        for k in (2, 5):
            for i in (0, 1):
                with pytest.raises(pkg.OetrError):
                    held.crop(k, i)
        keep = [0, 1, 3, 4, 6]
        fewer, _, _ = batched(gpu, [pairs[k] for k in keep], mode)
        assert fewer.valid == [1, 1, 0, 1, 1]
        for q, k in enumerate(keep):
            assert_same_record(info_fields(held.geometry()[k]), info_fields(fewer.geometry()[q]), k)
            assert torch.equal(bits(held._out[k]), bits(fewer._out[q])), k
            assert held._tmp is None or torch.equal(bits(held._tmp[k]), bits(fewer._tmp[q])), k
        assert g0.intact() and g1.intact()


@pytest.mark.parametrize('channels', [1, 3])
@pytest.mark.parametrize('divisor', [1, 8])
def test_what_a_call_writes_at_the_tile_edges(gpu, channels, divisor):
    """The batched kernel's tiles are 64 x 16 outputs, 4 rows per thread: output widths 63 / 64 / 65 times heights
    15 / 16 / 17, one output a single row high, and a pass-through pair, in ONE call - without the aspect rule, so
    the output takes the larger image's size.  Each slot holds exactly its crop (checked in :func:`check_pair`,
    for the per-pair entry's ``out1`` / ``out2`` too) and the sentinel after it."""
    mode = (False, divisor, False)
    pairs = []
    for w in (63, 64, 65):
        for h in (15, 16, 17):
            pairs.append(pair(gpu, Guarded((h, w), channels, gpu), Guarded((h - 3, w - 5), channels, gpu),
                              [2.0, 3.0, w - 4.0, h - 2.0], [1.0, 1.0, w - 20.0, h - 6.0]))
    # an output one row high: images one row high (the boxes pass the gate as integers and are clamped to the row)
    pairs.append(pair(gpu, Guarded((1, 64), channels, gpu), Guarded((1, 59), channels, gpu),
                      [2.0, 0.0, 60.0, 3.0], [1.0, 0.0, 44.0, 2.0]))
    # a failed gate (a box 1 px wide): both images pass through
    pairs.append(pair(gpu, Guarded((17, 65), channels, gpu), Guarded((15, 63), channels, gpu),
                      [10.0, 2.0, 11.9, 12.0], [1.0, 1.0, 40.0, 9.0]))
    held, _, _ = batched(gpu, pairs, mode)
    assert held.valid == [1] * 10 + [0]
    geo = held.geometry()
    up = lambda v: -(-v // divisor) * divisor
    ws, hs = (63, 63, 63, 64, 64, 64, 65, 65, 65, 64), (15, 16, 17) * 3 + (1,)
    for i in (0, 1):
        assert [int(g.new_w[i]) for g in geo][:10] == list(ws) and [int(g.new_h[i]) for g in geo][:10] == list(hs)
        assert [int(g.out_w[i]) for g in geo][:10] == [up(w) for w in ws]
        assert [int(g.out_h[i]) for g in geo][:10] == [up(h) for h in hs]
    assert list(geo[10].out_w) == [65, 63] and list(geo[10].out_h) == [17, 15]
    tails = 0
    for k, p in enumerate(pairs):
        one = check_pair(gpu, held, k, p, mode, channels)
        tails += one['cap'] > channels * int(geo[k].out_h[1]) * int(geo[k].out_w[1])
        assert p['g0'].intact() and p['g1'].intact(), k
    assert tails >= 1       # the per-pair entry's extent check had a rest to look at (the pass-through pair's side 1)


def test_captured_and_replayed_across_the_domain_edge(gpu):
    """The batched call captured with ``out=`` on device boxes.  Replay 1, boxes in the domain: the eager call's
    bits.  Replay 2, pair 0's box made negative in the boxes buffer: its record says -1 and its slots still hold
    replay 1's crop bit for bit - nothing written - while the other pairs are unchanged.  Replay 3, the first boxes
    again: replay 1's result."""
    mode = (True, 8, False)
    g0, g1 = Guarded((48, 56), 1, gpu), Guarded((41, 47), 1, gpu)
    pairs = [pair(gpu, g0, g1, [5.0, 6.0, 50.0, 40.0], BOX1),
             pair(gpu, g1, g0, [2.0, 3.0, 44.0, 38.0], [10.0, 8.0, 52.0, 44.0]),
             pair(gpu, g0, g0, [10.0, 10.0, 11.9, 40.0], [0.0, 0.0, 56.0, 48.0]),
             pair(gpu, g1, g1, [0.5, 0.25, 30.0, 41.0], [7.0, 9.0, 47.0, 30.0])]
    held, box0, box1 = batched(gpu, pairs, mode)
    table = held._table
    first_boxes = box0.clone()
    eager = dict(out=bits(held._out).clone(), tmp=bits(held._tmp).clone(), rec=[info_fields(g) for g in held.geometry()])
    assert held.valid == [1, 1, 0, 1]
    refill(held)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.overlap_crop_batch(table, box0, box1, *mode, out=held)
    assert captured is held

    def replay():
        graph.replay()
        torch.cuda.synchronize()
        return dict(out=bits(held._out).clone(), tmp=bits(held._tmp).clone(),
                    rec=[info_fields(g) for g in held.geometry(refresh=True)])

    def same(a, b, ks):
        for k in ks:
            assert_same_record(a['rec'][k], b['rec'][k], k)
            assert torch.equal(a['out'][k], b['out'][k]) and torch.equal(a['tmp'][k], b['tmp'][k]), k
    r1 = replay()
    same(r1, eager, range(4))
    assert not bool((r1['out'][0, 0, :48 * 56] == SENTINEL).any())
    box0[0].copy_(torch.tensor([-5.0, -3.0, 40.0, 30.0]))
    r2 = replay()
    assert held.valid == [-1, 1, 0, 1]
    outside = dict(pairs[0], b0=box0[0])
    assert_record_is(r2['rec'][0], oracle_record(outside, mode), 'replay 2')
    assert r2['rec'][0]['new_w'] == r2['rec'][0]['out_h'] == [0, 0]
    assert torch.equal(r2['out'][0], r1['out'][0]) and torch.equal(r2['tmp'][0], r1['tmp'][0])      # nothing written
    same(r2, r1, (1, 2, 3))
    with pytest.raises(pkg.OetrError):
        held.crop(0, 0)
    box0.copy_(first_boxes)
    r3 = replay()
    same(r3, r1, range(4))
    assert held.valid == [1, 1, 0, 1] and g0.intact() and g1.intact()


def test_a_pair_outside_the_domain_is_listed_among_few_downstream(gpu):
    """``assemble_matches`` on a crop result with one pair outside the domain: that pair is listed among ``few``
    ("no crops made"), its rows are NaN and its list empty; the other pairs' origin rows and lists equal those of a
    call without it."""
    rng = np.random.default_rng(9)
    g0, g1 = Guarded((48, 56), 1, gpu), Guarded((41, 47), 1, gpu)
    pairs = [pair(gpu, g0, g1, [5.0, 6.0, 50.0, 40.0], BOX1),
             pair(gpu, g0, g1, [5.0, -5.0, 50.0, 40.0], BOX1),
             pair(gpu, g1, g0, [2.0, 3.0, 44.0, 38.0], [10.0, 8.0, 52.0, 44.0], sc0=(1.6, 1.3), sc1=(0.75, 0.6))]
    mode = (True, 1, False)
    scales = np.array([[(1.6, 1.6), (0.75, 0.8)], [(1.0, 1.0), (1.25, 1.25)], [(0.9, 1.1), (1.6, 0.75)]])
    K0, K1 = (70, 45, 257), (64, 50, 100)
    kp0 = [rng.uniform(0, 40, size=(n, 2)).astype(np.float32) for n in K0]
    kp1 = [rng.uniform(0, 40, size=(n, 2)).astype(np.float32) for n in K1]
    matches = [np.where(rng.random(a) < 0.8, rng.integers(0, b, size=a), -1) for a, b in zip(K0, K1)]
    conf = [rng.random(n).astype(np.float32) for n in K0]
    dev = lambda seq, ks: [torch.from_numpy(seq[k]).to(gpu) for k in ks]

    def assemble(ks):
        held, _, _ = batched(gpu, [pairs[k] for k in ks], mode)
        res = pkg.assemble_matches(held, torch.from_numpy(scales[list(ks)]).to(gpu), dev(kp0, ks), dev(kp1, ks),
                                   dev(matches, ks), dev(conf, ks))
        return held, res, {k: v.cpu().numpy() for k, v in res.items() if torch.is_tensor(v)}
    held, res, got = assemble((0, 1, 2))
    _, res2, want = assemble((0, 2))
    assert held.valid == [1, -1, 1]
    assert pkg.few_match_pairs(res) == [1] and pkg.few_match_pairs(res2) == []
    assert got['counts'][1].tolist() == [-1] * 4 and got['offsets'][1] == got['offsets'][2]
    off0, off1 = np.concatenate([[0], np.cumsum(K0)]), np.concatenate([[0], np.cumsum(K1)])
    assert np.isnan(got['origin0'][off0[1]:off0[2]]).all() and np.isnan(got['origin1'][off1[1]:off1[2]]).all()
    w0 = np.concatenate([[0], np.cumsum([K0[0], K0[2]])])
    w1 = np.concatenate([[0], np.cumsum([K1[0], K1[2]])])
    for q, k in enumerate((0, 2)):
        assert got['counts'][k].tolist() == want['counts'][q].tolist() and got['counts'][k][2] >= 30, k
        assert got['origin0'][off0[k]:off0[k + 1]].tobytes() == want['origin0'][w0[q]:w0[q + 1]].tobytes(), k
        assert got['origin1'][off1[k]:off1[k + 1]].tobytes() == want['origin1'][w1[q]:w1[q + 1]].tobytes(), k
        a, b = slice(got['offsets'][k], got['offsets'][k + 1]), slice(want['offsets'][q], want['offsets'][q + 1])
        assert a.stop - a.start == b.stop - b.start > 0
        for name in ('index0', 'index1', 'k1', 'k2', 'mconf'):
            assert got[name][a].tobytes() == want[name][b].tobytes(), (k, name)
