"""CPU-only checks of the fine-match extension (``include/oetr_fine_match.h``, ``csrc/fine_match.hip``,
``csrc/fine_match_math.h``, ``imagematching_oetr_amd/fine_match.py``) and of its specification
``tests/fine_match_oracle.py``.

The specification: the pinned calls regenerate the recorded results; it equals a plain float64 restatement of the
published head on drawn pairs - the match list, the windows and the counters EQUAL, ``expec`` and ``mkpts1`` within four
times the recorded margin; a one-hot heat gives a grid point and the floor of the std bit for bit; a uniform window gives
``x = y = 0``; swapping ``ky`` / ``kx`` swaps ``x`` / ``y``; a planted offset is recovered within one fine cell; the
stated 16-partial sum gives the same bits under two emulated lane walks.

The arithmetic: ``fine_match_math.h`` compiled for the host, with the kernel's walk restated serially, equals the numpy
program bit for bit.

The ABI: header, export list and library agree and the other lists stand as they were; argument types are declared;
every host-checked argument error is reported without a GPU and touches nothing; the wrappers refuse before any device
use.  (The host code under ASan + UBSan is a stand-alone program: ``make hostcheck-fine_match``.)"""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd import hip_engine

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import dual_softmax_oracle as dso  # noqa: E402
import fine_match_cases as fmc  # noqa: E402
import fine_match_oracle as fmo  # noqa: E402
from nn_match_oracle import fma32  # noqa: E402

HEADER = 'oetr_fine_match.h'
BAD_ARG, BAD_SHAPE, WORKSPACE = 1, 2, 4
EXPECTED = json.loads((REPO / 'tests' / 'fine_match_expected.json').read_text())
F32 = np.float32
CSRC = REPO / 'imagematching_oetr_amd' / 'csrc'


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------- the specification
def test_pinned_calls_are_the_recorded_ones():
    assert sorted(EXPECTED['calls']) == sorted(fmc.SHAPES) and EXPECTED['partials'] == fmo.PARTIALS == 16
    assert {s[0] for s in fmc.SHAPES.values()} == {4, 8, 60, 64, 68, 128, 512}
    assert {s[1] for s in fmc.SHAPES.values()} == {3, 5, 7} and {s[2] for s in fmc.SHAPES.values()} == {1, 2, 4}
    for W in fmo.WINDOWS:
        assert EXPECTED['grids'][str(W)] == [float(g) for g in fmo.grid(W)]
        assert fmo.grid(W)[0] == -1 and fmo.grid(W)[-1] == 1 and fmo.grid(W)[W // 2] == 0
    dropped = unvouched = padded = 0
    for name, rec in EXPECTED['calls'].items():
        call = fmc.make_call(name)
        assert (rec['C'], rec['W'], rec['stride']) == (call['C'], call['W'], call['stride'])
        assert rec['inputs_sha256'] == dict(matches0=fmc.sha(call['matches0']), fine0=fmc.sha(call['fine0']),
                                            fine1=fmc.sha(call['fine1']))
        assert rec['matched'] == fmc.matched_total(call) and len(rec['results']) == 3
        for cap, want in rec['results'].items():
            win, fine = fmc.expected(call, int(cap))
            assert fmc.result_record(win, fine) == want, (name, cap)
            c = fine['counts']
            live = c[:, 0] >= 0
            assert int(c[live, 1].sum()) == int(win['moffsets'][-1]) == min(int(cap), rec['matched'])
            assert (win['rows'][win['moffsets'][-1]:] == -1).all() and not win['win0'][win['moffsets'][-1]:].any()
            dropped += int((c[live, 0] - c[live, 1]).sum())
            unvouched += int((~live).sum())
            n = int(win['moffsets'][-1])
            padded += int((np.abs(win['win1'][:n]).sum(-1) == 0).sum())
            assert np.isnan(fine['expec'][n:]).all() and np.isnan(fine['mkpts1'][n:]).all()
            assert not np.isnan(fine['expec'][:n]).any()
    assert dropped > 100 and unvouched == 9 and padded > 100


def test_the_specification_equals_the_float64_restatement():
    assert len(EXPECTED['head']) == len(fmc.HEAD_SHAPES) == 5
    for k, rec in enumerate(EXPECTED['head']):
        now = fmc.head_compare(k, rec['seed'])
        assert now['equal'] and rec['equal'], k                      # the list, the windows and the counters: EQUAL
        assert now['matches'] == rec['matches'] >= 4
        assert 0 < rec['expec_err'] < 1e-6 and 0 < rec['mkpts1_err'] < 1e-5          # statements about the fixture
        assert rec['spread'] > 0.1                                   # the expectations are no zeros
        assert now['expec_err'] <= 4 * rec['expec_err'] and now['mkpts1_err'] <= 4 * rec['mkpts1_err'], (k, now)


@pytest.mark.parametrize('W', fmo.WINDOWS)
def test_exact_cases(W):
    rng = np.random.default_rng(W)
    WW, G = W * W, fmo.grid(W)
    for C in (4, 64, 68):
        for at in (0, W - 1, WW // 2, WW - W, WW - 1, 1 + W):
            win0, win1 = fmc.one_hot_windows(W, C, at, rng)
            expec, has = fmo.head(win0, win1, W)
            ky, kx = divmod(at, W)
            floor = F32(np.sqrt(F32(1e-10))) + F32(np.sqrt(F32(1e-10)))
            # var = G2 - G * G: the rounded square minus the rounded product of the same factors, exactly 0
            assert has.all() and np.array_equal(bits(expec[0]), bits(np.array([G[kx], G[ky], floor], F32))), (C, at)
        # a uniform window: every position has the same product with the centre
        win0 = rng.standard_normal((3, WW, C)).astype(F32)
        win1 = np.repeat(rng.standard_normal((3, 1, C)).astype(F32), WW, 1)
        expec, has = fmo.head(win0, win1, W)
        # The heat is ONE float32 h = fl(1 / WW) at every position and G is symmetric, so the real sum h * sum(G) is
        # exactly 0; what the stated serial fmaf chain leaves is its WW roundings of a running sum below 1, each at
        # most 2^-25.  (Measured: 0 for W = 5 and for x at W = 3, -2^-26 for y at W = 3, below 2^-27 at W = 7.)
        assert has.all() and (np.abs(expec[:, :2]) <= WW * 2.0 ** -25).all() and (expec[:, 2] > 0.5).all()
        assert W != 3 or (expec[:, 0] == 0).all()                    # -h, +0, +h cancel within every window row
        # swapping ky / kx of window 1 swaps x / y
        win1 = rng.standard_normal((5, WW, C)).astype(F32)
        swapped = win1.reshape(5, W, W, C).transpose(0, 2, 1, 3).reshape(5, WW, C)
        a, _ = fmo.head(win0[:1].repeat(5, 0), win1, W)
        b, _ = fmo.head(win0[:1].repeat(5, 0), swapped, W)
        # The swap permutes the terms of the serial sums, so the bits may move: Z in another order moves every heat
        # by at most 2 * WW * 2^-24 relative (sum of heat * |G| <= 1), and each moment's own WW roundings of a
        # running sum below 1 add at most 2 * WW * 2^-25 between the two orders.
        swap_bound = 3 * WW * 2.0 ** -24
        assert np.abs(a[:, 0] - b[:, 1]).max() <= swap_bound and np.abs(a[:, 1] - b[:, 0]).max() <= swap_bound
        assert np.abs(a[:, 0] - a[:, 1]).max() > 100 * swap_bound    # x and y differ: the swap is seen
        # a window that is its own transpose: the same terms in the same order, the same bits
        sym = ((win1 + swapped) * F32(0.5)).astype(F32)
        c, _ = fmo.head(win0[:1].repeat(5, 0), sym, W)
        assert np.abs(c[:, 0] - c[:, 1]).max() <= swap_bound
    # no candidate: every correlation non-finite
    win0, win1 = fmc.one_hot_windows(W, 8, 0, rng)
    win1[0, :, 0] = np.nan
    expec, has = fmo.head(win0, win1, W)
    assert not has.any() and (expec[0, :2] == 0).all() and np.isnan(expec[0, 2])
    win1[0, 3, 0] = 0                                                # one candidate left: its grid point
    expec, has = fmo.head(win0, win1, W)
    assert has.all() and expec[0, 0] == G[3 % W] and expec[0, 1] == G[3 // W]


@pytest.mark.parametrize('W,stride,shift', [(5, 4, (1, -2)), (3, 2, (-1, 1)), (7, 4, (3, 2)), (5, 4, (0, 0))])
def test_a_planted_offset_is_recovered_within_one_fine_cell(W, stride, shift):
    s = fmc.planted_scene(W, stride, 32, shift, np.random.default_rng(5))
    win = fmo.windows_call(s['matches0'], s['off'], s['off'], s['grid'], s['grid'], s['K'], s['fine0'], s['foff'],
                           s['fgrid'], s['fine1'], s['foff'], s['fgrid'], W=W, stride=stride, max_matches=s['K'])
    fine = fmo.refine_call(win['win0'], win['win1'], win['rows'], win['moffsets'], win['counts'], s['kp'], s['off'],
                           s['kp'], s['off'], W=W, fine_cell=s['fine_cell'])
    assert win['counts'].tolist() == [[s['K'], s['K']]] and fine['counts'].tolist() == [[s['K'], s['K'], 0]]
    g, fg = s['grid'][0], s['fgrid'][0]
    row, col = np.divmod(np.arange(s['K']), g[1])
    ty, tx = row * stride + shift[0], col * stride + shift[1]
    seen = (ty >= 0) & (ty < fg[0]) & (tx >= 0) & (tx < fg[1])       # the displaced cell lies inside the map
    assert seen.sum() >= s['K'] // 2
    err = np.abs(fine['mkpts1'][:s['K']] - s['truth']).max(-1)
    assert (err[seen] < s['fine_cell']).all(), err[seen].max()
    coarse = np.abs(s['kp'] - s['truth']).max(-1)
    assert np.allclose(coarse, max(abs(shift[0]), abs(shift[1])) * s['fine_cell'])
    assert np.array_equal(fine['keypoints1'], fine['mkpts1'][:s['K']]) and np.array_equal(fine['mkpts0'][:s['K']], s['kp'])


def lane_walk_dot(a, b, lane_order, pairing):
    """One dot product as 16 lanes form it: lane ``l`` owns the float4 groups ``l, l + 16, ...`` in ascending order,
    the lanes run in ``lane_order``; then four shuffle levels in which every lane adds its partner (``pairing`` picks
    which operand comes first: float addition commutes)."""
    C = len(a)
    lane = np.zeros(16, F32)
    for l in lane_order:
        acc = F32(0)
        for g in range(l, C // 4, 16):
            for c in range(4 * g, 4 * g + 4):
                acc = fma32(a[c], b[c], acc)[()]
        lane[l] = acc
    d = 1
    while d < 16:
        nxt = lane.copy()
        for l in range(16):
            x, y = (lane[l], lane[l ^ d]) if pairing else (lane[l ^ d], lane[l])
            nxt[l] = F32(x + y)
        lane, d = nxt, d * 2
    assert (bits(lane) == bits(lane)[0]).all()                       # every lane ends with the same sum
    return lane[0]


def test_the_stated_dot_product_gives_the_same_bits_under_two_walks():
    rng = np.random.default_rng(31)
    differs = 0
    for C in (4, 8, 60, 64, 68, 128, 512):
        a, b = rng.standard_normal(C).astype(F32), rng.standard_normal(C).astype(F32)
        want = fmo.dot16(a, b[None])[0]
        assert bits(lane_walk_dot(a, b, range(16), True)) == bits(want), C
        assert bits(lane_walk_dot(a, b, range(15, -1, -1), False)) == bits(want), C
        chain = F32(0)
        for c in range(C):
            chain = fma32(a[c], b[c], chain)[()]
        differs += int(chain != want) + int(F32(a @ b) != want)
    assert differs >= 4                                              # the order is a statement: other orders differ
    assert fmo.partial_of(np.arange(128)).tolist() == [(c // 4) % 16 for c in range(128)]
    assert fmo.tree(np.arange(16, dtype=F32)) == 120


# ---------------------------------------------------------------------------------------- the header on the host
@pytest.fixture(scope='module')
def hostmath(tmp_path_factory):
    """``csrc/fine_match_math.h`` compiled for the host (tools/fine_match_hostmath.cpp)."""
    out = tmp_path_factory.mktemp('hostmath')
    subprocess.run(['make', '-C', str(CSRC), 'hostmath-fine_match', f'HOSTCHECK_BIN={out}'], check=True,
                   capture_output=True)
    lib = ctypes.CDLL(str(out / 'libfine_match_hostmath.so'))
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.fm_host_partials.restype = i
    lib.fm_host_scale.restype = lib.fm_host_radius.restype = ctypes.c_float
    lib.fm_host_scale.argtypes = [i]
    lib.fm_host_radius.argtypes = [i, ctypes.c_float]
    lib.fm_host_partial_of.restype = lib.fm_host_grid.restype = lib.fm_host_head.restype = None
    lib.fm_host_refined.restype = None
    lib.fm_host_partial_of.argtypes = [i, vp]
    lib.fm_host_grid.argtypes = [i, vp, vp]
    lib.fm_host_head.argtypes = [vp, vp, i, i, i, vp, vp, vp]
    lib.fm_host_refined.argtypes = [vp, vp, i, ctypes.c_float, vp]
    return lib


def host_head(lib, win0, win1, W):
    win0, win1 = np.ascontiguousarray(win0, F32), np.ascontiguousarray(win1, F32)
    M, WW, C = win1.shape
    s, expec, has = np.empty((M, WW), F32), np.empty((M, 3), F32), np.empty(M, np.int32)
    lib.fm_host_head(win0.ctypes.data, win1.ctypes.data, M, W, C, s.ctypes.data, expec.ctypes.data, has.ctypes.data)
    return s, expec, has.astype(bool)


def test_device_arithmetic_compiled_for_the_host_equals_the_specification(hostmath):
    assert hostmath.fm_host_partials() == fmo.PARTIALS == hip_engine.FINE_MATCH_PARTIALS
    part = np.empty(2048, np.int32)
    hostmath.fm_host_partial_of(2048, part.ctypes.data)
    assert np.array_equal(part, fmo.partial_of(np.arange(2048)))
    for W in fmo.WINDOWS:
        g, g2 = np.empty(W, F32), np.empty(W, F32)
        hostmath.fm_host_grid(W, g.ctypes.data, g2.ctypes.data)
        assert np.array_equal(bits(g), bits(fmo.grid(W))) and np.array_equal(bits(g2), bits(fmo.grid2(W)))
        for cell in (2.0, 1.0, 4.0, 2.6667, 0.1):
            assert bits(F32(hostmath.fm_host_radius(W, cell))) == bits(fmo.radius_of(W, cell))
    for C in range(4, 516, 4):
        assert bits(F32(hostmath.fm_host_scale(C))) == bits(fmo.scale_of(C)), C
    matches = 0
    rng = np.random.default_rng(77)
    for name in fmc.SHAPES:
        call = fmc.make_call(name)
        win = fmc.windows(call, fmc.matched_total(call))
        W, n = call['W'], int(win['moffsets'][-1])
        for spread in (1.0, 3.0):                                    # a flat and a peaked softmax
            w0, w1 = win['win0'][:n] * F32(spread), win['win1'][:n]
            s, expec, has = host_head(hostmath, w0, w1, W)
            assert np.array_equal(bits(s), bits(fmo.dot16(w0[:, W * W // 2], w1))), name
            want, want_has = fmo.head(w0, w1, W)
            assert np.array_equal(bits(expec), bits(want)) and np.array_equal(has, want_has), name
            matches += n
    # non-finite entries, a window with no candidate, a one-hot heat
    for W in fmo.WINDOWS:
        w0 = rng.standard_normal((6, W * W, 8)).astype(F32)
        w1 = rng.standard_normal((6, W * W, 8)).astype(F32)
        w1[0, 2, 3], w1[1, :, 0], w1[2, 4, 1], w1[3, 1, 2] = np.nan, np.nan, np.inf, -np.inf
        w0[4, W * W // 2, 5] = np.inf                                # the centre: every product non-finite
        w0[5], w1[5] = fmc.one_hot_windows(W, 8, W + 1, rng)
        s, expec, has = host_head(hostmath, w0, w1, W)
        want, want_has = fmo.head(w0, w1, W)
        assert np.array_equal(bits(expec), bits(want)) and np.array_equal(has, want_has)
        assert want_has.tolist() == [True, False, True, True, False, True] and np.isnan(want[[1, 4], 2]).all()
    kp = (rng.random(1000) * 640).astype(F32)
    v = (rng.random(1000) * 2 - 1).astype(F32)
    out = np.empty(1000, F32)
    for radius in (4.0, 2.0, 6.0, 0.3):
        hostmath.fm_host_refined(kp.ctypes.data, v.ctypes.data, 1000, radius, out.ctypes.data)
        assert np.array_equal(bits(out), bits((kp + (v * F32(radius)).astype(F32)).astype(F32)))
    assert matches > 300


# ---------------------------------------------------------------------------------------- the ABI
def header_text(name):
    return re.sub(r'/\*.*?\*/', '', (REPO / 'include' / name).read_text(), flags=re.S)


def header_functions(name):
    return sorted(set(re.findall(r'\b(oetr_[a-z_0-9]+)\s*\(', header_text(name))))


def parameter_count(name, fn):
    args = re.search(r'\b' + fn + r'\s*\(([^)]*)\)', header_text(name)).group(1).strip()
    return 0 if args == 'void' else len(args.split(','))


def test_header_exports_library_and_versions_agree():
    lib = pkg.load_library()
    names = header_functions(HEADER)
    assert len(names) == 4 and set(names) == set(hip_engine.FINE_MATCH_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/{HEADER} but not exported'
    assert lib.oetr_fine_match_abi_version() == hip_engine.FINE_MATCH_ABI_VERSION == 1
    text = (REPO / 'include' / HEADER).read_text()
    for macro, value in (('ABI_VERSION', 1), ('WINDOW_COUNTERS', hip_engine.FINE_MATCH_WINDOW_COUNTERS),
                         ('COUNTERS', hip_engine.FINE_MATCH_COUNTERS), ('PARTIALS', hip_engine.FINE_MATCH_PARTIALS),
                         ('MIN_C', hip_engine.FINE_MATCH_MIN_C), ('MAX_C', hip_engine.FINE_MATCH_MAX_C),
                         ('MAX_STRIDE', hip_engine.FINE_MATCH_MAX_STRIDE), ('MAX_W', max(hip_engine.FINE_MATCH_WINDOWS))):
        assert re.search(r'#define\s+OETR_FINE_MATCH_%s\s+%d\b' % (macro, value), text), macro
    assert (hip_engine.FINE_MATCH_WINDOW_COUNTERS, hip_engine.FINE_MATCH_COUNTERS, hip_engine.FINE_MATCH_PARTIALS) \
        == (fmo.WINDOW_COUNTERS, fmo.COUNTERS, fmo.PARTIALS) == (2, 3, 16)
    assert hip_engine.FINE_MATCH_WINDOWS == fmo.WINDOWS == (3, 5, 7)
    for W in fmo.WINDOWS:                                            # the header's tables are the specification's G
        table = re.search(r'#define\s+OETR_FINE_MATCH_G%d\s+\{([^}]*)\}' % W, text).group(1).replace('\\', '')
        assert [F32(v.strip().rstrip('f')) for v in table.split(',')] == fmo.grid(W).tolist()
    math = (CSRC / 'fine_match_math.h').read_text()
    assert '#include "dual_softmax_math.h"' in math and 'ds::e(' in math and 'E_LOG2E' not in math   # included, not restated
    # the other headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(hip_engine.EXPORTS) == 53
    assert len(header_functions('oetr_nn_match.h')) == 3 and len(header_functions('oetr_keypoint_select.h')) == 3
    assert len(header_functions('oetr_dual_softmax.h')) == 3 and len(header_functions('oetr_match_assembly.h')) == 3
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.COVIS_SET_EXPORTS) | set(hip_engine.CROP_BATCH_EXPORTS)
              | set(hip_engine.MATCH_SCORE_EXPORTS) | set(hip_engine.KEYPOINT_SCORE_EXPORTS)
              | set(hip_engine.MATCH_ASSEMBLY_EXPORTS) | set(hip_engine.HOMOGRAPHY_EXPORTS)
              | set(hip_engine.POSE_RANSAC_EXPORTS) | set(hip_engine.NN_MATCH_EXPORTS)
              | set(hip_engine.HOMOGRAPHY_RANSAC_EXPORTS) | set(hip_engine.POSE_REFIT_EXPORTS)
              | set(hip_engine.KEYPOINT_SELECT_EXPORTS) | set(hip_engine.DUAL_SOFTMAX_EXPORTS))
    assert not set(hip_engine.FINE_MATCH_EXPORTS) & others
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_nn_match_abi_version() == hip_engine.NN_MATCH_ABI_VERSION == 1
    assert lib.oetr_keypoint_select_abi_version() == hip_engine.KEYPOINT_SELECT_ABI_VERSION == 1
    assert lib.oetr_dual_softmax_abi_version() == hip_engine.DUAL_SOFTMAX_ABI_VERSION == 1
    assert lib.oetr_match_assembly_abi_version() == hip_engine.MATCH_ASSEMBLY_ABI_VERSION == 1
    for name in ('fine_windows', 'refine_matches', 'fine_match_counts'):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_argument_types_are_declared():
    lib = pkg.load_library()
    for fn in hip_engine.FINE_MATCH_EXPORTS:
        f = getattr(lib, fn)
        assert f.argtypes is not None and len(f.argtypes) == parameter_count(HEADER, fn), fn
    assert lib.oetr_fine_windows.restype is ctypes.c_int and lib.oetr_fine_refine.restype is ctypes.c_int
    assert lib.oetr_fine_match_workspace_bytes.restype is ctypes.c_size_t
    at = lib.oetr_fine_windows.argtypes
    i64, ints = (5, 6, 12, 16, 20), (7, 8, 17, 18, 19)
    assert len(at) == 29 and all(at[k] is ctypes.c_int64 for k in i64) and all(at[k] is ctypes.c_int for k in ints)
    assert at[22] is ctypes.c_size_t
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in i64 + ints + (22,))
    at = lib.oetr_fine_refine.argtypes
    assert len(at) == 22 and all(at[k] is ctypes.c_int64 for k in (6, 9, 12)) and all(at[k] is ctypes.c_int for k in (5, 13, 14))
    assert at[15] is ctypes.c_float
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (5, 6, 9, 12, 13, 14, 15))
    ws = lib.oetr_fine_match_workspace_bytes
    assert ws(0) == ws(-3) == 0 and ws(1) >= 4 and ws(1000) >= 4000 and ws(300) % 256 == 0


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(b'\xa5' * 80, 80)   # host memory standing in for the device: never touched
    p = (ctypes.addressof(keep) + 15) // 16 * 16           # 16-byte aligned, 64 bytes behind it

    def windows(matches0=p, off0=p, off1=p, grids0=p, grids1=p, n0=5, n1=4, n=2, max_k0=3, fine0=p, foff0=p, fgrids0=p,
                f0=80, fine1=p, foff1=p, fgrids1=p, f1=64, C=128, W=5, stride=4, cap=6, ws=p, ws_bytes=1 << 20, rows=p,
                moffsets=p, counts=p, win0=p, win1=p):
        return lib.oetr_fine_windows(matches0, off0, off1, grids0, grids1, n0, n1, n, max_k0, fine0, foff0, fgrids0, f0,
                                     fine1, foff1, fgrids1, f1, C, W, stride, cap, ws, ws_bytes, rows, moffsets, counts,
                                     win0, win1, None)

    def refine(win0=p, win1=p, rows=p, moffsets=p, wcounts=p, n=2, cap=6, kp0=p, off0=p, n0=5, kp1=p, off1=p, n1=4,
               C=128, W=5, cell=2.0, expec=p, mkpts0=p, mkpts1=p, kp1f=p, counts=p):
        return lib.oetr_fine_refine(win0, win1, rows, moffsets, wcounts, n, cap, kp0, off0, n0, kp1, off1, n1, C, W, cell,
                                    expec, mkpts0, mkpts1, kp1f, counts, None)

    bad = [{k: None} for k in ('matches0', 'off0', 'off1', 'grids0', 'grids1', 'fine0', 'foff0', 'fgrids0', 'fine1', 'foff1',
                               'fgrids1', 'ws', 'rows', 'moffsets', 'counts', 'win0', 'win1')]
    bad += [dict(n=0), dict(n=-2), dict(n0=-1), dict(n1=-(1 << 63)), dict(f0=-1), dict(f1=-7), dict(max_k0=-1),
            dict(cap=-1), dict(W=0), dict(W=1), dict(W=4), dict(W=6), dict(W=9), dict(W=-5), dict(stride=0),
            dict(stride=9), dict(stride=-4), dict(C=0), dict(C=2), dict(C=-4), dict(C=130), dict(C=516), dict(C=1024),
            dict(fine0=p + 4), dict(fine1=p + 8), dict(win0=p + 8), dict(win1=p + 4), dict(matches0=p + 2),
            dict(off0=p + 1), dict(fgrids1=p + 2), dict(ws=p + 2), dict(rows=p + 2), dict(moffsets=p + 1),
            dict(counts=p + 2)]
    for kw in bad:
        assert windows(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_fine_windows'), kw
    for kw in (dict(n0=1 << 31), dict(n1=(1 << 63) - 1), dict(f0=1 << 31), dict(f1=1 << 40), dict(n=(1 << 31) - 1),
               dict(cap=(2 ** 31 - 1) // 25 + 1), dict(W=3, cap=(2 ** 31 - 1) // 9 + 1), dict(W=7, cap=(2 ** 31 - 1) // 49 + 1),
               dict(cap=(1 << 63) - 1)):
        assert windows(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_fine_windows'), kw
    need = lib.oetr_fine_match_workspace_bytes(100000)
    for kw in (dict(ws_bytes=0), dict(ws_bytes=7), dict(n=100000, ws_bytes=need - 1)):
        assert windows(**kw) == WORKSPACE, kw
        assert lib.oetr_last_error().startswith(b'oetr_fine_windows'), kw
    bad = [{k: None} for k in ('win0', 'win1', 'rows', 'moffsets', 'wcounts', 'kp0', 'off0', 'kp1', 'off1', 'expec',
                               'mkpts0', 'mkpts1', 'kp1f', 'counts')]
    bad += [dict(n=0), dict(n=-1), dict(n0=-1), dict(n1=-1), dict(cap=-1), dict(W=4), dict(W=0), dict(W=11), dict(C=0),
            dict(C=6), dict(C=520), dict(cell=0.0), dict(cell=-2.0), dict(cell=float('inf')), dict(cell=float('nan')),
            dict(win0=p + 8), dict(win1=p + 4), dict(kp0=p + 4), dict(kp1=p + 4), dict(kp1f=p + 4), dict(mkpts0=p + 4),
            dict(mkpts1=p + 4), dict(expec=p + 2), dict(rows=p + 1), dict(moffsets=p + 2), dict(wcounts=p + 2),
            dict(counts=p + 2), dict(off1=p + 1)]
    for kw in bad:
        assert refine(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_fine_refine'), kw
    for kw in (dict(n0=1 << 31), dict(n1=(1 << 63) - 1), dict(n=(1 << 31) - 1), dict(cap=(2 ** 31 - 1) // 25 + 1),
               dict(W=7, cap=(2 ** 31 - 1) // 49 + 1)):
        assert refine(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_fine_refine'), kw
    assert keep.raw == b'\xa5' * 80


def test_the_wrappers_refuse_before_any_device_use(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    off, grid = np.array([0, 4], np.int32), np.array([[2, 2]], np.int32)
    coarse = dict(matches0=np.array([0, 1, -1, 3], np.int32), keypoints0=dso.keypoints(2, 2, 8),
                  keypoints1=dso.keypoints(2, 2, 8), _inputs=(None, None, off, off, grid, grid))
    f32 = np.zeros((64, 8), np.float32)
    foff, fgrid = np.array([0, 64], np.int32), np.array([[8, 8]], np.int32)
    joined = dict(fine_offsets0=foff, fine_offsets1=foff, fine_grids0=fgrid, fine_grids1=fgrid, max_matches=4)
    for f0, f1 in ((f32.astype(np.float64), f32), (f32, torch.zeros(64, 8, dtype=torch.float64))):
        with pytest.raises(ValueError, match='float64'):
            pkg.fine_windows(coarse, f0, f1, **joined)
    with pytest.raises(ValueError, match='float64'):
        pkg.fine_windows(coarse, [np.zeros((8, 8, 8))], [np.zeros((8, 8, 8), np.float32)], max_matches=4)
    for missing in ('fine_offsets0', 'fine_offsets1', 'fine_grids0', 'fine_grids1', 'max_matches'):
        with pytest.raises(ValueError, match=missing):
            pkg.fine_windows(coarse, f32, f32, **{k: v for k, v in joined.items() if k != missing})
    with pytest.raises(ValueError, match='fine_offsets'):
        pkg.fine_windows(coarse, [f32.reshape(8, 8, 8)], [f32.reshape(8, 8, 8)], fine_offsets0=foff, max_matches=4)
    with pytest.raises(ValueError, match='one map per pair'):
        pkg.fine_windows(coarse, [f32.reshape(8, 8, 8)], [], max_matches=4)
    with pytest.raises(ValueError, match='offsets0'):
        pkg.fine_windows(dict(matches0=coarse['matches0']), f32, f32, **joined)
    with pytest.raises(ValueError, match='match_dense result'):
        pkg.fine_windows([1, 2], f32, f32, **joined)
    for kw, what in ((dict(window=4), 'window'), (dict(window=9), 'window'), (dict(stride=0), 'stride'),
                     (dict(stride=9), 'stride'), (dict(stride=1.5), 'stride'), (dict(max_matches=-1), 'max_matches'),
                     (dict(max_matches=2.5), 'max_matches'), (dict(max_matches=2 ** 31), 'max_matches')):
        with pytest.raises(ValueError, match=what):
            pkg.fine_windows(coarse, f32, f32, **{**joined, **kw})
    with pytest.raises(RuntimeError, match='GPU.*no CPU implementation'):
        pkg.fine_windows(coarse, f32, f32, **joined)
    with pytest.raises(RuntimeError, match='GPU.*no CPU implementation'):
        pkg.fine_windows(coarse, [torch.zeros(8, 8, 8)], [torch.zeros(7, 8, 8)], max_matches=4)
    windows = dict(rows=torch.zeros(4, 3, dtype=torch.int32), moffsets=torch.zeros(2, dtype=torch.int32), window=5,
                   win0=torch.zeros(4, 25, 8), win1=torch.zeros(4, 25, 8))
    for kw in (dict(fine_cell=0), dict(fine_cell=-2.0), dict(fine_cell=float('nan')), dict(fine_cell=float('inf'))):
        with pytest.raises(ValueError, match='fine_cell'):
            pkg.refine_matches(windows, coarse, **kw)
    with pytest.raises(ValueError, match='fine_windows result'):
        pkg.refine_matches(dict(win0=0), coarse)
    with pytest.raises(ValueError, match='match_dense result'):
        pkg.refine_matches(windows, dict(matches0=0))
    with pytest.raises(ValueError, match='float64'):
        pkg.refine_matches(windows, coarse, win0=torch.zeros(4, 25, 8, dtype=torch.float64))
    # host inputs inside a capture: refused by name before anything is uploaded
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: __import__('contextlib').nullcontext())
    with pytest.raises(ValueError, match=r"inside a graph capture.*'matches0'.*'offsets0'.*'fine_grids1'.*'fine0'"):
        pkg.fine_windows(coarse, f32, f32, **joined)
    from imagematching_oetr_amd.dloc_matcher import CoarseToFine, DualSoftmax
    assert CoarseToFine.required_inputs == ['image0', 'image1']
    assert CoarseToFine.default_conf == {**DualSoftmax.default_conf, 'window': 5, 'stride': 4, 'max_matches': None}
    assert CoarseToFine({'window': 7}).conf['window'] == 7
    with pytest.raises(ValueError, match='net'):
        CoarseToFine({})({'image0': torch.zeros(1), 'image1': torch.zeros(1)})
