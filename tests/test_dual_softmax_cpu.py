"""CPU-only checks of the dual-softmax matcher extension (``include/oetr_dual_softmax.h``, ``csrc/dual_softmax.hip``,
``csrc/dual_softmax_math.h``, ``imagematching_oetr_amd/dense_match.py``) and of its specification
``tests/dual_softmax_oracle.py``.

The specification: its exponential against float64 ``np.exp`` inside and beyond the cut-off, gated at four times the
recorded error; its stated sums under two emulated walks; the pinned calls regenerate the recorded results; it equals a
plain float64 restatement of the published head on the drawn calls - ``matches0`` and the counters on EVERY row, the
confidences within four times the recorded error; swapping the sides gives the inverse mapping.

The arithmetic: ``dual_softmax_math.h`` compiled for the host, with the kernels' walk restated serially, equals the numpy
program bit for bit - ``e``, every statistic, every confidence, every decision.

The ABI: header, export list and library agree and the other lists stand as they were; argument types are declared;
every host-checked argument error is reported without a GPU and touches nothing; the wrapper refuses before any device
use.  (The host code under ASan + UBSan is a stand-alone program: ``make hostcheck-dual_softmax``.)"""
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
import dual_softmax_cases as dsc  # noqa: E402
import dual_softmax_oracle as dso  # noqa: E402
import nn_match_oracle as nmo  # noqa: E402

HEADER = 'oetr_dual_softmax.h'
BAD_ARG, BAD_SHAPE, WORKSPACE = 1, 2, 4
EXPECTED = json.loads((REPO / 'tests' / 'dual_softmax_expected.json').read_text())
F32 = np.float32
CSRC = REPO / 'imagematching_oetr_amd' / 'csrc'


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------- the specification
def test_e_against_float64_exp_inside_and_beyond_the_cut_off():
    inside, beyond = dsc.e_sweep()
    assert len(inside) > 2_000_000 and inside.min() == dso.E_CUT == F32(-87) and inside.max() == 0
    err = dsc.e_error(inside)
    recorded = EXPECTED['e_max_rel_err']
    assert 0 < recorded < 2.0 ** -22                                 # about an ulp: a statement about the fixture
    assert err <= 4 * recorded, (err, recorded)
    e = dso.e32(inside)
    assert e.dtype == F32 and (e >= np.finfo(F32).tiny).all() and (e <= 1).all()     # never subnormal, never above 1
    assert dso.e32(F32(0)) == 1 and dso.e32(F32(-0.0)) == 1 and bits(dso.e32(F32(0))) == bits(F32(1))
    assert (np.diff(dso.e32(np.sort(inside[::97]))) >= 0).all()      # monotone on a subsample
    assert len(beyond) > 20_000 and (bits(dso.e32(beyond)) == 0).all()               # exactly +0 below the cut-off
    assert dso.e32(np.nextafter(F32(-87), F32(-np.inf))) == 0 and dso.e32(F32(-87)) > 0
    assert EXPECTED['e_cut'] == -87.0 and EXPECTED['partials'] == dso.PARTIALS == 8 and dso.Q_MIN == F32(2.0 ** -62)


def kernel_walk_sum(terms, lane_order, register_order):
    """A row's sum as the kernel's lanes form it: tiles of 128 columns in ascending order; within a tile the four
    (key wave, lane half) owners in ``lane_order``, each walking its sixteen registers of either accumulator in
    ``register_order`` (ascending within an accumulator); then the two accumulators, the two lane halves, the two
    key waves."""
    K = len(terms)
    z = np.zeros((2, 2, 2), F32)
    for k0 in range(0, K, 128):
        for kh, h in lane_order:
            for g, a in register_order:
                j = k0 + kh * 64 + a * 32 + 4 * h + (g & 3) + 8 * (g >> 2)
                if j < K:
                    z[kh, h, a] = z[kh, h, a] + terms[j]
    halves = [F32(F32(z[kh, 0, 0] + z[kh, 0, 1]) + F32(z[kh, 1, 0] + z[kh, 1, 1])) for kh in range(2)]
    return F32(halves[0] + halves[1])


def test_the_stated_sums_give_the_same_bits_under_two_walks():
    rng = np.random.default_rng(23)
    a_inner = [(g, a) for g in range(16) for a in range(2)]          # the kernel: both accumulators per register
    a_outer = [(g, a) for a in range(2) for g in range(16)]          # one accumulator after the other
    lanes = [(kh, h) for kh in range(2) for h in range(2)]
    differs = 0
    for K in (0, 1, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300, 1000):
        terms = dso.e32(-rng.exponential(3.0, K).astype(F32))
        want = dso.ordered_sum(terms)
        assert kernel_walk_sum(terms, lanes, a_inner) == want, K
        assert kernel_walk_sum(terms, lanes[::-1], a_outer) == want, K
        assert dso.ordered_sum(np.stack([terms, terms[::-1]]))[0] == want
        differs += int(terms.sum(dtype=F32) != want) + int(F32(np.cumsum(terms, dtype=F32)[-1] if K else 0) != want)
        slots = dso.slot(np.arange(K))
        for s in range(dso.PARTIALS):                                # a partial's columns: fixed by position alone
            mine = np.nonzero(slots == s)[0]
            assert ((mine >> 6) & 1).tolist() == [s >> 2] * len(mine) and ((mine >> 2) & 1).tolist() == [(s >> 1) & 1] * len(mine)
    assert differs >= 4                                              # the order is a statement: other orders differ
    assert dso.tree(np.arange(8, dtype=F32)) == 28 and dso.slot(np.arange(256)).tolist() == dso.slot(np.arange(256) % 128).tolist()
    assert sorted(set(dso.slot(np.arange(128)).tolist())) == list(range(8))
    assert np.bincount(dso.slot(np.arange(128))).tolist() == [16] * 8


def test_pinned_calls_are_the_recorded_ones():
    assert EXPECTED['settings'] == [dsc.setting_key(*s) for s in dsc.SETTINGS] and len(dsc.SETTINGS) == 4
    assert sorted(EXPECTED['calls']) == sorted(f'{n}/{k}' for n, k in dsc.CALLS)
    counts_seen = {q for n in dsc.SHAPES for pair in dsc.SHAPES[n][1] for q in pair}
    assert {0, 1, 63, 64, 65, 127, 128, 129, 300} <= counts_seen
    assert {dsc.SHAPES[n][0] for n in dsc.SHAPES} == {4, 64, 68, 256, 512}
    assert {dsc.GRID_OF[k] for k in (1, 9, 20, 25, 300)} == {(1, 1), (3, 3), (4, 5), (5, 5), (15, 20)}
    assert all(h * w == k for k, (h, w) in dsc.GRID_OF.items())
    matched = unmatched = unmutual = 0
    for name, kind in dsc.CALLS:
        call, rec = dsc.make_call(name, kind), EXPECTED['calls'][f'{name}/{kind}']
        assert rec['D'] == call['D'] and rec['pairs'] == [list(q) for q in call['pairs']]
        assert rec['inputs_sha256'] == dict(feat0=dsc.sha(call['feat0']), feat1=dsc.sha(call['feat1']))
        if kind == 'grid':
            exact = [(a.astype(np.float64) @ b.astype(np.float64).T) for a, b in
                     ((call['feat0'][call['off0'][p]:call['off0'][p + 1]], call['feat1'][call['off1'][p]:call['off1'][p + 1]])
                      for p in range(len(call['pairs'])))]
            assert all(np.array_equal(e, s) for e, s in zip(exact, call['sims']))         # any order: the same similarity
        for setting in dsc.SETTINGS:
            res = dsc.expected(call, *setting)
            assert dsc.result_record(res) == rec['results'][dsc.setting_key(*setting)], (name, kind, setting)
            c = res['counts']
            matched += int(c[:, 3].sum())
            unmatched += int((c[:, 2] < c[:, 0]).sum())
            unmutual += int((c[:, 3] < c[:, 2]).sum())
            assert ((res['matching_scores0'] > 0).sum() >= (res['matches0'] > -1).sum())
            assert not np.isnan(res['keypoints0']).any() and (res['keypoints0'] % dsc.CELL == 0).all()
    assert matched > 1000 and unmatched and unmutual


def test_the_specification_equals_the_float64_head_on_every_row():
    assert EXPECTED['head_margin'] == dsc.HEAD_MARGIN == 1e-3 and len(EXPECTED['head']) == len(dsc.HEAD_SHAPES) == 6
    matched = 0
    for k, rec in enumerate(EXPECTED['head']):
        assert tuple(rec['shape']) == dsc.HEAD_SHAPES[k]
        now = dsc.head_compare(k, rec['seed'])
        assert now['margin'] == rec['margin'] >= dsc.HEAD_MARGIN, (k, now)            # the float64 program's own margins
        assert now['equal'] and rec['equal'], k                                       # matches0 and counters, no row left out
        assert now['matched'] == rec['matched']
        assert 0 < rec['conf_rel_err'] < 1e-4 and 0 < rec['conf_abs_err'] < 1e-5      # statements about the fixture
        assert now['conf_rel_err'] <= 4 * rec['conf_rel_err'] and now['conf_abs_err'] <= 4 * rec['conf_abs_err'], (k, now)
        matched += rec['matched']
    assert matched > 100
    assert {s[3] for s in dsc.HEAD_SHAPES} == {0.1, 1.0} and {s[4] for s in dsc.HEAD_SHAPES} == {0.0, 0.2}


def test_swapped_sides_give_the_inverse_mapping():
    for name, kind, setting in (('ragged64', 'grid', (0.1, 0.0, 0)), ('ragged64', 'gauss', (0.1, 0.2, 1)),
                                ('d512', 'gauss', (1.0, 0.0, 0))):
        call = dsc.make_call(name, kind)
        for p, tt in enumerate(dsc.ts_of(call, setting[0])):
            g0, g1 = tuple(call['grids0'][p]), tuple(call['grids1'][p])
            fwd = dso.match_t(tt, g0, g1, *setting[1:])
            back = dso.match_t(np.ascontiguousarray(tt.T), g1, g0, *setting[1:])
            m, inv = fwd['matches0'], back['matches0']
            assert fwd['counts'][3] == back['counts'][3] == (m > -1).sum() == (inv > -1).sum()
            rows = np.nonzero(m > -1)[0]
            assert np.array_equal(inv[m[rows]], rows)
            cols = np.nonzero(inv > -1)[0]
            assert np.array_equal(m[inv[cols]], cols)
            conf, _ = dso.confidence(tt)                             # the product commutes: the transpose, bit for bit
            assert np.array_equal(bits(dso.confidence(np.ascontiguousarray(tt.T))[0]), bits(conf.T))


# ---------------------------------------------------------------------------------------- the header on the host
@pytest.fixture(scope='module')
def hostmath(tmp_path_factory):
    """``csrc/dual_softmax_math.h`` compiled for the host (tools/dual_softmax_hostmath.cpp)."""
    out = tmp_path_factory.mktemp('hostmath')
    subprocess.run(['make', '-C', str(CSRC), 'hostmath-dual_softmax', f'HOSTCHECK_BIN={out}'], check=True,
                   capture_output=True)
    lib = ctypes.CDLL(str(out / 'libdual_softmax_hostmath.so'))
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.ds_host_partials.restype = i
    lib.ds_host_e.restype = lib.ds_host_slots.restype = lib.ds_host_pair.restype = None
    lib.ds_host_e.argtypes = [vp, ctypes.c_int64, vp]
    lib.ds_host_slots.argtypes = [i, vp]
    lib.ds_host_pair.argtypes = [vp, i, i, i, vp, i, i, i, i, ctypes.c_float, ctypes.c_float, i] + [vp] * 9
    return lib


def host_pair(lib, A, B, g0, g1, scale, threshold, border):
    A, B = np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)
    L, S = len(A), len(B)
    out = dict(m=np.empty(L, F32), Z=np.empty(L, F32), c=np.empty(S, F32), Y=np.empty(S, F32),
               conf=np.empty((L, S), F32), matches0=np.empty(L, np.int32), matching_scores0=np.empty(L, F32),
               matches1=np.empty(S, np.int32), counts=np.empty(4, np.int32))
    lib.ds_host_pair(A.ctypes.data, L, int(g0[0]), int(g0[1]), B.ctypes.data, S, int(g1[0]), int(g1[1]), A.shape[1],
                     float(scale), float(F32(threshold)), border, *[a.ctypes.data for a in out.values()])
    return out


def test_device_arithmetic_compiled_for_the_host_equals_the_specification(hostmath):
    assert hostmath.ds_host_partials() == dso.PARTIALS == hip_engine.DUAL_SOFTMAX_PARTIALS
    inside, beyond = dsc.e_sweep()
    x = np.concatenate([inside, beyond])
    got = np.empty_like(x)
    hostmath.ds_host_e(x.ctypes.data, len(x), got.ctypes.data)
    assert np.array_equal(bits(got), bits(dso.e32(x)))
    slots = np.empty(1000, np.int32)
    hostmath.ds_host_slots(1000, slots.ctypes.data)
    assert np.array_equal(slots, dso.slot(np.arange(1000)))
    pairs = elements = 0
    cases = [(name, kind, setting) for name, kind, setting in
             (('ragged64', 'gauss', (0.1, 0.2, 1)), ('ragged64', 'grid', (0.1, 0.0, 0)), ('borders', 'grid', (1.0, 0.0, 1)),
              ('d4', 'gauss', (0.1, 0.0, 0)), ('d68', 'grid', (1.0, 0.2, 0)), ('d512', 'gauss', (0.1, 0.2, 2)))]
    special = []
    A, B, g0, g1 = dsc.cutoff_pair()
    special.append((A, B, g0, g1, 0.1, 0.2, 0))
    A, B, g0, g1 = dsc.all_equal_call()
    special.append((A, B, g0, g1, 0.1, 0.0, 0))
    A, B = dsc.gauss_pair(np.random.default_rng(8), 33, 65, 8)
    A[3, 2], B[7, :] = np.nan, np.inf
    special.append((A, B, dsc.GRID_OF[33], dsc.GRID_OF[65], 1.0, 0.0, 0))
    for name, kind, (temperature, threshold, border) in cases:
        call = dsc.make_call(name, kind)
        for p in range(len(call['pairs'])):
            A = call['feat0'][call['off0'][p]:call['off0'][p + 1]]
            B = call['feat1'][call['off1'][p]:call['off1'][p + 1]]
            special.append((A, B, tuple(call['grids0'][p]), tuple(call['grids1'][p]), temperature, threshold, border))
    for A, B, g0, g1, temperature, threshold, border in special:
        scale = dso.scale_of(A.shape[1], temperature)
        tt = (nmo.similarity(A, B) * scale).astype(F32)
        want = dso.match_t(tt, g0, g1, threshold, border)
        (m, Z), (c, Y) = dso.statistics(tt), dso.statistics(tt.T)
        conf, _ = dso.confidence(tt)
        got = host_pair(hostmath, A, B, g0, g1, scale, threshold, border)
        tag = (A.shape, B.shape, temperature, threshold, border)
        for key, w in (('m', m), ('Z', Z), ('c', c), ('Y', Y), ('conf', conf), ('matching_scores0', want['matching_scores0'])):
            assert np.array_equal(bits(got[key]), bits(w)), (tag, key)
        for key in ('matches0', 'matches1', 'counts'):
            assert np.array_equal(got[key], want[key]), (tag, key)
        pairs += 1
        elements += conf.size
    assert pairs > 30 and elements > 300_000


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
    assert len(names) == 3 and set(names) == set(hip_engine.DUAL_SOFTMAX_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/{HEADER} but not exported'
    assert lib.oetr_dual_softmax_abi_version() == hip_engine.DUAL_SOFTMAX_ABI_VERSION == 1
    text = (REPO / 'include' / HEADER).read_text()
    for macro, value in (('ABI_VERSION', 1), ('COUNTERS', hip_engine.DUAL_SOFTMAX_COUNTERS),
                         ('PARTIALS', hip_engine.DUAL_SOFTMAX_PARTIALS), ('MIN_D', hip_engine.DUAL_SOFTMAX_MIN_D),
                         ('MAX_D', hip_engine.DUAL_SOFTMAX_MAX_D)):
        assert re.search(r'#define\s+OETR_DUAL_SOFTMAX_%s\s+%d\b' % (macro, value), text), macro
    assert (hip_engine.DUAL_SOFTMAX_COUNTERS, hip_engine.DUAL_SOFTMAX_PARTIALS) == (dso.COUNTERS, dso.PARTIALS) == (4, 8)
    math = (CSRC / 'dual_softmax_math.h').read_text()
    assert 'E_CUT = -87.0f' in math and 'Q_MIN = 0x1p-62f' in math and 'PARTIALS = 8' in math
    # the other headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(hip_engine.EXPORTS) == 53
    assert len(header_functions('oetr_nn_match.h')) == 3 and len(header_functions('oetr_keypoint_select.h')) == 3
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.COVIS_SET_EXPORTS) | set(hip_engine.CROP_BATCH_EXPORTS)
              | set(hip_engine.MATCH_SCORE_EXPORTS) | set(hip_engine.KEYPOINT_SCORE_EXPORTS)
              | set(hip_engine.MATCH_ASSEMBLY_EXPORTS) | set(hip_engine.HOMOGRAPHY_EXPORTS)
              | set(hip_engine.POSE_RANSAC_EXPORTS) | set(hip_engine.NN_MATCH_EXPORTS)
              | set(hip_engine.HOMOGRAPHY_RANSAC_EXPORTS) | set(hip_engine.POSE_REFIT_EXPORTS)
              | set(hip_engine.KEYPOINT_SELECT_EXPORTS))
    assert not set(hip_engine.DUAL_SOFTMAX_EXPORTS) & others
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_nn_match_abi_version() == hip_engine.NN_MATCH_ABI_VERSION == 1
    assert lib.oetr_keypoint_select_abi_version() == hip_engine.KEYPOINT_SELECT_ABI_VERSION == 1
    for name in ('match_dense', 'dense_match_counts'):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_argument_types_are_declared():
    lib = pkg.load_library()
    for fn in hip_engine.DUAL_SOFTMAX_EXPORTS:
        f = getattr(lib, fn)
        assert f.argtypes is not None and len(f.argtypes) == parameter_count(HEADER, fn), fn
    assert lib.oetr_dual_softmax_match.restype is ctypes.c_int
    assert lib.oetr_dual_softmax_workspace_bytes.restype is ctypes.c_size_t
    at = lib.oetr_dual_softmax_match.argtypes
    assert len(at) == 25 and at[3] is at[7] is ctypes.c_int64 and at[17] is ctypes.c_size_t
    assert all(at[k] is ctypes.c_int for k in (8, 9, 10, 11, 14, 15)) and at[12] is at[13] is ctypes.c_float
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (3, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17))
    ws = lib.oetr_dual_softmax_workspace_bytes
    assert ws(0, 0) == ws(-3, -1) == 0 and ws(1, 0) >= 8 and ws(0, 1) >= 12 and ws(1000, 1000) >= 20 * 1000
    assert ws(2 ** 31 - 1, 2 ** 31 - 1) >= 20 * (2 ** 31 - 1) and ws(300, 300) % 256 == 0


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(b'\xa5' * 80, 80)   # host memory standing in for the device: never touched
    p = (ctypes.addressof(keep) + 15) // 16 * 16           # 16-byte aligned, 64 bytes behind it

    def call(feat0=p, off0=p, grids0=p, n0=5, feat1=p, off1=p, grids1=p, n1=4, n=2, D=128, max_k0=3, max_k1=2,
             scale=0.078125, thr=0.2, border=2, cell=8, ws=p, ws_bytes=1 << 20, matches0=p, scores0=p, matches1=p, kp0=p,
             kp1=p, counts=p):
        return lib.oetr_dual_softmax_match(feat0, off0, grids0, n0, feat1, off1, grids1, n1, n, D, max_k0, max_k1, scale,
                                           thr, border, cell, ws, ws_bytes, matches0, scores0, matches1, kp0, kp1, counts,
                                           None)

    bad = [{k: None} for k in ('feat0', 'off0', 'grids0', 'feat1', 'off1', 'grids1', 'matches0', 'scores0', 'kp0', 'kp1',
                               'counts', 'ws')]
    bad += [dict(counts=None, n0=0, n1=0), dict(n=0), dict(n=-2), dict(n0=-1), dict(n1=-(1 << 63)), dict(max_k0=-1),
            dict(max_k1=-5), dict(D=0), dict(D=2), dict(D=-4), dict(D=130), dict(D=516), dict(D=1024), dict(scale=0.0),
            dict(scale=-1.0), dict(scale=float('inf')), dict(scale=float('nan')), dict(thr=-1e-9), dict(thr=float('nan')),
            dict(thr=float('inf')), dict(border=-1), dict(cell=0), dict(cell=-8), dict(feat0=p + 4), dict(feat1=p + 8),
            dict(kp0=p + 4), dict(kp1=p + 4), dict(ws=p + 4), dict(matches0=p + 2), dict(scores0=p + 1),
            dict(matches1=p + 3), dict(counts=p + 2), dict(off0=p + 1), dict(grids1=p + 2)]
    for kw in bad:
        assert call(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_dual_softmax_match'), kw
    for kw in (dict(n0=1 << 31), dict(n1=(1 << 63) - 1), dict(n=(1 << 31) - 1),
               dict(n=1 << 20, max_k0=(1 << 31) - 1, max_k1=(1 << 31) - 1)):
        assert call(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_dual_softmax_match'), kw
    need = lib.oetr_dual_softmax_workspace_bytes(5, 4)
    for kw in (dict(ws_bytes=0), dict(ws_bytes=15), dict(matches1=None, ws_bytes=need - 1),
               dict(ws_bytes=need - 256 - 1)):
        assert call(**kw) == WORKSPACE, kw
        assert lib.oetr_last_error().startswith(b'oetr_dual_softmax_match'), kw
    assert keep.raw == b'\xa5' * 80


def test_match_dense_refuses_before_any_device_use(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    f32 = np.zeros((4, 8), np.float32)
    off, grid = np.array([0, 4], np.int32), np.array([[2, 2]], np.int32)
    joined = dict(offsets0=off, offsets1=off, grids0=grid, grids1=grid, max_k0=4, max_k1=4)
    for f0, f1 in ((f32.astype(np.float64), f32), (f32, torch.zeros(4, 8, dtype=torch.float64))):
        with pytest.raises(ValueError, match='float64'):
            pkg.match_dense(f0, f1, **joined)
    with pytest.raises(ValueError, match='float64'):
        pkg.match_dense([np.zeros((2, 2, 8))], [np.zeros((2, 2, 8), np.float32)])
    for missing in ('offsets0', 'offsets1', 'grids0', 'grids1', 'max_k0', 'max_k1'):
        with pytest.raises(ValueError, match=missing):
            pkg.match_dense(f32, f32, **{k: v for k, v in joined.items() if k != missing})
    with pytest.raises(ValueError, match='offsets0'):
        pkg.match_dense([f32.reshape(2, 2, 8)], [f32.reshape(2, 2, 8)], offsets0=off, offsets1=off)
    with pytest.raises(ValueError, match='one map per pair'):
        pkg.match_dense([f32.reshape(2, 2, 8)], [])
    for kw, what in ((dict(temperature=0), 'temperature'), (dict(temperature=-0.1), 'temperature'),
                     (dict(temperature=float('nan')), 'temperature'), (dict(threshold=-0.01), 'threshold'),
                     (dict(threshold=float('inf')), 'threshold'), (dict(border_rm=-1), 'border_rm'),
                     (dict(border_rm=1.5), 'border_rm'), (dict(cell=0), 'cell')):
        with pytest.raises(ValueError, match=what):
            pkg.match_dense(f32, f32, **joined, **kw)
    with pytest.raises(RuntimeError, match='GPU.*no CPU implementation'):
        pkg.match_dense(f32, f32, **joined)
    with pytest.raises(RuntimeError, match='GPU.*no CPU implementation'):
        pkg.match_dense([torch.zeros(2, 2, 8)], [torch.zeros(1, 3, 8)])
    # host inputs inside a capture: refused by name before anything is uploaded
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: __import__('contextlib').nullcontext())
    with pytest.raises(ValueError, match=r"inside a graph capture.*'offsets0'.*'grids1'.*'feat0'"):
        pkg.match_dense(f32, f32, **joined)
    from imagematching_oetr_amd.dloc_matcher import DualSoftmax
    assert DualSoftmax.required_inputs == ['image0', 'image1']
    assert DualSoftmax.default_conf == {'temperature': 0.1, 'threshold': 0.2, 'border_rm': 2, 'cell': 8}
    assert DualSoftmax({'threshold': 0.3}).conf['threshold'] == 0.3
    with pytest.raises(ValueError, match='net'):
        DualSoftmax({})({'image0': torch.zeros(1), 'image1': torch.zeros(1)})
