"""CPU-only checks of the nearest-neighbour matcher extension (``include/oetr_nn_match.h``, ``csrc/nn_match.hip``,
``imagematching_oetr_amd/nn_match.py``) and of its specification ``tests/nn_match_oracle.py``.

The specification: its ``fmaf`` emulation equals exact rational arithmetic rounded once, on random and on constructed
near-midpoint triples; its order-free top two equal a brute-force sort; the pinned calls regenerate the recorded
results; swapping the sides under the mutual check gives the inverse mapping.  The fixture's comparison with the
reference's own ``find_nn`` / ``mutual_check`` happened and stayed inside its caps.

The ABI: header, export list and library agree and the other lists stand as they were; argument types are declared;
every host-checked argument error is reported without a GPU and touches nothing; the wrapper refuses before any device
use."""
import ctypes
import json
import re
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd import hip_engine

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import nn_match_cases as nmc  # noqa: E402
import nn_match_oracle as nmo  # noqa: E402

BAD_ARG, BAD_SHAPE, WORKSPACE = 1, 2, 4
EXPECTED = json.loads((REPO / 'tests' / 'nn_match_expected.json').read_text())
F32 = np.float32


# ---------------------------------------------------------------------------------------- the specification
def round_to_float32(x):
    """The float32 nearest to the rational ``x``, ties to even, found among the neighbours of a first guess."""
    guess = F32(float(x))
    best = None
    for c in (np.nextafter(guess, F32(-np.inf)), guess, np.nextafter(guess, F32(np.inf))):
        err = abs(x - Fraction(float(c)))
        even = (int(c.view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, c)
    return best[1]


def fma_triples():
    rng = np.random.default_rng(11)
    n = 1500
    a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    yield a, b, rng.standard_normal(n).astype(F32)
    # cancellation: c close to -a * b
    yield a, b, (-(a.astype(np.float64) * b)).astype(F32) + (rng.standard_normal(n) * 1e-7).astype(F32)
    # near a float32 midpoint: c = 1 + k ulp, a * b = 2^-24 (1 + e1)(1 + e2) with |e| a few ulp: the exact sum is a
    # midpoint of float32 plus or minus less than float64 can hold, so only the rounding to odd tells the side
    k = rng.integers(0, 64, n)
    e1, e2 = rng.integers(-3, 4, n), rng.integers(-3, 4, n)
    yield ((1 + e1 * 2.0 ** -23) * 2.0 ** -12).astype(F32), ((1 + e2 * 2.0 ** -23) * 2.0 ** -12).astype(F32), \
        (1 + k * 2.0 ** -23).astype(F32)
    # small and subnormal results
    yield (a * F32(2.0 ** -70)), (b * F32(2.0 ** -70)), (rng.standard_normal(n) * 2.0 ** -140).astype(F32)


def test_fma_emulation_equals_exact_rationals():
    checked = ties = 0
    for a, b, c in fma_triples():
        got = nmo.fma32(a, b, c)
        assert got.dtype == F32
        for x, y, z, g in zip(a, b, c, got):
            exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
            assert g.view(np.uint32) == round_to_float32(exact).view(np.uint32) or (g == 0 and exact == 0), (x, y, z, g)
            ties += Fraction(float(x) * float(y) + float(z)) != exact       # the float64 sum alone was inexact
            checked += 1
    assert checked >= 6000 and ties >= 1000
    # the chain is one rounding per step: not the float64 dot product rounded once
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((40, 128)).astype(F32), rng.standard_normal((50, 128)).astype(F32)
    sim = nmo.similarity(A, B)
    assert sim.dtype == F32 and sim.shape == (40, 50)
    assert (sim != (A.astype(np.float64) @ B.astype(np.float64).T).astype(F32)).any()
    assert np.array_equal(nmo.similarity(B, A), sim.T)                     # fmaf commutes: the transpose, bit for bit
    acc = F32(0)
    for d in range(128):
        acc = nmo.fma32(A[3, d], B[7, d], acc)
    assert acc == sim[3, 7]


def brute_top2(row):
    order = sorted((j for j, v in enumerate(row) if not np.isnan(v) and v != -np.inf), key=lambda j: (-row[j], j))
    b1 = row[order[0]] if order else F32(-np.inf)
    b2 = row[order[1]] if len(order) > 1 else F32(-np.inf)
    return b1, (order[0] if order else -1), b2


def test_top_two_is_order_free():
    rng = np.random.default_rng(3)
    for K in (0, 1, 2, 3, 17, 64):
        sim = (rng.integers(-3, 4, (200, K)) / 4).astype(F32)               # few values: many ties
        special = rng.random((200, K))
        sim[special < 0.15] = np.nan
        sim[(special >= 0.15) & (special < 0.3)] = -np.inf
        sim[(special >= 0.3) & (special < 0.33)] = np.inf
        b1, i1, b2 = nmo.top2(sim)
        for r in range(200):
            want = brute_top2(sim[r])
            assert (b1[r], i1[r], b2[r]) == want, (K, r, sim[r])
            perm = rng.permutation(K)                                       # walked in another order: same values
            p1, pi, p2 = nmo.top2(sim[r][perm])
            assert (p1, p2) == (want[0], want[2]) and (pi < 0 or perm[pi] >= want[1])
    m, s = nmo.find_nn(np.array([[0.5]], F32), ratio_threshold=0.8)         # K1 = 1: b2 = -inf passes the ratio test
    assert m.tolist() == [0] and s.tolist() == [0.75]
    m, s = nmo.find_nn(np.array([[np.nan, -np.inf]], F32))
    assert m.tolist() == [-1] and s.tolist() == [0.0]


def test_pinned_calls_are_the_recorded_ones():
    assert EXPECTED['settings'] == [nmc.setting_key(*s) for s in nmc.SETTINGS] and len(nmc.SETTINGS) == 8
    assert sorted(EXPECTED['calls']) == sorted(f'{n}/{k}' for n, k in nmc.CALLS)
    sides = nmc.SHAPES['ragged128'][1]
    assert nmc.SHAPES['ragged128'][0] == 128 and len(sides) == 12
    assert {q[0] for q in sides} == {q[1] for q in sides} == set(nmc.K_EDGES)
    assert max(nmc.SHAPES['wide256'][1]) == (300, 257) and nmc.SHAPES['wide256'][0] == 256
    assert all(max(q) <= 65 for n in ('d4', 'd512') for q in nmc.SHAPES[n][1])
    passed_some = failed_some = unmutual = 0
    for name, kind in nmc.CALLS:
        call, rec = nmc.make_call(name, kind), EXPECTED['calls'][f'{name}/{kind}']
        assert rec['D'] == call['D'] and rec['pairs'] == [list(q) for q in call['pairs']]
        assert rec['inputs_sha256'] == dict(desc0=nmc.sha(call['desc0']), desc1=nmc.sha(call['desc1']))
        if kind == 'grid':
            assert (np.abs(call['desc0'] * 64) <= 8).all() and (call['desc0'] * 64 == np.round(call['desc0'] * 64)).all()
            exact = [(a.astype(np.float64) @ b.astype(np.float64).T) for a, b in
                     ((call['desc0'][call['off0'][p]:call['off0'][p + 1]], call['desc1'][call['off1'][p]:call['off1'][p + 1]])
                      for p in range(len(call['pairs'])))]
            assert all(np.array_equal(e, s) for e, s in zip(exact, call['sims']))         # any order: the same similarity
        for setting in nmc.SETTINGS:
            res = nmc.expected(call, *setting)
            assert nmc.result_record(res) == rec['results'][nmc.setting_key(*setting)], (name, kind, setting)
            c = res['counts']
            passed_some += int((c[:, 2] > 0).sum())
            failed_some += int((c[:, 2] < c[:, 0]).sum())
            unmutual += int((c[:, 3] < c[:, 2]).sum())
            # scores stay direction 0's, before the mutual check
            assert ((res['matching_scores0'] != 0).sum() >= (res['matches0'] > -1).sum())
    assert passed_some and failed_some and unmutual


def test_grid_calls_carry_ties_and_duplicates():
    for name in ('ragged128', 'wide256'):
        call = nmc.make_call(name, 'grid')
        tied_rows = tied_cols = 0
        for sim in call['sims']:
            if min(sim.shape) >= 2:
                b1, _, b2 = nmo.top2(sim)
                tied_rows += int((b1 == b2).sum())
                c1, _, c2 = nmo.top2(sim.T)
                tied_cols += int((c1 == c2).sum())
        assert tied_rows >= 4 and tied_cols >= 4, (name, tied_rows, tied_cols)
        for desc, off in ((call['desc0'], call['off0']), (call['desc1'], call['off1'])):
            copies = 0
            for p, (K0, _) in enumerate(call['pairs']):
                rows = desc[off[p]:off[p + 1]]
                copies += len(rows) - len(np.unique(rows, axis=0)) if len(rows) else 0
                assert K0 >= nmc.DUPLICATE_MIN_K0 or len(rows) == len(np.unique(rows, axis=0)) or not len(rows)
            assert 1 <= copies <= nmc.MAX_DUPLICATES, (name, copies)


def test_reference_bookkeeping_of_the_fixture():
    assert EXPECTED['reference_checked'] is True, 'regenerate the fixture where build() has placed the reference snapshot'
    assert EXPECTED['max_excluded_share'] == {'unit': 0.0, 'grid': 0.10}
    for key, rec in EXPECTED['calls'].items():
        ref = rec['reference']
        kind = key.split('/')[1]
        assert ref['rows_compared'] > 0 and ref['excluded_share'] <= EXPECTED['max_excluded_share'][kind], key
        if kind == 'unit':
            assert ref['rows_excluded'] == 0, key
        assert ref['excluded_share'] == ref['rows_excluded'] / (ref['rows_compared'] + ref['rows_excluded'])
    # a side without rows, and a side of one row under a ratio threshold: counted, not compared
    assert EXPECTED['calls']['ragged128/unit']['reference']['reference_cannot_run'] == 2 * 8 + 2 * 4
    assert len(EXPECTED['departures']) == 2


def test_swapped_sides_give_the_inverse_mapping():
    for name, kind in (('ragged128', 'grid'), ('d512', 'unit')):
        call = nmc.make_call(name, kind)
        for sim in call['sims']:
            for ratio, distance in nmc.THRESHOLDS:
                fwd = nmo.match_similarity(sim, ratio, distance, True)
                back = nmo.match_similarity(np.ascontiguousarray(sim.T), ratio, distance, True)
                m, inv = fwd['matches0'], back['matches0']
                assert fwd['counts'][3] == back['counts'][3] == (m > -1).sum() == (inv > -1).sum()
                rows = np.nonzero(m > -1)[0]
                assert np.array_equal(inv[m[rows]], rows)
                cols = np.nonzero(inv > -1)[0]
                assert np.array_equal(m[inv[cols]], cols)


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
    names = header_functions('oetr_nn_match.h')
    assert len(names) == 3 and set(names) == set(hip_engine.NN_MATCH_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/oetr_nn_match.h but not exported'
    assert lib.oetr_nn_match_abi_version() == hip_engine.NN_MATCH_ABI_VERSION == 1
    text = (REPO / 'include' / 'oetr_nn_match.h').read_text()
    assert re.search(r'#define\s+OETR_NN_MATCH_ABI_VERSION\s+1\b', text)
    assert re.search(r'#define\s+OETR_NN_MATCH_COUNTERS\s+4\b', text)
    for macro, value in (('RATIO', hip_engine.NN_MATCH_RATIO), ('DISTANCE', hip_engine.NN_MATCH_DISTANCE),
                         ('MUTUAL', hip_engine.NN_MATCH_MUTUAL)):
        assert re.search(r'#define\s+OETR_NN_MATCH_%s\s+%du\b' % (macro, value), text), macro
    assert re.search(r'#define\s+OETR_NN_MATCH_MIN_D\s+4\b', text) and re.search(r'#define\s+OETR_NN_MATCH_MAX_D\s+512\b', text)
    assert hip_engine.NN_MATCH_COUNTERS == nmo.COUNTERS == 4
    # the other headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(header_functions('oetr_match_assembly.h')) == 3
    assert len(header_functions('oetr_homography.h')) == 4 and len(header_functions('oetr_pose_ransac.h')) == 4
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.COVIS_SET_EXPORTS) | set(hip_engine.CROP_BATCH_EXPORTS)
              | set(hip_engine.MATCH_SCORE_EXPORTS) | set(hip_engine.KEYPOINT_SCORE_EXPORTS)
              | set(hip_engine.MATCH_ASSEMBLY_EXPORTS) | set(hip_engine.HOMOGRAPHY_EXPORTS)
              | set(hip_engine.POSE_RANSAC_EXPORTS))
    assert not set(hip_engine.NN_MATCH_EXPORTS) & others
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_match_assembly_abi_version() == hip_engine.MATCH_ASSEMBLY_ABI_VERSION == 1
    assert lib.oetr_pose_ransac_abi_version() == hip_engine.POSE_RANSAC_ABI_VERSION == 1


def test_argument_types_are_declared():
    lib = pkg.load_library()
    for fn in hip_engine.NN_MATCH_EXPORTS:
        f = getattr(lib, fn)
        assert f.argtypes is not None and len(f.argtypes) == parameter_count('oetr_nn_match.h', fn), fn
    assert lib.oetr_nn_match.restype is ctypes.c_int and lib.oetr_nn_match_workspace_bytes.restype is ctypes.c_size_t
    at = lib.oetr_nn_match.argtypes
    assert len(at) == 20 and at[2] is ctypes.c_int64 and at[5] is ctypes.c_int64 and at[14] is ctypes.c_size_t
    assert all(at[k] is ctypes.c_int for k in (6, 7, 8, 9)) and at[10] is at[11] is ctypes.c_float
    assert at[12] is ctypes.c_uint
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (2, 5, 6, 7, 8, 9, 10, 11, 12, 14))
    assert lib.oetr_nn_match_workspace_bytes(0) == 0 and lib.oetr_nn_match_workspace_bytes(-3) == 0
    assert lib.oetr_nn_match_workspace_bytes(1) >= 4 and lib.oetr_nn_match_workspace_bytes(1000) >= 4000
    assert lib.oetr_nn_match_workspace_bytes(2 ** 31 - 1) >= 4 * (2 ** 31 - 1)


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(b'\xa5' * 80, 80)   # host memory standing in for the device: never touched
    p = (ctypes.addressof(keep) + 15) // 16 * 16           # 16-byte aligned, 64 bytes behind it

    def call(desc0=p, off0=p, n0=5, desc1=p, off1=p, n1=4, n=2, D=128, max_k0=3, max_k1=2, flags=7, ws=p,
             ws_bytes=1 << 20, matches0=p, scores0=p, matches1=p, counts=p):
        return lib.oetr_nn_match(desc0, off0, n0, desc1, off1, n1, n, D, max_k0, max_k1, 0.64, 0.49, flags, ws, ws_bytes,
                                 matches0, scores0, matches1, counts, None)

    bad = [{k: None} for k in ('desc0', 'off0', 'desc1', 'off1', 'matches0', 'scores0', 'counts')]
    bad += [dict(matches1=None, ws=None), dict(counts=None, n0=0, n1=0), dict(n=0), dict(n=-2), dict(n0=-1),
            dict(n1=-(1 << 63)), dict(max_k0=-1), dict(max_k1=-5), dict(D=0), dict(D=2), dict(D=-4), dict(D=130),
            dict(D=516), dict(D=1024), dict(flags=8), dict(flags=0xffffffff), dict(desc0=p + 4), dict(desc1=p + 8),
            dict(matches0=p + 2), dict(scores0=p + 1), dict(matches1=p + 3), dict(counts=p + 2), dict(ws=p + 1)]
    for kw in bad:
        assert call(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_nn_match'), kw
    for kw in (dict(n0=1 << 31), dict(n1=(1 << 63) - 1), dict(n=(1 << 31) - 1),
               dict(n=1 << 20, max_k0=(1 << 31) - 1, max_k1=(1 << 31) - 1)):
        assert call(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_nn_match'), kw
    for kw in (dict(matches1=None, ws_bytes=0), dict(matches1=None, ws_bytes=15),
               dict(matches1=None, n1=100000, ws_bytes=399999)):
        assert call(**kw) == WORKSPACE, kw
        assert lib.oetr_last_error().startswith(b'oetr_nn_match'), kw
    assert keep.raw == b'\xa5' * 80


def test_match_descriptors_refuses_before_any_device_use(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    d32 = np.zeros((4, 8), np.float32)
    off = np.array([0, 4], np.int32)
    for d0, d1 in ((d32.astype(np.float64), d32), (d32, torch.zeros(4, 8, dtype=torch.float64))):
        with pytest.raises(ValueError, match='float64'):
            pkg.match_descriptors(d0, d1, offsets0=off, offsets1=off, max_k0=4, max_k1=4)
        with pytest.raises(ValueError, match='float64'):
            pkg.match_descriptors([d0], [d1])
    with pytest.raises(ValueError, match='offsets0'):
        pkg.match_descriptors(d32, d32, max_k0=4, max_k1=4)
    with pytest.raises(ValueError, match='offsets0'):
        pkg.match_descriptors(d32, d32, offsets0=off, max_k0=4, max_k1=4)
    with pytest.raises(ValueError, match='offsets0'):
        pkg.match_descriptors([d32], [d32], offsets0=off, offsets1=off)
    with pytest.raises(ValueError, match='max_k0'):
        pkg.match_descriptors(d32, d32, offsets0=off, offsets1=off)
    with pytest.raises(ValueError, match='max_k0'):
        pkg.match_descriptors(d32, d32, offsets0=off, offsets1=off, max_k0=4)
    with pytest.raises(ValueError, match='one tensor per pair'):
        pkg.match_descriptors([d32], [d32, d32])
    with pytest.raises(RuntimeError, match='GPU.*no CPU implementation'):
        pkg.match_descriptors(d32, d32, offsets0=off, offsets1=off, max_k0=4, max_k1=4)
    with pytest.raises(RuntimeError, match='GPU.*no CPU implementation'):
        pkg.match_descriptors([torch.zeros(4, 8)], [torch.zeros(3, 8)])
    for name in ('match_descriptors', 'match_counts'):
        assert name in pkg.__all__ and hasattr(pkg, name)
    from imagematching_oetr_amd.dloc_matcher import NearestNeighbor
    assert NearestNeighbor.default_conf == {'ratio_threshold': None, 'distance_threshold': None, 'do_mutual_check': True}
    assert NearestNeighbor({}).conf['do_mutual_check'] is True
