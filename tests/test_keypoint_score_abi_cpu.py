"""CPU-only checks of the keypoint-repeatability extension (``include/oetr_keypoint_score.h``,
``csrc/keypoint_score.hip``, ``imagematching_oetr_amd/keypoint_score.py``, ``evaluate.keypoint_repeatability``): header,
export list and library agree, the new exports are disjoint from all the others and the other six headers stand as they
were; the entry's argument types are declared; every host-checked argument error is reported without a GPU and touches
nothing; ``score_keypoints`` refuses float64 keypoints, too many thresholds and a set that is not on a GPU before any
device use; ``keypoint_repeatability`` summarises the pinned counters; ``ground_truth_matches`` on a hand-made result."""
import ctypes
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd import hip_engine

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import keypoint_score_oracle as kso  # noqa: E402

BAD_ARG, BAD_SHAPE = 1, 2
EXPECTED = json.loads((REPO / 'tests' / 'keypoint_score_expected.json').read_text())
HEADER = 'oetr_keypoint_score.h'


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
    assert len(names) == 2 and set(names) == set(hip_engine.KEYPOINT_SCORE_EXPORTS), names
    assert set(names) == {'oetr_keypoint_score_abi_version', 'oetr_keypoint_repeatability'}
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/{HEADER} but not exported'
    assert lib.oetr_keypoint_score_abi_version() == hip_engine.KEYPOINT_SCORE_ABI_VERSION == 1
    text = (REPO / 'include' / HEADER).read_text()
    assert re.search(r'#define\s+OETR_KEYPOINT_SCORE_ABI_VERSION\s+1\b', text)
    assert re.search(r'#define\s+OETR_KEYPOINT_SCORE_MAX_THRESHOLDS\s+8\b', text)
    assert re.search(r'#define\s+OETR_KEYPOINT_SCORE_HEAD_COUNTERS\s+2\b', text)
    assert hip_engine.KEYPOINT_SCORE_MAX_THRESHOLDS == kso.MAX_THRESHOLDS == 8 and hip_engine.KEYPOINT_SCORE_HEAD_COUNTERS == 2
    assert 'typedef struct' not in header_text(HEADER)                      # the set's table type, no second one
    # the other headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(header_functions('oetr_bank.h')) == 3
    assert len(header_functions('oetr_covis.h')) == 3 and len(header_functions('oetr_covis_set.h')) == 4
    assert len(header_functions('oetr_crop_batch.h')) == 3 and len(header_functions('oetr_match_score.h')) == 2
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.COVIS_SET_EXPORTS) | set(hip_engine.CROP_BATCH_EXPORTS) | set(hip_engine.MATCH_SCORE_EXPORTS))
    assert not set(hip_engine.KEYPOINT_SCORE_EXPORTS) & others
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_bank_abi_version() == hip_engine.BANK_ABI_VERSION == 1
    assert lib.oetr_covis_abi_version() == hip_engine.COVIS_ABI_VERSION == 1
    assert lib.oetr_covis_set_abi_version() == hip_engine.COVIS_SET_ABI_VERSION == 1
    assert lib.oetr_crop_batch_abi_version() == hip_engine.CROP_BATCH_ABI_VERSION == 1
    assert lib.oetr_match_score_abi_version() == hip_engine.MATCH_SCORE_ABI_VERSION == 1


def test_argument_types_are_declared():
    lib = pkg.load_library()
    for fn in hip_engine.KEYPOINT_SCORE_EXPORTS:
        f = getattr(lib, fn)
        assert f.argtypes is not None and len(f.argtypes) == parameter_count(HEADER, fn), fn
        assert f.restype is ctypes.c_int, fn
    at = lib.oetr_keypoint_repeatability.argtypes
    assert len(at) == 16
    assert at[3] is ctypes.c_int64 and at[9] is ctypes.POINTER(ctypes.c_double)
    assert all(at[k] is ctypes.c_int for k in (1, 8, 10, 11))
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (1, 3, 8, 9, 10, 11))


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(b'\xa5' * 64, 64)   # host memory standing in for the device: never touched
    p = ctypes.addressof(keep)
    thresholds = (ctypes.c_double * 8)(1, 2, 3, 5, 8, 13, 21, 34)

    def score(maps=p, n_maps=3, kpts=p, n_kpts=7, offsets=p, idx1=p, idx2=p, params=p, n=2, thr=thresholds, n_thr=4,
              max_kp=5, counts=p, nearest=p, dist_sq=p):
        return lib.oetr_keypoint_repeatability(maps, n_maps, kpts, n_kpts, offsets, idx1, idx2, params, n, thr, n_thr,
                                               max_kp, counts, nearest, dist_sq, None)

    for kw in (dict(maps=None), dict(offsets=None), dict(idx1=None), dict(idx2=None), dict(params=None), dict(counts=None),
               dict(counts=None, n_kpts=0, max_kp=0), dict(kpts=None), dict(thr=None), dict(n_thr=-1), dict(n_thr=9),
               dict(n=0), dict(n=-2), dict(n_maps=0), dict(n_maps=-1), dict(n_kpts=-1), dict(n_kpts=-(1 << 63)),
               dict(max_kp=-1), dict(max_kp=-(1 << 31))):
        assert score(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_keypoint_repeatability'), kw
    for kw in (dict(n_kpts=1 << 31), dict(n_kpts=(1 << 63) - 1, nearest=None, dist_sq=None), dict(n=(1 << 31) - 1),
               dict(n=1 << 28, n_thr=8, max_kp=1), dict(n=1 << 20, max_kp=(1 << 31) - 1)):
        assert score(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_keypoint_repeatability'), kw
    assert keep.raw == b'\xa5' * 64


class _Set:
    """Stands in for a DepthSet: ``score_keypoints`` must refuse before it asks it for anything but its device."""
    def __init__(self, device):
        self.device = torch.device(device)

    def __len__(self):
        raise AssertionError('the set was used')

    def _commit(self):
        raise AssertionError('the set was used')


def test_score_keypoints_refuses_before_any_device_use(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    k32 = np.zeros((4, 2), np.float32)
    on_gpu = _Set('cuda:0')
    for kps in ([k32.astype(np.float64), k32], [k32, torch.zeros(4, 2, dtype=torch.float64)],
                (torch.zeros(8, 2, dtype=torch.float64), torch.zeros(3, dtype=torch.int32), 4)):
        with pytest.raises(ValueError, match='float64'):
            pkg.score_keypoints(on_gpu, [(0, 1)], kps)
    with pytest.raises(ValueError, match='at most 8 thresholds'):
        pkg.score_keypoints(on_gpu, [(0, 1)], [k32, k32], thresholds=range(1, 10))
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.score_keypoints(_Set('cpu'), [(0, 1)], [k32, k32])
    with pytest.raises(ValueError, match='nearest=True'):
        pkg.ground_truth_matches({'counts': torch.zeros(1, 2, 6, dtype=torch.int32)}, 3.0)
    for name in ('score_keypoints', 'keypoint_repeatability', 'ground_truth_matches'):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_keypoint_repeatability_on_the_pinned_counters():
    counts = np.array([p['counts'] for s in EXPECTED['sets'] for p in s['pairs']], np.int32)
    assert counts.shape == (48, 2, 6)
    res = pkg.keypoint_repeatability({'counts': torch.from_numpy(counts), 'thresholds': (1.0, 2.0, 3.0, 5.0)})
    want = np.zeros((48, 4))
    for p, c in enumerate(counts.tolist()):
        for t in range(4):
            want[p, t] = sum(side[2 + t] / side[1] if side[1] else 0 for side in c) / 2
    assert np.array_equal(res['repeatability'], want) and np.array_equal(res['repeatability'], kso.repeatability(counts))
    assert np.array_equal(res['mean_repeatability'], want.mean(0)) and res['thresholds'] == (1.0, 2.0, 3.0, 5.0)
    assert (res['n_pairs'], res['n_not_scored']) == (48, 0)
    assert res['n_keypoints'] == int(counts[:, :, 0].sum()) == 2 * 4 * sum(sum(c) for c in kso.COUNTS)
    assert res['n_kept'] == int(counts[:, :, 1].sum())
    assert 0 < want.max() <= 1 and (np.diff(want, axis=1) >= 0).all()
    # pairs the set did not vouch for are left out and counted
    mixed = counts.copy()
    mixed[5] = -1
    res = pkg.keypoint_repeatability(mixed)
    assert np.isnan(res['repeatability'][5]).all() and np.array_equal(np.delete(res['repeatability'], 5, 0), np.delete(want, 5, 0))
    assert np.array_equal(res['mean_repeatability'], np.delete(want, 5, 0).mean(0)) and res['thresholds'] is None
    assert (res['n_pairs'], res['n_not_scored']) == (47, 1)
    none = pkg.keypoint_repeatability(np.full((2, 2, 3), -1, np.int32))
    assert none['n_pairs'] == 0 and np.isnan(none['mean_repeatability']).all() and none['repeatability'].shape == (2, 1)
    with pytest.raises(ValueError, match=r'\[P,2,2\+T\]'):
        pkg.keypoint_repeatability(np.zeros((3, 5), np.int32))


def test_ground_truth_matches_on_a_hand_made_result():
    """Torch gathers, so the function runs on host tensors as well."""
    nan, inf = float('nan'), float('inf')
    #            a: 0  1  2   3  4                b: 0  1  2  3   4
    near = torch.tensor([[[1, 0, 0, -1, 4], [1, 0, 3, 2, -1]],                  # 0 <-> 1 mutual both ways; 2 -> 0 is not
                         [[2, 2, -1, -1, -1], [-1, -1, 1, -1, -1]]], dtype=torch.int32)
    dist = torch.tensor([[[0.5, 8.9, 1.0, nan, inf], [0.5, 9.1, 2.0, 2.0, nan]],
                         [[0.0, 0.0, nan, nan, nan], [nan, nan, 0.0, nan, nan]]], dtype=torch.float64)
    got = pkg.ground_truth_matches({'nearest': near, 'dist_sq': dist}, 3.0)
    # pair 0: a=0 <-> b=1 (0.5, 9.1 >= 9: no); a=1 <-> b=0 (8.9 and 0.5: yes); a=4 -> b=4, whose nearest is -1
    # pair 1: a=0 and a=1 both point at b=2, which points back at a=1 only
    assert got.dtype == torch.int32 and got.tolist() == [[-1, 0, -1, -1, -1], [-1, 2, -1, -1, -1]]
    assert pkg.ground_truth_matches({'nearest': near, 'dist_sq': dist}, 3.5).tolist()[0] == [1, 0, -1, -1, -1]
    empty = {'nearest': torch.zeros(2, 2, 0, dtype=torch.int32), 'dist_sq': torch.zeros(2, 2, 0, dtype=torch.float64)}
    assert pkg.ground_truth_matches(empty, 3.0).shape == (2, 0)
