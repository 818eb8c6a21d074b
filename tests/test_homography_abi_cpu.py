"""CPU-only checks of the homography extension (``include/oetr_homography.h``, ``csrc/homography.hip``,
``imagematching_oetr_amd/homography.py``): header, export list and library agree and the other headers stand as they
were; the entries' argument types are declared; every host-checked argument error of the header's table is reported
without a GPU and touches nothing; the Python wrappers refuse float64 keypoints, ``lengths`` together with ``offsets``
and a machine without a GPU before any device use."""
import ctypes
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
import homography_oracle as ho  # noqa: E402

BAD_ARG, BAD_SHAPE = 1, 2
INT32_MAX = (1 << 31) - 1


def header_text(name):
    return re.sub(r'/\*.*?\*/', '', (REPO / 'include' / name).read_text(), flags=re.S)


def header_functions(name):
    return sorted(set(re.findall(r'\b(oetr_[a-z_0-9]+)\s*\(', header_text(name))))


def parameter_count(name, fn):
    args = re.search(r'\b' + fn + r'\s*\(([^)]*)\)', header_text(name)).group(1).strip()
    return 0 if args == 'void' else len(args.split(','))


def test_header_exports_library_and_versions_agree():
    lib = pkg.load_library()
    names = header_functions('oetr_homography.h')
    assert len(names) == 4 and set(names) == set(hip_engine.HOMOGRAPHY_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/oetr_homography.h but not exported'
    assert lib.oetr_homography_abi_version() == hip_engine.HOMOGRAPHY_ABI_VERSION == 1
    text = (REPO / 'include' / 'oetr_homography.h').read_text()
    assert re.search(r'#define\s+OETR_HOMOGRAPHY_ABI_VERSION\s+1\b', text)
    assert re.search(r'#define\s+OETR_HOMOGRAPHY_PARAM_DOUBLES\s+16\b', text)
    assert re.search(r'#define\s+OETR_HOMOGRAPHY_MAX_THRESHOLDS\s+16\b', text)
    assert hip_engine.HOMOGRAPHY_PARAM_DOUBLES == ho.PARAM_DOUBLES == 16
    assert hip_engine.HOMOGRAPHY_MAX_THRESHOLDS == ho.MAX_THRESHOLDS == 16
    assert 'typedef struct' not in header_text('oetr_homography.h')
    # the other headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(header_functions('oetr_bank.h')) == 3
    assert len(header_functions('oetr_covis.h')) == 3 and len(header_functions('oetr_covis_set.h')) == 4
    assert len(header_functions('oetr_crop_batch.h')) == 3 and len(header_functions('oetr_match_score.h')) == 2
    assert len(header_functions('oetr_keypoint_score.h')) == 2 and len(header_functions('oetr_match_assembly.h')) == 3
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.COVIS_SET_EXPORTS) | set(hip_engine.CROP_BATCH_EXPORTS)
              | set(hip_engine.MATCH_SCORE_EXPORTS) | set(hip_engine.KEYPOINT_SCORE_EXPORTS)
              | set(hip_engine.MATCH_ASSEMBLY_EXPORTS))
    assert not set(hip_engine.HOMOGRAPHY_EXPORTS) & others
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_covis_abi_version() == hip_engine.COVIS_ABI_VERSION == 1
    assert lib.oetr_match_score_abi_version() == hip_engine.MATCH_SCORE_ABI_VERSION == 1
    assert lib.oetr_keypoint_score_abi_version() == hip_engine.KEYPOINT_SCORE_ABI_VERSION == 1
    assert lib.oetr_match_assembly_abi_version() == hip_engine.MATCH_ASSEMBLY_ABI_VERSION == 1


def test_argument_types_are_declared():
    lib = pkg.load_library()
    for fn in hip_engine.HOMOGRAPHY_EXPORTS:
        f = getattr(lib, fn)
        assert f.argtypes is not None and len(f.argtypes) == parameter_count('oetr_homography.h', fn), fn
        assert f.restype is (ctypes.c_size_t if fn.endswith('workspace_bytes') else ctypes.c_int), fn
    at = lib.oetr_homography_match_score.argtypes
    assert len(at) == 11 and at[5] is ctypes.c_int64 and at[2] is ctypes.c_int and at[7] is ctypes.c_int
    assert at[6] is ctypes.POINTER(ctypes.c_double)                      # the HOST thresholds
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (2, 5, 6, 7))
    at = lib.oetr_homography_boxes.argtypes
    assert len(at) == 11 and list(at[1:4]) == [ctypes.c_int] * 3 and at[5] is ctypes.c_size_t
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (1, 2, 3, 5))


def test_workspace_bytes():
    lib = pkg.load_library()
    assert lib.oetr_homography_workspace_bytes(0) == 0 and lib.oetr_homography_workspace_bytes(-4) == 0
    assert lib.oetr_homography_workspace_bytes(1) > 0
    assert lib.oetr_homography_workspace_bytes(7) == 7 * lib.oetr_homography_workspace_bytes(1)


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(b'\xa5' * 64, 64)   # host memory standing in for the device: never touched
    p = ctypes.addressof(keep)
    thr = (ctypes.c_double * 16)(*range(1, 17))

    def score(params=p, offsets=p, n=2, k1=p, k2=p, m=5, thresholds=thr, t=15, dist_sq=p, counts=p):
        return lib.oetr_homography_match_score(params, offsets, n, k1, k2, m, thresholds, t, dist_sq, counts, None)

    for kw in (dict(params=None), dict(offsets=None), dict(counts=None), dict(counts=None, m=0), dict(k1=None),
               dict(k2=None), dict(thresholds=None), dict(t=-1), dict(t=17), dict(n=0), dict(n=-2), dict(m=-1),
               dict(m=-(1 << 63))):
        assert score(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_homography_match_score'), kw
    for kw in (dict(m=1 << 31), dict(m=(1 << 31) + 5, dist_sq=None), dict(m=(1 << 63) - 1),
               dict(n=INT32_MAX // 17 + 1), dict(n=INT32_MAX)):
        assert score(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_homography_match_score'), kw

    need = lib.oetr_homography_workspace_bytes(2)

    def boxes(params=p, n=2, max_h1=480, max_w1=640, workspace=p, nbytes=need, box1=p, box2=p, valid=p, count=p):
        return lib.oetr_homography_boxes(params, n, max_h1, max_w1, workspace, nbytes, box1, box2, valid, count, None)

    for kw in (dict(params=None), dict(box1=None), dict(box2=None), dict(valid=None), dict(n=0), dict(n=-1),
               dict(workspace=None), dict(nbytes=need - 1), dict(nbytes=0), dict(valid=None, count=None)):
        assert boxes(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_homography_boxes'), kw
    for kw in (dict(max_h1=0), dict(max_w1=0), dict(max_h1=-3), dict(max_h1=8193), dict(max_w1=8193),
               dict(max_w1=INT32_MAX), dict(n=INT32_MAX // 17 + 1, nbytes=(1 << 63))):
        assert boxes(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_homography_boxes'), kw
    assert keep.raw == b'\xa5' * 64


def test_wrappers_refuse_before_any_device_use(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    k32 = np.zeros((4, 2), np.float32)
    H = np.eye(3)
    for k1, k2 in ((k32.astype(np.float64), k32), (k32, torch.zeros(4, 2, dtype=torch.float64))):
        with pytest.raises(ValueError, match='float64'):
            pkg.score_matches_homography(H, k1, k2, lengths=[4])
    with pytest.raises(ValueError, match='exactly one'):
        pkg.score_matches_homography(H, k32, k32, lengths=[4], offsets=torch.tensor([0, 4], dtype=torch.int32))
    with pytest.raises(ValueError, match='exactly one'):
        pkg.score_matches_homography(H, k32, k32)
    with pytest.raises(ValueError, match='at most 16'):
        pkg.score_matches_homography(H, k32, k32, lengths=[4], thresholds=range(17))
    sentence = 'There is no CPU implementation'
    with pytest.raises(RuntimeError, match=sentence):
        pkg.score_matches_homography(H, k32, k32, lengths=[4])
    with pytest.raises(RuntimeError, match=sentence):
        pkg.overlap_boxes_from_homography(H, (5, 7), (7, 5))
    with pytest.raises(RuntimeError, match=sentence):
        pkg.homography_params(H, (5, 7), (7, 5))
    with pytest.raises(RuntimeError, match=sentence):
        pkg.homography_params(H, (5, 7), (7, 5), device='cpu')
    for name in ('homography_params', 'rescale_homography', 'score_matches_homography', 'homography_accuracy',
                 'overlap_boxes_from_homography'):
        assert name in pkg.__all__ and hasattr(pkg, name)
