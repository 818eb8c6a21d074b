"""CPU-only checks of the pose-refit extension (``include/oetr_pose_refit.h``, ``csrc/pose_refit.hip``,
``imagematching_oetr_amd/pose_refit.py``): header, export list and library agree and the other headers stand as they
were; the entry's argument types are declared; every host-checked argument error of the header's table is reported
without a GPU and touches nothing; the Python wrapper refuses float64 keypoints, ``lengths`` together with
``offsets``, limits out of range, misshapen models and a machine without a GPU before any device use."""
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
import pose_refit_oracle as pfo  # noqa: E402

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
    names = header_functions('oetr_pose_refit.h')
    assert len(names) == 2 and set(names) == set(hip_engine.POSE_REFIT_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/oetr_pose_refit.h but not exported'
    assert lib.oetr_pose_refit_abi_version() == hip_engine.POSE_REFIT_ABI_VERSION == 1
    text = (REPO / 'include' / 'oetr_pose_refit.h').read_text()
    assert re.search(r'#define\s+OETR_POSE_REFIT_ABI_VERSION\s+1\b', text)
    assert re.search(r'#define\s+OETR_POSE_REFIT_MAX_ITERS\s+8\b', text)
    assert re.search(r'#define\s+OETR_POSE_REFIT_COUNTERS\s+5\b', text)
    assert hip_engine.POSE_REFIT_MAX_ITERS == pfo.MAX_REFIT == 8
    assert hip_engine.POSE_REFIT_COUNTERS == pfo.COUNTERS == hip_engine.POSE_RANSAC_COUNTERS == 5
    assert 'typedef struct' not in header_text('oetr_pose_refit.h')
    # the other headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(header_functions('oetr_bank.h')) == 3
    assert len(header_functions('oetr_covis.h')) == 3 and len(header_functions('oetr_covis_set.h')) == 4
    assert len(header_functions('oetr_crop_batch.h')) == 3 and len(header_functions('oetr_match_score.h')) == 2
    assert len(header_functions('oetr_keypoint_score.h')) == 2 and len(header_functions('oetr_match_assembly.h')) == 3
    assert len(header_functions('oetr_homography.h')) == 4 and len(header_functions('oetr_pose_ransac.h')) == 4
    assert len(header_functions('oetr_nn_match.h')) == 3 and len(header_functions('oetr_homography_ransac.h')) == 3
    assert parameter_count('oetr_pose_ransac.h', 'oetr_pose_ransac') == 20
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.COVIS_SET_EXPORTS) | set(hip_engine.CROP_BATCH_EXPORTS)
              | set(hip_engine.MATCH_SCORE_EXPORTS) | set(hip_engine.KEYPOINT_SCORE_EXPORTS)
              | set(hip_engine.MATCH_ASSEMBLY_EXPORTS) | set(hip_engine.HOMOGRAPHY_EXPORTS)
              | set(hip_engine.POSE_RANSAC_EXPORTS) | set(hip_engine.NN_MATCH_EXPORTS)
              | set(hip_engine.HOMOGRAPHY_RANSAC_EXPORTS))
    assert not set(hip_engine.POSE_REFIT_EXPORTS) & others
    assert len(hip_engine.POSE_RANSAC_EXPORTS) == 4 and len(hip_engine.HOMOGRAPHY_RANSAC_EXPORTS) == 3
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_match_score_abi_version() == hip_engine.MATCH_SCORE_ABI_VERSION == 1
    assert lib.oetr_pose_ransac_abi_version() == hip_engine.POSE_RANSAC_ABI_VERSION == 1
    assert lib.oetr_homography_ransac_abi_version() == hip_engine.HOMOGRAPHY_RANSAC_ABI_VERSION == 1
    assert lib.oetr_nn_match_abi_version() == hip_engine.NN_MATCH_ABI_VERSION == 1


def test_argument_types_are_declared():
    lib = pkg.load_library()
    for fn in hip_engine.POSE_REFIT_EXPORTS:
        f = getattr(lib, fn)
        assert f.argtypes is not None and len(f.argtypes) == parameter_count('oetr_pose_refit.h', fn), fn
        assert f.restype is ctypes.c_int, fn
    at = lib.oetr_pose_refit.argtypes
    assert len(at) == 15 and at[5] is ctypes.c_int64 and at[7] is ctypes.c_double and at[2] is at[8] is ctypes.c_int
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (2, 5, 7, 8))


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(b'\xa5' * 64, 64)   # host memory standing in for the device: never touched
    p = ctypes.addressof(keep)

    def call(params=p, offsets=p, n=2, k1=p, k2=p, m=5, model_in=p, px_thr=1.0, refit=4, model=p, pose=p, cosines=p,
             counts=p, inliers=p):
        return lib.oetr_pose_refit(params, offsets, n, k1, k2, m, model_in, px_thr, refit, model, pose, cosines, counts,
                                   inliers, None)

    for kw in (dict(params=None), dict(offsets=None), dict(model_in=None), dict(model=None), dict(pose=None),
               dict(cosines=None), dict(counts=None), dict(k1=None), dict(k2=None), dict(n=0), dict(n=-3), dict(m=-1),
               dict(m=-(1 << 63)), dict(refit=-1), dict(refit=9), dict(refit=INT32_MAX), dict(refit=-INT32_MAX - 1),
               dict(px_thr=0.0), dict(px_thr=-1.0), dict(px_thr=float('nan')), dict(px_thr=float('inf'))):
        assert call(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_pose_refit:'), kw
    for kw in (dict(m=1 << 31), dict(m=(1 << 63) - 1)):
        assert call(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_pose_refit:'), kw
    assert keep.raw == b'\xa5' * 64


def test_wrapper_refuses_before_any_device_use(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    k32 = np.zeros((8, 2), np.float32)
    P, F = np.zeros((1, 20)), np.ones((1, 9))
    for k1, k2 in ((k32.astype(np.float64), k32), (k32, torch.zeros(8, 2, dtype=torch.float64))):
        with pytest.raises(ValueError, match='float64'):
            pkg.refine_poses(P, k1, k2, F, lengths=[8])
    with pytest.raises(ValueError, match='exactly one'):
        pkg.refine_poses(P, k32, k32, F, lengths=[8], offsets=torch.tensor([0, 8], dtype=torch.int32))
    with pytest.raises(ValueError, match='exactly one'):
        pkg.refine_poses(P, k32, k32, F)
    for refit in (-1, 9, 1.5):
        with pytest.raises(ValueError, match='refit_iters'):
            pkg.refine_poses(P, k32, k32, F, lengths=[8], refit_iters=refit)
    for thr in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='px_thr'):
            pkg.refine_poses(P, k32, k32, F, lengths=[8], px_thr=thr)
    for models in (np.zeros((1, 3, 9)), np.zeros((1, 8)), np.zeros(9)):
        with pytest.raises(ValueError, match='models must be'):
            pkg.refine_poses(P, k32, k32, models, lengths=[8])
    with pytest.raises(RuntimeError, match='There is no CPU implementation'):
        pkg.refine_poses(P, k32, k32, F, lengths=[8])
    assert 'refine_poses' in pkg.__all__ and hasattr(pkg, 'refine_poses')
    for name in ('estimate_poses', 'pose_errors', 'pose_auc', 'match_pose_auc'):
        assert name in pkg.__all__
