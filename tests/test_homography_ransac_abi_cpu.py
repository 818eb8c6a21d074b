"""CPU-only checks of the homography-estimation extension (``include/oetr_homography_ransac.h``,
``csrc/homography_ransac.hip``, ``imagematching_oetr_amd/homography_ransac.py``): header, export list and library
agree and the other headers stand as they were; the entries' argument types are declared; the workspace size; every
host-checked argument error of the header's table is reported without a GPU and touches nothing; the Python wrapper
refuses float64 keypoints, ``lengths`` together with ``offsets``, limits out of range and a machine without a GPU
before any device use."""
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
import homography_ransac_oracle as hro  # noqa: E402

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
    names = header_functions('oetr_homography_ransac.h')
    assert len(names) == 3 and set(names) == set(hip_engine.HOMOGRAPHY_RANSAC_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/oetr_homography_ransac.h but not exported'
    assert lib.oetr_homography_ransac_abi_version() == hip_engine.HOMOGRAPHY_RANSAC_ABI_VERSION == 1
    text = (REPO / 'include' / 'oetr_homography_ransac.h').read_text()
    assert re.search(r'#define\s+OETR_HOMOGRAPHY_RANSAC_ABI_VERSION\s+1\b', text)
    assert re.search(r'#define\s+OETR_HOMOGRAPHY_RANSAC_MAX_HYPOTHESES\s+4096\b', text)
    assert re.search(r'#define\s+OETR_HOMOGRAPHY_RANSAC_MAX_MODELS\s+4096\b', text)
    assert re.search(r'#define\s+OETR_HOMOGRAPHY_RANSAC_COUNTERS\s+6\b', text)
    assert hip_engine.HOMOGRAPHY_RANSAC_MAX_HYPOTHESES == hro.MAX_HYPOTHESES == 4096
    assert hip_engine.HOMOGRAPHY_RANSAC_MAX_MODELS == hro.MAX_MODELS == 4096
    assert re.search(r'#define\s+OETR_HOMOGRAPHY_RANSAC_MAX_REFIT\s+4\b', text)
    assert hip_engine.HOMOGRAPHY_RANSAC_MAX_REFIT == hro.MAX_REFIT == 4
    assert hip_engine.HOMOGRAPHY_RANSAC_COUNTERS == hro.COUNTERS == 6
    assert hip_engine.HOMOGRAPHY_PARAM_DOUBLES == hro.PARAM_DOUBLES == 16 and hip_engine.COVIS_MAX_SIDE == hro.MAX_SIDE
    assert 'typedef struct' not in header_text('oetr_homography_ransac.h')
    # the other headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(header_functions('oetr_bank.h')) == 3
    assert len(header_functions('oetr_covis.h')) == 3 and len(header_functions('oetr_covis_set.h')) == 4
    assert len(header_functions('oetr_crop_batch.h')) == 3 and len(header_functions('oetr_match_score.h')) == 2
    assert len(header_functions('oetr_keypoint_score.h')) == 2 and len(header_functions('oetr_match_assembly.h')) == 3
    assert len(header_functions('oetr_homography.h')) == 4 and len(header_functions('oetr_pose_ransac.h')) == 4
    assert len(header_functions('oetr_nn_match.h')) == 3
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.COVIS_SET_EXPORTS) | set(hip_engine.CROP_BATCH_EXPORTS)
              | set(hip_engine.MATCH_SCORE_EXPORTS) | set(hip_engine.KEYPOINT_SCORE_EXPORTS)
              | set(hip_engine.MATCH_ASSEMBLY_EXPORTS) | set(hip_engine.HOMOGRAPHY_EXPORTS) | set(hip_engine.POSE_RANSAC_EXPORTS)
              | set(hip_engine.NN_MATCH_EXPORTS))
    assert not set(hip_engine.HOMOGRAPHY_RANSAC_EXPORTS) & others
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_covis_abi_version() == hip_engine.COVIS_ABI_VERSION == 1
    assert lib.oetr_match_score_abi_version() == hip_engine.MATCH_SCORE_ABI_VERSION == 1
    assert lib.oetr_keypoint_score_abi_version() == hip_engine.KEYPOINT_SCORE_ABI_VERSION == 1
    assert lib.oetr_match_assembly_abi_version() == hip_engine.MATCH_ASSEMBLY_ABI_VERSION == 1
    assert lib.oetr_homography_abi_version() == hip_engine.HOMOGRAPHY_ABI_VERSION == 1
    assert lib.oetr_pose_ransac_abi_version() == hip_engine.POSE_RANSAC_ABI_VERSION == 1
    assert lib.oetr_nn_match_abi_version() == hip_engine.NN_MATCH_ABI_VERSION == 1


def test_argument_types_are_declared():
    lib = pkg.load_library()
    for fn in hip_engine.HOMOGRAPHY_RANSAC_EXPORTS:
        f = getattr(lib, fn)
        assert f.argtypes is not None and len(f.argtypes) == parameter_count('oetr_homography_ransac.h', fn), fn
        assert f.restype is (ctypes.c_size_t if fn.endswith('workspace_bytes') else ctypes.c_int), fn
    at = lib.oetr_homography_ransac.argtypes
    assert len(at) == 21 and at[6] is ctypes.c_int64 and at[8] is ctypes.c_uint32 and at[9] is ctypes.c_double
    assert at[3] is at[7] is at[10] is at[12] is ctypes.c_int and at[14] is ctypes.c_size_t
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (3, 6, 7, 8, 9, 10, 12, 14))
    assert list(lib.oetr_homography_ransac_workspace_bytes.argtypes) == [ctypes.c_int, ctypes.c_int]


def test_workspace_bytes():
    ws = pkg.load_library().oetr_homography_ransac_workspace_bytes
    assert ws(0, 5) == 0 and ws(-4, 5) == 0 and ws(5, 0) == 0 and ws(5, -1) == 0
    assert ws(1, 1) == 9 * 8 + 4                                  # one model and its count
    assert ws(7, 600) == 7 * 600 * 76
    assert ws(INT32_MAX // 4096, 4096) == (INT32_MAX // 4096) * 4096 * 76       # no 32-bit overflow


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(b'\xa5' * 64, 64)   # host memory standing in for the device: never touched
    p = ctypes.addressof(keep)
    big = 1 << 62

    def call(params=p, offsets=p, pair_ids=p, n=2, k1=p, k2=p, m=5, n_hyp=8, seed=1, px_thr=3.0, refit=2,
             models_in=None, n_models_in=0, workspace=p, nbytes=big, model=p, H=p, corner_sq=p, counts=p, inliers=p):
        return lib.oetr_homography_ransac(params, offsets, pair_ids, n, k1, k2, m, n_hyp, seed, px_thr, refit,
                                          models_in, n_models_in, workspace, nbytes, model, H, corner_sq, counts,
                                          inliers, None)

    need = lib.oetr_homography_ransac_workspace_bytes(2, 8)
    for kw in (dict(params=None), dict(offsets=None), dict(model=None), dict(H=None), dict(corner_sq=None),
               dict(counts=None), dict(k1=None), dict(k2=None), dict(n=0), dict(n=-3), dict(m=-1), dict(m=-(1 << 63)),
               dict(n_hyp=0), dict(n_hyp=-1), dict(n_hyp=4097), dict(n_hyp=INT32_MAX),
               dict(models_in=p, n_models_in=0), dict(models_in=p, n_models_in=-2), dict(models_in=p, n_models_in=4097),
               dict(refit=-1), dict(refit=5), dict(refit=INT32_MAX),
               dict(px_thr=0.0), dict(px_thr=-1.0), dict(px_thr=float('nan')), dict(px_thr=float('inf')),
               dict(workspace=None), dict(nbytes=need - 1), dict(nbytes=0),
               dict(models_in=p, n_models_in=9, nbytes=need)):
        assert call(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_homography_ransac:'), kw
    for kw in (dict(m=1 << 31), dict(m=(1 << 63) - 1), dict(n=INT32_MAX // 8 + 1), dict(n=INT32_MAX, n_hyp=2),
               dict(n=INT32_MAX // 4096 + 1, models_in=p, n_models_in=4096)):
        assert call(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_homography_ransac:'), kw
    assert keep.raw == b'\xa5' * 64


def test_wrappers_refuse_before_any_device_use(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    k32 = np.zeros((8, 2), np.float32)
    P = np.zeros((1, 16))
    for k1, k2 in ((k32.astype(np.float64), k32), (k32, torch.zeros(8, 2, dtype=torch.float64))):
        with pytest.raises(ValueError, match='float64'):
            pkg.estimate_homographies(P, k1, k2, lengths=[8])
    with pytest.raises(ValueError, match='exactly one'):
        pkg.estimate_homographies(P, k32, k32, lengths=[8], offsets=torch.tensor([0, 8], dtype=torch.int32))
    with pytest.raises(ValueError, match='exactly one'):
        pkg.estimate_homographies(P, k32, k32)
    for n_hyp in (0, 4097):
        with pytest.raises(ValueError, match='n_hyp'):
            pkg.estimate_homographies(P, k32, k32, lengths=[8], n_hyp=n_hyp)
    for thr in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='px_thr'):
            pkg.estimate_homographies(P, k32, k32, lengths=[8], px_thr=thr)
    for models in (np.zeros((1, 0, 9)), np.zeros((1, 4097, 9)), np.zeros((1, 9))):
        with pytest.raises(ValueError, match='models must be'):
            pkg.estimate_homographies(P, k32, k32, lengths=[8], models=models)
    for refit in (-1, 5, 1.5):
        with pytest.raises(ValueError, match='refit_iters'):
            pkg.estimate_homographies(P, k32, k32, lengths=[8], refit_iters=refit)
    with pytest.raises(RuntimeError, match='There is no CPU implementation'):
        pkg.estimate_homographies(P, k32, k32, lengths=[8])
    for name in ('estimate_homographies', 'transfer_points', 'homography_errors', 'homography_auc',
                 'match_homography_auc'):
        assert name in pkg.__all__ and hasattr(pkg, name)
