"""CPU-only checks of the keypoint-selection extension's ABI (``include/oetr_keypoint_select.h``,
``csrc/keypoint_select.hip``, ``imagematching_oetr_amd/keypoint_select.py``): header, export list and library agree and
the other lists stand as they were; argument types are declared; the record's layout is the header's; every
host-checked argument error is reported without a GPU and touches nothing; the wrapper refuses before any device
use."""
import ctypes
import re
import sys
from pathlib import Path

import pytest
import torch

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd import hip_engine, keypoint_select

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import keypoint_select_oracle as kso  # noqa: E402

HEADER = 'oetr_keypoint_select.h'
BAD_ARG, BAD_SHAPE, WORKSPACE = 1, 2, 4


def header_text(name):
    text = (REPO / 'include' / name).read_text()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def header_functions(name):
    return sorted(set(re.findall(r'\b(oetr_[a-z_0-9]+)\s*\(', header_text(name))))


def parameter_count(name, fn):
    args = re.search(r'\b' + fn + r'\s*\(([^)]*)\)', header_text(name)).group(1).strip()
    return 0 if args == 'void' else len(args.split(','))


def test_header_exports_library_and_versions_agree():
    lib = pkg.load_library()
    names = header_functions(HEADER)
    assert len(names) == 3 and set(names) == set(hip_engine.KEYPOINT_SELECT_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/{HEADER} but not exported'
    assert lib.oetr_keypoint_select_abi_version() == hip_engine.KEYPOINT_SELECT_ABI_VERSION == 1
    text = (REPO / 'include' / HEADER).read_text()
    for macro, value in (('ABI_VERSION', 1), ('COUNTERS', hip_engine.KEYPOINT_SELECT_COUNTERS),
                         ('MAX_RADIUS', hip_engine.KEYPOINT_SELECT_MAX_RADIUS),
                         ('MAX_KEYPOINTS', hip_engine.KEYPOINT_SELECT_MAX_KEYPOINTS),
                         ('MIN_D', hip_engine.KEYPOINT_SELECT_MIN_D), ('MAX_D', hip_engine.KEYPOINT_SELECT_MAX_D),
                         ('MAX_SIDE', hip_engine.KEYPOINT_SELECT_MAX_SIDE),
                         ('PIXEL_ALIGN', hip_engine.KEYPOINT_SELECT_PIXEL_ALIGN)):
        assert re.search(r'#define\s+OETR_KEYPOINT_SELECT_%s\s+%d\b' % (macro, value), text), macro
    assert (hip_engine.KEYPOINT_SELECT_COUNTERS, hip_engine.KEYPOINT_SELECT_MAX_RADIUS,
            hip_engine.KEYPOINT_SELECT_MAX_KEYPOINTS) == (kso.COUNTERS, kso.MAX_RADIUS, kso.MAX_KEYPOINTS) == (2, 8, 4096)
    # the other headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(header_functions('oetr_match_assembly.h')) == 3
    assert len(header_functions('oetr_nn_match.h')) == 3 and len(header_functions('oetr_crop_batch.h')) == 3
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.COVIS_SET_EXPORTS) | set(hip_engine.CROP_BATCH_EXPORTS)
              | set(hip_engine.MATCH_SCORE_EXPORTS) | set(hip_engine.KEYPOINT_SCORE_EXPORTS)
              | set(hip_engine.MATCH_ASSEMBLY_EXPORTS) | set(hip_engine.HOMOGRAPHY_EXPORTS)
              | set(hip_engine.POSE_RANSAC_EXPORTS) | set(hip_engine.NN_MATCH_EXPORTS)
              | set(hip_engine.HOMOGRAPHY_RANSAC_EXPORTS) | set(hip_engine.POSE_REFIT_EXPORTS))
    assert not set(hip_engine.KEYPOINT_SELECT_EXPORTS) & others
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_nn_match_abi_version() == hip_engine.NN_MATCH_ABI_VERSION == 1
    assert lib.oetr_match_assembly_abi_version() == hip_engine.MATCH_ASSEMBLY_ABI_VERSION == 1
    for name in ('keypoint_map_table', 'select_keypoints', 'keypoint_counts'):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_argument_types_and_the_record_are_declared():
    lib = pkg.load_library()
    for fn in hip_engine.KEYPOINT_SELECT_EXPORTS:
        f = getattr(lib, fn)
        assert f.argtypes is not None and len(f.argtypes) == parameter_count(HEADER, fn), fn
    assert lib.oetr_keypoint_select.restype is ctypes.c_int
    assert lib.oetr_keypoint_select_workspace_bytes.restype is ctypes.c_size_t
    at = lib.oetr_keypoint_select.argtypes
    assert len(at) == 18 and at[2] is at[3] is ctypes.c_int64 and at[6] is ctypes.c_float and at[11] is ctypes.c_size_t
    assert all(at[k] is ctypes.c_int for k in (1, 4, 5, 7, 8, 9))
    assert all(t is ctypes.c_void_p for k, t in enumerate(at) if k not in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11))
    # the record: the header's fields in the header's order, 72 bytes
    body = re.search(r'typedef struct oetr_keypoint_map \{(.*?)\} oetr_keypoint_map;', header_text(HEADER), re.S).group(1)
    fields = re.findall(r'\b\*?([A-Za-z_]+)(?:\[\d\])?\s*[,;]', body)
    assert fields == ['scores', 'H', 'W', 'score_stride', 'desc', 'h', 'w', 'desc_stride', 'pixel_offset'], fields
    M = hip_engine._KeypointMap
    assert [f[0] for f in M._fields_] == fields and ctypes.sizeof(M) == 72
    assert (M.scores.offset, M.H.offset, M.W.offset, M.score_stride.offset, M.desc.offset, M.h.offset, M.w.offset,
            M.desc_stride.offset, M.pixel_offset.offset) == (0, 8, 12, 16, 24, 32, 36, 40, 64)
    ws = lib.oetr_keypoint_select_workspace_bytes
    assert ws(0, 1, 1) == ws(-5, 1, 1) == ws(100, 0, 1) == ws(100, 1, 0) == ws(100, 1, 4097) == ws(2 ** 40 + 1, 1, 1) == 0
    assert ws(2 ** 20, 2 ** 20, 4096) == 0                          # more than 2^31 - 1 rows of capacity
    assert ws(1000, 2, 16) >= 7 * 1000 + 4 * 2 * 16 and ws(64 * 307200, 64, 2048) >= 7 * 64 * 307200


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(b'\xa5' * 80, 80)   # host memory standing in for the device: never touched
    p = (ctypes.addressof(keep) + 15) // 16 * 16           # 16-byte aligned, 64 bytes behind it

    def call(maps=p, n=3, max_pixels=480 * 640, total=3 * 480 * 640, D=256, r=4, thr=0.005, border=4, k=2048, cell=8,
             ws=p, ws_bytes=1 << 30, keypoints=p, scores=p, descriptors=p, offsets=p, counts=p):
        return lib.oetr_keypoint_select(maps, n, max_pixels, total, D, r, thr, border, k, cell, ws, ws_bytes, keypoints,
                                        scores, descriptors, offsets, counts, None)

    bad = [{k: None} for k in ('maps', 'ws', 'keypoints', 'scores', 'descriptors', 'offsets', 'counts')]
    bad += [dict(n=0), dict(n=-2), dict(max_pixels=0), dict(total=0), dict(total=-(1 << 63)), dict(D=0), dict(D=2),
            dict(D=-4), dict(D=130), dict(D=516), dict(D=1024), dict(r=-1), dict(r=9), dict(thr=-1e-9),
            dict(thr=float('nan')), dict(thr=-float('inf')), dict(border=-1), dict(k=0), dict(k=-1), dict(k=4097),
            dict(cell=0), dict(cell=-8), dict(maps=p + 4), dict(keypoints=p + 4), dict(scores=p + 2),
            dict(descriptors=p + 1), dict(offsets=p + 2), dict(counts=p + 3), dict(ws=p + 1)]
    for kw in bad:
        assert call(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_keypoint_select'), kw
    for kw in (dict(max_pixels=8192 * 8192 + 1), dict(max_pixels=(1 << 63) - 1), dict(total=(1 << 40) + 1),
               dict(n=(1 << 31) - 1), dict(n=(1 << 21) + 1, k=1), dict(n=1 << 20, k=2048)):
        assert call(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_keypoint_select'), kw
    need = lib.oetr_keypoint_select_workspace_bytes(3 * 480 * 640, 3, 2048)
    for kw in (dict(ws_bytes=0), dict(ws_bytes=15), dict(ws_bytes=need - 1)):
        assert call(**kw) == WORKSPACE, kw
        assert lib.oetr_last_error().startswith(b'oetr_keypoint_select'), kw
    assert keep.raw == b'\xa5' * 80


def test_the_wrapper_refuses_before_any_device_use(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    S, F = torch.zeros(12, 16), torch.zeros(8, 3, 4)
    with pytest.raises(ValueError, match='float64'):
        pkg.keypoint_map_table([S.double()], [F])
    with pytest.raises(ValueError, match='float64'):
        pkg.keypoint_map_table([S], [F.double()])
    with pytest.raises(ValueError, match='float32'):
        pkg.keypoint_map_table([S.half()], [F])
    for D in (2, 6, 130, 516):
        with pytest.raises(ValueError, match='D % 4 == 0'):
            pkg.keypoint_map_table([S], [torch.zeros(D, 3, 4)])
    with pytest.raises(ValueError, match='channels'):
        pkg.keypoint_map_table([S, S], [F, torch.zeros(12, 3, 4)])
    with pytest.raises(ValueError, match='one score map and one descriptor map per image'):
        pkg.keypoint_map_table([S, S], [F])
    with pytest.raises(ValueError, match='dimensions'):
        pkg.keypoint_map_table([S[0]], [F])
    with pytest.raises(ValueError, match='ONE GPU'):                # maps on different devices
        pkg.keypoint_map_table([S], [F.to('meta')])
    with pytest.raises(RuntimeError, match='GPU.*no CPU implementation'):
        pkg.keypoint_map_table([S], [F])
    table = object()
    for kw, what in ((dict(max_keypoints=0), 'max_keypoints'), (dict(max_keypoints=4097), 'max_keypoints'),
                     (dict(max_keypoints=-1), 'max_keypoints'), (dict(), 'max_keypoints'),
                     (dict(max_keypoints=8, nms_radius=9), 'nms_radius'), (dict(max_keypoints=8, nms_radius=-1), 'nms_radius'),
                     (dict(max_keypoints=8, threshold=-0.001), 'threshold'),
                     (dict(max_keypoints=8, threshold=float('nan')), 'threshold'),
                     (dict(max_keypoints=8, remove_borders=-1), 'remove_borders'), (dict(max_keypoints=8, cell=0), 'cell')):
        with pytest.raises(ValueError, match=what):
            pkg.select_keypoints(table, **kw)
    with pytest.raises(ValueError, match='keypoint_map_table'):
        pkg.select_keypoints(table, max_keypoints=8)
    # host inputs inside a capture: refused by name before anything is uploaded
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: __import__('contextlib').nullcontext())
    with pytest.raises(ValueError, match=r"inside a graph capture.*\['descriptors', 'scores'\]"):
        pkg.keypoint_map_table([S], [F])
    from imagematching_oetr_amd.dloc_extractor import DenseExtractor
    assert DenseExtractor.required_inputs == ['image'] and DenseExtractor.default_conf['nms_radius'] == 4
    assert DenseExtractor.default_conf['keypoint_threshold'] == 0.005 and DenseExtractor.default_conf['remove_borders'] == 4
    with pytest.raises(ValueError, match='net'):
        DenseExtractor({})
    assert DenseExtractor({'max_keypoints': 7}, net=torch.nn.Identity()).conf['max_keypoints'] == 7
    assert keypoint_select.KeypointMapTable is not None
