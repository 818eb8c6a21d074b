"""CPU-only checks of the depth-map-set extension (``include/oetr_covis_set.h``,
``imagematching_oetr_amd/covis_set.py``, ``evaluate.evaluate_indexed``): header, export list and library
agree and the other four headers stand as they were; argument errors and workspace sizes are reported
without a GPU; there is no CPU route; the ``H1 x W1`` against ``H2 x W2`` restatement
(``tests/covis_set_oracle.py``) is ``covis_oracle.overlap_box`` on equal-size square sets and - where the
reference snapshot exists - the reference's ``numpy_overlap_box`` and ``scale_diff``; the pinned sets
(``tests/covis_set_expected.json``) are what the restatement computes and what the generator writes;
the shared scoring helper reproduces the pinned recall table."""
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
from imagematching_oetr_amd import covis_set, evaluate, hip_engine

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import covis_set_oracle as cso  # noqa: E402
from oracle import ref_snapshot  # noqa: E402

BAD_ARG, BAD_SHAPE = 1, 2
EXPECTED = json.loads((REPO / 'tests' / 'covis_set_expected.json').read_text())['sets']
needs_reference = pytest.mark.skipif(not ref_snapshot.available(),
                                     reason='needs the reference snapshot that build() places in oracle/_ref/')


def header_functions(name):
    text = (REPO / 'include' / name).read_text()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(oetr_[a-z_0-9]+)\s*\(', text)))


def draw(e):
    views, results = cso.checked_set(tuple(tuple(s) for s in e['sizes']), e['seed'])
    return views, results


# ------------------------------------------------------------------ header / exports / argument errors
def test_header_exports_library_and_versions_agree():
    lib = pkg.load_library()
    names = header_functions('oetr_covis_set.h')
    assert len(names) == 4 and set(names) == set(hip_engine.COVIS_SET_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/oetr_covis_set.h but not exported'
    assert lib.oetr_covis_set_abi_version() == hip_engine.COVIS_SET_ABI_VERSION == 1
    text = (REPO / 'include' / 'oetr_covis_set.h').read_text()
    assert re.search(r'#define\s+OETR_COVIS_SET_ABI_VERSION\s+1\b', text)
    assert 'departure' in text.lower() and 'NO MASKS' in text                  # both are said again
    # the other four headers keep their function counts, lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(header_functions('oetr_bank.h')) == 3
    assert len(header_functions('oetr_covis.h')) == 3 and len(header_functions('oetr_crop_batch.h')) == 3
    others = (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS) | set(hip_engine.COVIS_EXPORTS)
              | set(hip_engine.CROP_BATCH_EXPORTS))
    assert not set(hip_engine.COVIS_SET_EXPORTS) & others
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert lib.oetr_bank_abi_version() == hip_engine.BANK_ABI_VERSION == 1
    assert lib.oetr_covis_abi_version() == hip_engine.COVIS_ABI_VERSION == 1
    assert lib.oetr_crop_batch_abi_version() == hip_engine.CROP_BATCH_ABI_VERSION == 1
    assert re.search(r'#define\s+OETR_COVIS_MAX_SIDE\s+8192\b', (REPO / 'include' / 'oetr_covis.h').read_text())
    assert hip_engine.COVIS_MAX_SIDE == 8192


def test_map_table_mirror_is_16_bytes():
    assert ctypes.sizeof(hip_engine._CovisMap) == 16
    assert hip_engine._CovisMap.H.offset == 8 and hip_engine._CovisMap.W.offset == 12
    assert re.search(r'16 bytes', (REPO / 'include' / 'oetr_covis_set.h').read_text())


def test_workspace_bytes_need_no_gpu():
    lib = pkg.load_library()
    assert lib.oetr_covis_set_workspace_bytes(0) == 0 and lib.oetr_covis_set_workspace_bytes(-4) == 0
    one = lib.oetr_covis_set_workspace_bytes(1)
    assert one >= 9 * 4                                   # eight bounds and a count
    for n in (2, 8, 1024, 70000):
        assert lib.oetr_covis_set_workspace_bytes(n) == n * one


def test_argument_errors_need_no_gpu_and_touch_nothing():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(64)      # host memory standing in for device buffers: must never be touched
    p = ctypes.addressof(keep)
    big = 1 << 20

    def boxes(maps=p, n_maps=3, idx1=p, idx2=p, params=p, n=2, max_pixels=4096, ws=p, ws_bytes=big, box1=p, box2=p,
              valid=p, count=p):
        return lib.oetr_covis_boxes_indexed(maps, n_maps, idx1, idx2, params, n, max_pixels, ws, ws_bytes, box1, box2,
                                            valid, count, None)

    for kw in (dict(maps=None), dict(idx1=None), dict(idx2=None), dict(params=None), dict(ws=None), dict(box1=None),
               dict(box2=None), dict(valid=None), dict(n=0), dict(n=-2), dict(n_maps=0), dict(n_maps=-1),
               dict(ws_bytes=0), dict(ws_bytes=lib.oetr_covis_set_workspace_bytes(2) - 1)):
        assert boxes(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_covis_boxes_indexed'), kw
    for kw in (dict(max_pixels=0), dict(max_pixels=-5), dict(max_pixels=8192 * 8192 + 1), dict(max_pixels=1 << 40)):
        assert boxes(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_covis_boxes_indexed'), kw

    def select(box1=p, box2=p, valid=p, n=2, thr=2.0, limit=0, kept=p, n_kept=p, sd=p):
        return lib.oetr_covis_select(box1, box2, valid, n, thr, limit, kept, n_kept, sd, None, 0, None)

    for kw in (dict(box1=None), dict(box2=None), dict(valid=None), dict(kept=None), dict(n_kept=None), dict(n=0),
               dict(n=-1), dict(thr=float('nan'))):
        assert select(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_covis_select'), kw
    assert keep.raw == b'\0' * 64


def test_there_is_no_cpu_route(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.DepthSet()
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.DepthSet('cpu')
    with pytest.raises(RuntimeError, match='GPU'):
        covis_set.select_pairs(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, dtype=torch.bool))
    for name in ('DepthSet', 'overlap_boxes_indexed', 'mine_pairs', 'evaluate_indexed'):
        assert name in pkg.__all__ and hasattr(pkg, name)


# ------------------------------------------------------------------ the restatement
def test_restatement_equals_covis_oracle_on_equal_size_square_sets():
    for size, seed in ((56, 5), (40, 6)):
        views, results = cso.checked_set(((size, size),) * 3, seed)
        assert len(results) == 6
        for (i, j), mine in results.items():
            theirs = cvo.restate(cso.as_scene(views, i, j))
            for k in ('box1', 'box2'):
                assert np.array_equal(mine[k], theirs[k]), (i, j, k)
            assert (mine['valid'], mine['count'], mine['margin']) == (theirs['valid'], theirs['count'], theirs['margin'])


def test_restatement_uses_each_maps_own_size():
    """Box 1 lives in map 1's extent and box 2 in map 2's, and the pinned mixed set has pairs where a wrong
    extent would show: source columns / rows beyond map 2's and landing columns / rows beyond map 1's."""
    views, results = cso.checked_set(cso.SIZES, 0)
    seen = set()
    for (i, j), r in results.items():
        if not r['valid']:
            continue
        (h1, w1), (h2, w2) = cso.SIZES[i], cso.SIZES[j]
        assert 0 <= r['box1'][0] <= r['box1'][2] < w1 and 0 <= r['box1'][1] <= r['box1'][3] < h1, (i, j)
        assert 0 <= r['box2'][0] <= r['box2'][2] < w2 and 0 <= r['box2'][1] <= r['box2'][3] < h2, (i, j)
        seen |= {name for name, hit in (('source column >= W2', r['box1'][2] >= w2), ('source row >= H2', r['box1'][3] >= h2),
                                        ('landing column >= W1', r['box2'][2] >= w1), ('landing row >= H1', r['box2'][3] >= h1))
                 if hit}
    assert len(seen) == 4, seen


def test_scale_diff_and_keep_follow_pythons_max():
    assert cso.scale_diff([0, 0, 40, 10], [0, 0, 20, 10]) == 2.0
    assert not cso.keep([0, 0, 40, 10], [0, 0, 20, 10], True)                # exactly 2 is not kept
    assert cso.keep([0, 0, 41, 10], [0, 0, 20, 10], True) and not cso.keep([0, 0, 41, 10], [0, 0, 20, 10], False)
    assert cso.scale_diff([5, 0, 5, 10], [0, 0, 20, 10]) == np.inf           # zero width: 0 / 20, then 20 / 0
    assert np.isnan(cso.scale_diff([5, 0, 5, 10], [3, 0, 3, 10]))             # 0 / 0 first: NaN stays
    assert np.isnan(cso.scale_diff([0, 0, 0, 0], [0, 0, 0, 0])) and not cso.keep([0] * 4, [0] * 4, False)
    # a NaN width ratio hides a large height ratio: max(nan, x) is nan in Python
    assert np.isnan(cso.scale_diff([5, 0, 5, 90], [3, 0, 3, 10])) and not cso.keep([5, 0, 5, 90], [3, 0, 3, 10], True)
    kept, n, sd = cso.select([[0, 0, 41, 10], [0, 0, 40, 10], [0, 0, 9, 30]], [[0, 0, 20, 10]] * 3, [True] * 3, limit=1)
    assert list(kept) == [0, -1, -1] and n == 1 and sd[1] == 2.0 and sd[2] == 3.0


@needs_reference
def test_restatement_equals_the_reference_on_an_equal_size_square_set():
    before = {n: sys.modules.get(n) for n in ('cv2', 'h5py', 'src', 'src.datasets.utils')}
    numpy_overlap_box, ref_scale_diff = cso.load_reference(ref_snapshot.DEST)
    assert {n: sys.modules.get(n) for n in before} == before               # the stand-ins are gone again
    views, results = cso.checked_set(((56, 56),) * 4, 5)
    for (i, j), mine in results.items():
        theirs = cso.reference_pair(numpy_overlap_box, views, i, j)
        assert np.array_equal(theirs['box1'], mine['box1']) and np.array_equal(theirs['box2'], mine['box2']), (i, j)
        assert (theirs['valid'], theirs['count']) == (mine['valid'], mine['count']), (i, j)
        with np.errstate(all='ignore'):
            sd = ref_scale_diff(theirs['box1'], theirs['box2'], None, None)
        assert repr(float(sd)) == repr(float(cso.scale_diff(mine['box1'], mine['box2'])))
    with np.errstate(all='ignore'):       # the degenerate boxes too
        for b1, b2 in (([5, 0, 5, 10], [0, 0, 20, 10]), ([5, 0, 5, 10], [3, 0, 3, 10]), ([0, 0, 40, 10], [0, 0, 20, 10])):
            assert repr(float(ref_scale_diff(np.array(b1), np.array(b2), None, None))) == repr(float(cso.scale_diff(b1, b2)))


# ------------------------------------------------------------------ the pinned sets
def test_pinned_sets_cover_what_they_are_for():
    by_name = {e['name']: e for e in EXPECTED}
    mixed = by_name['mixed']
    assert [tuple(s) for s in mixed['sizes']] == list(cso.SIZES) and len(mixed['pairs']) == 30
    assert 0 < sum(mixed['valid']) < 30 and 0 < len(mixed['kept']) < sum(mixed['valid'])
    away = [k for k, p in enumerate(mixed['pairs']) if cso.AWAY_VIEW in p]
    assert not any(mixed['valid'][k] for k in away)
    assert all(cso.ZOOM_VIEW in mixed['pairs'][k] for k in mixed['kept'])
    square = by_name['square']
    assert len({tuple(s) for s in square['sizes']}) == 1 and all(square['valid'])


@pytest.mark.parametrize('e', EXPECTED, ids=lambda e: e['name'])
def test_restatement_equals_the_recorded_results(e):
    views, results = draw(e)
    assert min(r['margin'] for r in results.values()) >= cso.MIN_MARGIN
    rec = cso.set_record(views, results, e['min_scale_diff'])
    assert rec == {k: e[k] for k in rec}


def test_expected_file_is_regenerated_bit_for_bit(tmp_path):
    """``tools/gen_golden_covis_set.py`` (which asserts reference == restatement where the snapshot exists) writes
    the committed file again."""
    proc = subprocess.run([sys.executable, str(REPO / 'tools' / 'gen_golden_covis_set.py'), '--out', str(tmp_path / 'e.json')],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert (tmp_path / 'e.json').read_text() == (REPO / 'tests' / 'covis_set_expected.json').read_text()


# ------------------------------------------------------------------ the scoring tail
@pytest.mark.parametrize('oiou', [False, True])
def test_scoring_helper_reproduces_the_pinned_recall_table(oiou):
    rec = json.loads((REPO / 'tests' / 'covis_expected.json').read_text())['recalls']
    name = 'oiou' if oiou else 'iou'
    gt, pred = (torch.from_numpy(a) for a in cvo.recall_table())
    whole = evaluate.score_boxes([(gt[0], gt[1], None, pred[0], pred[1])], rec['thrs'], oiou)
    parts = evaluate.score_boxes([(gt[0, :7], gt[1, :7], None, pred[0, :7], pred[1, :7]),
                                  (gt[0, 7:], gt[1, 7:], None, pred[0, 7:], pred[1, 7:])], rec['thrs'], oiou)
    for res in (whole, parts):
        assert list(res['recalls']) == rec[f'{name}_recalls']
        assert res['n'] == 48 and res['n_valid_pairs'] == 21
        assert res['mean_iou'] == pytest.approx(rec[f'{name}_nansum'] / 48, rel=1e-12)
    valid = torch.zeros(24, dtype=torch.bool)
    valid[:5] = True                                                       # a ground truth that carries its own flags
    assert evaluate.score_boxes([(gt[0], gt[1], valid, pred[0], pred[1])], rec['thrs'], oiou)['n_valid_pairs'] == 5
    assert evaluate.score_boxes([], rec['thrs'], oiou)['n'] == 0
    assert pkg.evaluate_indexed(None, [], None, [])['n'] == 0             # an empty list touches nothing


def test_evaluate_indexed_wants_one_depth_map_per_image():
    class FourMaps:
        def __len__(self):
            return 4
    with pytest.raises(ValueError, match='slot k'):
        pkg.evaluate_indexed(None, [torch.zeros(8, 8, 3)] * 3, FourMaps(), [(0, 1)])
