"""CPU-only checks of the co-visibility extension (``include/oetr_covis.h``,
``imagematching_oetr_amd/covis.py``, ``imagematching_oetr_amd/evaluate.py``): the pinned scenes
(``tests/covis_expected.json``: recipes, input hashes, recorded results) are what the float64
restatement computes and - where the reference is present - what the reference computes; header,
export list and library agree; argument errors are reported without a GPU; the evaluator's counting
equals the reference's ``_recalls``; there is no CPU route."""
import ctypes
import importlib.util
import json
import logging
import re
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd import hip_engine

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
from oracle import ref_snapshot  # noqa: E402

BAD_ARG, BAD_SHAPE = 1, 2
EXPECTED = json.loads((REPO / 'tests' / 'covis_expected.json').read_text())
SCENES = EXPECTED['scenes']
scene_id = lambda e: f"{e['kind']}_{e['size']}_s{e['seed']}"
needs_reference = pytest.mark.skipif(not ref_snapshot.available(),
                                     reason='needs the reference snapshot that build() places in oracle/_ref/')


def draw(e):
    """A pinned scene from its recipe; the inputs are the recorded ones, bit for bit."""
    scene, res = cvo.checked_scene(e['kind'], e['size'], e['size'], e['seed'])
    assert scene['depth1'].dtype == np.float32 and scene['depth1'].shape == (e['size'], e['size'])   # square: parity claimed
    assert cvo.sha(scene['depth1']) == e['depth1_sha256'] and cvo.sha(scene['depth2']) == e['depth2_sha256']
    return scene, res


def test_pinned_scene_set():
    assert len(SCENES) == 6
    assert {e['kind'] for e in SCENES} == set(cvo.KINDS)
    assert all(96 <= e['size'] <= 320 for e in SCENES)


@pytest.mark.parametrize('e', SCENES, ids=scene_id)
def test_restatement_equals_the_recorded_results(e):
    scene, res = draw(e)
    assert res['margin'] >= cvo.MIN_MARGIN
    assert cvo.result_record(res) == {k: e[k] for k in cvo.result_record(res)}
    assert int(res['mask1'].sum()) == e['count']


@needs_reference
@pytest.mark.parametrize('e', SCENES, ids=scene_id)
def test_reference_equals_the_recorded_results(e):
    """The reference's own ``numpy_overlap_box`` (from the snapshot), on float64 copies of the inputs."""
    for n in ('cv2', 'h5py'):
        sys.modules.setdefault(n, types.ModuleType(n))
    spec = importlib.util.spec_from_file_location('ref_datasets_utils', ref_snapshot.DEST / 'src' / 'datasets' / 'utils.py')
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)
    scene, _ = draw(e)
    with np.errstate(all='ignore'):
        box1, mask1, box2, mask2, valid = utils.numpy_overlap_box(*cvo.scene_args(scene))
    theirs = dict(box1=np.asarray(box1, np.int64), box2=np.asarray(box2, np.int64), valid=bool(valid),
                  count=int((mask1 != 0).sum()), mask1=(mask1 != 0).astype(np.uint8), mask2=(mask2 != 0).astype(np.uint8))
    assert cvo.result_record(theirs) == {k: e[k] for k in cvo.result_record(theirs)}


def test_pinned_scenes_cover_what_they_are_for():
    by_kind = {e['kind']: e for e in SCENES}
    assert by_kind['plane']['valid'] and by_kind['plane']['count'] > 1000
    assert not by_kind['no_overlap']['valid'] and not any(by_kind['no_overlap']['box1'])
    assert not by_kind['behind']['valid']
    # truncation towards zero: source column 0 / row 0 land at u2 = -0.3 / v2 = -0.4 and are INLIERS
    scene, res = draw(by_kind['trunc'])
    assert by_kind['trunc']['box1'][:2] == [0, 0] and res['mask1'][:, 0].any() and res['mask1'][0, :].any()
    # holes in both maps
    scene, _ = draw(by_kind['plane'])
    assert (scene['depth1'] == 0).any() and (scene['depth2'] == 0).any()


def test_a_perturbed_transform_changes_nothing():
    """What the margin is for: T with a relative error of 1e-13 (another inverse, another sum order)
    gives the same integers."""
    for e in SCENES:
        scene, _ = draw(e)
        T = (scene['pose2'] @ np.linalg.inv(scene['pose1'])) * (1 + 1e-13)
        res = cvo.overlap_box(*cvo.scene_args(scene), T=T)
        assert cvo.result_record(res) == {k: e[k] for k in cvo.result_record(res)}


@needs_reference
def test_expected_file_is_regenerated_bit_for_bit(tmp_path):
    """``tools/gen_golden_covis.py`` (which asserts reference == restatement for scenes, masks and recalls)
    writes the committed file again."""
    proc = subprocess.run([sys.executable, str(REPO / 'tools' / 'gen_golden_covis.py'), '--out', str(tmp_path / 'e.json')],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert (tmp_path / 'e.json').read_text() == (REPO / 'tests' / 'covis_expected.json').read_text()


# ------------------------------------------------------------------ header / exports / argument errors
def header_functions(name):
    text = (REPO / 'include' / name).read_text()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(oetr_[a-z_0-9]+)\s*\(', text)))


def test_covis_header_exports_and_library_agree():
    lib = pkg.load_library()
    names = header_functions('oetr_covis.h')
    assert len(names) == 3, names
    assert set(names) == set(hip_engine.COVIS_EXPORTS)
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/oetr_covis.h but not exported'
    assert lib.oetr_covis_abi_version() == hip_engine.COVIS_ABI_VERSION == 1
    text = (REPO / 'include' / 'oetr_covis.h').read_text()
    assert re.search(r'#define\s+OETR_COVIS_ABI_VERSION\s+1\b', text)
    assert re.search(r'#define\s+OETR_COVIS_PARAM_DOUBLES\s+40\b', text)
    assert hip_engine.COVIS_PARAM_DOUBLES == cvo.PARAM_DOUBLES == 40
    # the extension stays out of the base header, the bank's, and their export lists and versions
    assert len(header_functions('oetr_hip.h')) == 53 and len(header_functions('oetr_bank.h')) == 3
    assert not set(hip_engine.COVIS_EXPORTS) & (set(hip_engine.EXPORTS) | set(hip_engine.BANK_EXPORTS))
    assert lib.oetr_abi_version() == hip_engine.ABI_VERSION == 6
    assert 'departed' in text.lower() or 'departure' in text.lower()      # the non-square rule is named


def test_covis_workspace_bytes_needs_no_gpu():
    lib = pkg.load_library()
    assert lib.oetr_covis_workspace_bytes(0) == 0 and lib.oetr_covis_workspace_bytes(-4) == 0
    one = lib.oetr_covis_workspace_bytes(1)
    assert one >= 9 * 4                                   # eight bounds and a count
    for n in (2, 8, 32, 1000):
        assert lib.oetr_covis_workspace_bytes(n) == n * one


def test_covis_argument_errors_need_no_gpu():
    lib = pkg.load_library()
    keep = ctypes.create_string_buffer(64)      # host memory standing in for device buffers: must never be touched
    p = ctypes.addressof(keep)
    big = 1 << 20

    def call(d1=p, d2=p, params=p, n=2, H=64, W=64, ws=p, ws_bytes=big, box1=p, box2=p, valid=p, count=p,
             m1=None, m2=None):
        return lib.oetr_covis_boxes(d1, d2, params, n, H, W, ws, ws_bytes, box1, box2, valid, count, m1, m2, None)

    for kw in (dict(d1=None), dict(d2=None), dict(params=None), dict(ws=None), dict(box1=None), dict(box2=None),
               dict(valid=None), dict(n=0), dict(n=-2), dict(m1=p), dict(m2=p), dict(ws_bytes=0),
               dict(ws_bytes=lib.oetr_covis_workspace_bytes(2) - 1)):
        assert call(**kw) == BAD_ARG, kw
        assert lib.oetr_last_error().startswith(b'oetr_covis_boxes'), kw
    for kw in (dict(H=0), dict(W=0), dict(H=-1), dict(H=8193), dict(W=8193), dict(W=1 << 30)):
        assert call(**kw) == BAD_SHAPE, kw
        assert lib.oetr_last_error().startswith(b'oetr_covis_boxes'), kw
    assert keep.raw == b'\0' * 64


def _cpu_batch(n=2, size=16):
    eye4, eye3 = torch.eye(4).repeat(n, 1, 1), torch.eye(3).repeat(n, 1, 1)
    side = dict(depth=torch.ones(n, size, size), intrinsics=eye3, pose=eye4, bbox=torch.zeros(n, 2), ratio=torch.ones(n, 2))
    return {f'{k}{s}': v for s in (1, 2) for k, v in side.items()}


def test_python_entry_has_no_cpu_route(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the same answer on a GPU machine
    b = _cpu_batch()
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.overlap_boxes_from_batch(b)
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.overlap_boxes_from_depth(b['depth1'], b['intrinsics1'], b['pose1'], b['bbox1'], b['ratio1'],
                                     b['depth2'], b['intrinsics2'], b['pose2'], b['bbox2'], b['ratio2'], masks=True)


def test_python_entry_checks_its_batch():
    b = _cpu_batch()
    del b['pose2']
    with pytest.raises(KeyError, match='pose2'):
        pkg.overlap_boxes_from_batch(b)
    from imagematching_oetr_amd.covis import covis_boxes, covis_params
    b = _cpu_batch(3)
    params = covis_params(*(b[f'{k}{s}'] for s in (1, 2) for k in ('intrinsics', 'pose', 'bbox', 'ratio')))
    assert params.shape == (3, 40) and params.dtype == torch.float64
    row = params[0].numpy()
    assert np.array_equal(row[:16].reshape(4, 4), np.eye(4)) and np.array_equal(row[20:29].reshape(3, 3), np.eye(3))
    assert list(row[16:20]) == [1, 1, 0, 0] and list(row[29:37]) == [0, 0, 1, 1, 0, 0, 1, 1]
    with pytest.raises(RuntimeError, match='GPU'):
        covis_boxes(b['depth1'], b['depth2'], params)


def test_param_block_layout_matches_the_test_side_one():
    """``covis_params`` (torch) and ``covis_oracle.param_block`` (numpy) build the same block, up to the
    last bits of the 4 x 4 inverse."""
    from imagematching_oetr_amd.covis import covis_params
    g, _ = draw(SCENES[1])
    t = lambda k: torch.from_numpy(g[k])[None]
    mine = covis_params(t('intrinsics1'), t('pose1'), t('bbox1'), t('ratio1'), t('intrinsics2'), t('pose2'),
                        t('bbox2'), t('ratio2'))[0].numpy()
    theirs = cvo.param_block(g)
    assert np.array_equal(mine[16:], theirs[16:])
    assert np.allclose(mine[:16], theirs[:16], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ evaluate_dummy's counting on a stand-in model
class StubModel:
    """``forward_dummy`` returning fixed boxes, batch after batch, with OETR's deferred-check contract:
    a batch's boxes are garbage until ``hip_flush()`` settles them in place."""

    def __init__(self, pred1, pred2, batch):
        self.pred1, self.pred2, self.batch, self.at, self._pending, self.flushes = pred1, pred2, batch, 0, [], 0

    def hip_flush(self):
        self.flushes += 1
        for t, good in self._pending:
            t.copy_(good)
        self._pending = []

    def forward_dummy(self, image1, image2):
        n = image1.shape[0]
        assert image2.shape[0] == n and image1.shape[-1] == 3
        good = (self.pred1[self.at:self.at + n], self.pred2[self.at:self.at + n])
        self.at += n
        out = tuple(torch.full_like(t, 7.0e4) for t in good)
        self._pending += list(zip(out, good))                 # settled at the flush only
        return out


def _table():
    gt, pred = cvo.recall_table()
    return dict(gt1=gt[0], gt2=gt[1], pred1=pred[0], pred2=pred[1])


def _eval_batches(g, sizes, with_boxes=True):
    at = 0
    for n in sizes:
        b = {'image1': torch.rand(n, 8, 8, 3), 'image2': torch.rand(n, 8, 8, 3)}
        if with_boxes:
            b['overlap_box1'] = torch.from_numpy(g['gt1'][at:at + n])
            b['overlap_box2'] = torch.from_numpy(g['gt2'][at:at + n])
        at += n
        yield b


@pytest.mark.parametrize('oiou', [False, True])
@pytest.mark.parametrize('sizes', [(24,), (5, 8, 1, 10)])
def test_evaluate_dummy_counts_as_the_reference(oiou, sizes):
    g, rec = _table(), EXPECTED['recalls']
    name = 'oiou' if oiou else 'iou'
    model = StubModel(torch.from_numpy(g['pred1']), torch.from_numpy(g['pred2']), sizes)
    for gt in ('auto', 'batch'):
        model.at = 0
        res = pkg.evaluate_dummy(model, _eval_batches(g, sizes), oiou=oiou, gt=gt)
        assert np.array_equal(res['recalls'], np.array(rec[f'{name}_recalls'])), (res['recalls'], rec[f'{name}_recalls'])
        assert res['n'] == 48 and res['n_valid_pairs'] == 21            # three pairs have a zero ground-truth box
        assert res['mean_iou'] == pytest.approx(rec[f'{name}_nansum'] / 48, rel=1e-12)
    assert model.flushes == 2                                           # once per evaluation, at the end
    assert rec['thrs'] == list(np.arange(0.5, 0.96, 0.05))
    assert rec['iou_recalls'][0] > rec['iou_recalls'][5] > rec['iou_recalls'][8] > 0    # the table discriminates
    # the recorded recalls are the test-side formula's too (the generator asserts they are the reference's)
    gt, pred = cvo.recall_table()
    assert list(cvo.recalls(cvo.box_scores(gt, pred, oiou), rec['thrs'])) == rec[f'{name}_recalls']


def test_evaluate_dummy_logs_the_reference_table_and_checks_arguments(caplog):
    g, rec = _table(), EXPECTED['recalls']
    model = StubModel(torch.from_numpy(g['pred1']), torch.from_numpy(g['pred2']), (24,))
    with caplog.at_level(logging.INFO, logger='covis-test'):
        res = pkg.evaluate_dummy(model, _eval_batches(g, (24,)), logger=logging.getLogger('covis-test'))
    r = res['recalls']
    assert 'Recalls\t R0.5\t R0.75\t R0.9\t' in caplog.text
    assert 'Values\t {:.5f}\t {:.5f}\t {:.5f}\t'.format(r[0], r[5], r[8]) in caplog.text
    with pytest.raises(ValueError):
        pkg.evaluate_dummy(model, [], gt='poses')
    model.at = 0
    with pytest.raises(KeyError):
        pkg.evaluate_dummy(model, _eval_batches(g, (24,), with_boxes=False), gt='batch')
    assert pkg.evaluate_dummy(model, [])['n'] == 0
    # two thresholds only: no table, the two recalls
    model.at = 0
    two = pkg.evaluate_dummy(model, _eval_batches(g, (24,)), iou_thrs=np.array(rec['thrs'])[[0, 5]])
    assert list(two['recalls']) == [r[0], r[5]]
