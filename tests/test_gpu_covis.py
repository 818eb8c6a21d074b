"""GPU tests of the co-visibility boxes (``oetr_covis_boxes``, ``csrc/covis.hip``) and of
``evaluate_dummy``: the pinned scenes of ``tests/covis_expected.json`` (recorded results that the
reference's ``numpy_overlap_box`` gives as well: ``tools/gen_golden_covis.py``, ``tests/test_covis_cpu.py``) and
generated scenes restated in float64 numpy (``tests/covis_oracle.py``) are reproduced EXACTLY - boxes, valid,
count and masks are integers, and every scene's decision margin is >= 1e-9 (asserted where the scene
is drawn; none is left out)."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
from oracle import oetr_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
PINNED = json.loads((REPO / 'tests' / 'covis_expected.json').read_text())['scenes']
SIDES = ('depth', 'intrinsics', 'pose', 'bbox', 'ratio')
MIXED = ('plane', 'no_overlap', 'plane', 'behind', 'trunc', 'plane', 'no_overlap', 'plane')


def as_batch(arrays):
    """numpy arrays under the dataset's names -> CPU tensors (what a DataLoader hands over)."""
    return {f'{k}{s}': torch.from_numpy(np.ascontiguousarray(arrays[f'{k}{s}'])) for s in (1, 2) for k in SIDES}


def assert_equals(out, expected, masks=True):
    """Device results of a batch == list of reference / restatement results, exactly."""
    n = len(expected)
    box1, box2 = out['overlap_box1'].cpu().numpy(), out['overlap_box2'].cpu().numpy()
    valid, count = out['overlap_valid'].cpu().numpy(), out['overlap_count'].cpu().numpy()
    assert box1.shape == box2.shape == (n, 4) and box1.dtype == np.float32
    assert out['overlap_valid'].dtype == torch.bool and out['overlap_count'].dtype == torch.int32
    for p, e in enumerate(expected):
        assert e['margin'] >= cvo.MIN_MARGIN
        assert np.array_equal(box1[p], e['box1'].astype(np.float32)), (p, box1[p], e['box1'])
        assert np.array_equal(box2[p], e['box2'].astype(np.float32)), (p, box2[p], e['box2'])
        assert bool(valid[p]) == bool(e['valid']) and int(count[p]) == int(e['count']), (p, count[p], e['count'])
    if masks:
        m1, m2 = out['overlap_mask1'].cpu().numpy(), out['overlap_mask2'].cpu().numpy()
        assert m1.dtype == np.uint8
        for p, e in enumerate(expected):
            assert np.array_equal(m1[p], e['mask1']) and np.array_equal(m2[p], e['mask2']), p
            assert int(m1[p].sum()) == int(count[p])              # source pixels are distinct


@pytest.mark.parametrize('e', PINNED, ids=lambda e: f"{e['kind']}_{e['size']}_s{e['seed']}")
def test_pinned_scenes_equal_the_recorded_results(gpu, e):
    """Boxes, valid, count and masks EQUAL the recorded ones (the reference's), on the recorded inputs."""
    import imagematching_oetr_amd as pkg
    scene, res = cvo.checked_scene(e['kind'], e['size'], e['size'], e['seed'])
    assert cvo.sha(scene['depth1']) == e['depth1_sha256'] and cvo.sha(scene['depth2']) == e['depth2_sha256']
    batch = as_batch({k: v[None] for k, v in scene.items()})
    out = pkg.overlap_boxes_from_batch(batch, masks=True)
    assert out['overlap_box1'].device.type == 'cuda'
    got = dict(box1=out['overlap_box1'][0].cpu().numpy(), box2=out['overlap_box2'][0].cpu().numpy(),
               valid=bool(out['overlap_valid'][0]), count=int(out['overlap_count'][0]),
               mask1=out['overlap_mask1'][0].cpu().numpy(), mask2=out['overlap_mask2'][0].cpu().numpy())
    assert got['box1'].dtype == np.float32 and got['mask1'].dtype == np.uint8
    assert np.array_equal(got['box1'], got['box1'].astype(np.int64)) and np.array_equal(got['box2'], got['box2'].astype(np.int64))
    assert cvo.result_record(got) == {k: e[k] for k in cvo.result_record(got)}
    assert_equals(out, [res])                                      # and the restatement run here
    plain = pkg.overlap_boxes_from_batch(batch)                   # without masks: the same boxes, no mask keys
    assert sorted(plain) == ['overlap_box1', 'overlap_box2', 'overlap_count', 'overlap_valid']
    assert_equals(plain, [res], masks=False)


def test_one_call_on_device_resident_inputs(gpu):
    """Inputs already on the device (the small tensors too: T is then inverted there)."""
    import imagematching_oetr_amd as pkg
    scenes = [cvo.checked_scene(k, 160, 160, 40 + n) for n, k in enumerate(cvo.KINDS)]
    batch = as_batch({key: np.stack([sc[key] for sc, _ in scenes]) for key in scenes[0][0]})
    batch = {k: v.to(gpu) for k, v in batch.items()}
    assert_equals(pkg.overlap_boxes_from_batch(batch, masks=True), [r for _, r in scenes])


def test_generated_640_batch_mixed_valid_and_invalid(gpu):
    import imagematching_oetr_amd as pkg
    arrays, expected = cvo.scene_batch(MIXED, 640, 640, seed=100)
    assert [e['valid'] for e in expected] == [k in ('plane', 'trunc') for k in MIXED]
    out = pkg.overlap_boxes_from_batch(as_batch(arrays), masks=True)
    assert_equals(out, expected)


def test_generated_1024_pairs(gpu):
    import imagematching_oetr_amd as pkg
    arrays, expected = cvo.scene_batch(('plane', 'trunc'), 1024, 1024, seed=200)
    assert all(e['valid'] for e in expected)
    assert_equals(pkg.overlap_boxes_from_batch(as_batch(arrays), masks=True), expected)


def test_non_square_maps_follow_the_documented_rule(gpu):
    """480 x 640: landing columns are tested against W and rows against H (the reference compares with
    the other side and would index depth2 out of range)."""
    import imagematching_oetr_amd as pkg
    arrays, expected = cvo.scene_batch(('plane', 'trunc', 'plane'), 480, 640, seed=300)
    assert max(e['box2'][2] for e in expected) >= 480             # a landing column beyond H: the rule matters
    assert_equals(pkg.overlap_boxes_from_batch(as_batch(arrays), masks=True), expected)
    arrays, expected = cvo.scene_batch(('plane', 'trunc'), 640, 480, seed=301)
    assert max(e['box2'][3] for e in expected) >= 480
    assert_equals(pkg.overlap_boxes_from_batch(as_batch(arrays), masks=True), expected)


def test_float16_depth_equals_its_float32_upcast(gpu):
    import imagematching_oetr_amd as pkg
    arrays, _ = cvo.scene_batch(('plane', 'trunc'), 256, 256, seed=400)
    half = as_batch(arrays)
    half['depth1'], half['depth2'] = half['depth1'].half(), half['depth2'].half()
    up = dict(half, depth1=half['depth1'].float(), depth2=half['depth2'].float())
    a, b = pkg.overlap_boxes_from_batch(half, masks=True), pkg.overlap_boxes_from_batch(up, masks=True)
    assert int(a['overlap_count'].sum()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # ... and float64 maps are rounded to float32 (documented): the same as handing over the float32 maps
    c = pkg.overlap_boxes_from_batch(dict(up, depth1=up['depth1'].double(), depth2=up['depth2'].double()), masks=True)
    for k in a:
        assert torch.equal(b[k], c[k]), k


def _device_inputs(arrays, gpu):
    from imagematching_oetr_amd.covis import covis_params
    b = as_batch(arrays)
    params = covis_params(*(b[f'{k}{s}'] for s in (1, 2) for k in SIDES[1:])).to(gpu).contiguous()
    return b['depth1'].to(gpu).contiguous(), b['depth2'].to(gpu).contiguous(), params


def _snapshot(out):
    return {k: v.clone() for k, v in out.items() if k != 'workspace'}


def test_runs_are_bit_identical_and_a_workspace_carries_nothing_over(gpu):
    from imagematching_oetr_amd.covis import covis_boxes
    arr_a, exp_a = cvo.scene_batch(('plane', 'plane', 'trunc'), 320, 320, seed=500)
    arr_b, exp_b = cvo.scene_batch(('no_overlap', 'plane', 'behind'), 320, 320, seed=501)
    in_a, in_b = _device_inputs(arr_a, gpu), _device_inputs(arr_b, gpu)
    out = covis_boxes(*in_a, masks=True)
    first = _snapshot(out)
    ws = out['workspace']
    covis_boxes(*in_a, masks=True, out=out)                       # same workspace, same outputs
    second = _snapshot(out)
    for k in first:
        assert torch.equal(first[k], second[k]), k
    assert_equals(first, exp_a)
    # other inputs on the SAME workspace and output tensors: nothing of the first call is left
    # (pair 0 and 2 of the second batch have no inlier at all where the first had thousands)
    covis_boxes(*in_b, masks=True, out=out)
    assert out['workspace'] is ws
    assert_equals(_snapshot(out), exp_b)
    # a workspace full of garbage is as good as a fresh one
    ws.fill_(0xA5)
    covis_boxes(*in_a, masks=True, out=out)
    for k in first:
        assert torch.equal(first[k], out[k]), k


def test_captured_into_a_hip_graph_and_replayed_on_new_inputs(gpu):
    """Enqueue-only, no host read: the call is captured with default settings; a replay sees what the
    input buffers hold at replay time."""
    from imagematching_oetr_amd.covis import covis_boxes
    arr_a, exp_a = cvo.scene_batch(('plane', 'no_overlap'), 256, 256, seed=600)
    arr_b, exp_b = cvo.scene_batch(('trunc', 'plane'), 256, 256, seed=601)
    d1, d2, params = _device_inputs(arr_a, gpu)
    eager = _snapshot(covis_boxes(d1, d2, params, masks=True))    # also loads the library's code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = covis_boxes(d1, d2, params, masks=True)
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(captured[k], eager[k]), k
    new = _device_inputs(arr_b, gpu)
    d1.copy_(new[0]); d2.copy_(new[1]); params.copy_(new[2])
    graph.replay()
    torch.cuda.synchronize()
    assert_equals(captured, exp_b)
    assert_equals(eager, exp_a)


GUARD = 64


def _guarded(nbytes, gpu, skew=0):
    """``nbytes`` of device memory between two guard regions, starting ``skew`` bytes past a 64-byte boundary ->
    (the two guards, filled with 0xA5, and the slice between them)."""
    whole = torch.full((GUARD + skew + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    assert whole.data_ptr() % 64 == 0
    return (whole[:GUARD + skew], whole[GUARD + skew + nbytes:]), whole[GUARD + skew:GUARD + skew + nbytes]


def _guards_intact(guards):
    return all(bool((g == 0xA5).all()) for g in guards)


@pytest.mark.parametrize('n,h,w', [(3, 7, 9), (5, 5, 7)], ids=['189_bytes', '175_bytes'])
def test_ragged_clears_replayed_three_times_with_copies_between(gpu, n, h, w):
    """The call's clears under graph replay: the workspace (64 bytes a pair) and, with masks, two of ``n * h * w``
    bytes - here 189 and 175, no multiple of 16.  While the clears were ``hipMemsetAsync`` nodes, the 3-pair capture
    came back with a foreign pattern in its accumulators on the graph's SECOND replay after device copies, the
    fault ``clear_i32`` (``csrc/match_score.hip``) records; they are kernels now (``clear_acc``, ``k_clear_u8_pair``).
    Three replays with ``copy_`` of new scenes between them: after each, boxes, counts, valid and masks are the
    restatement of what the inputs held, and the bytes around the masks and the workspace are untouched.  The second
    set of scenes has no inlier at all where the first had many: nothing may be left."""
    from imagematching_oetr_amd import hip_engine
    from imagematching_oetr_amd.covis import covis_boxes
    kinds = (('plane', 'trunc', 'plane', 'trunc', 'plane'), ('no_overlap', 'behind', 'no_overlap', 'behind', 'no_overlap'),
             ('trunc', 'no_overlap', 'plane', 'plane', 'behind'))
    rounds = [cvo.scene_batch(k[:n], h, w, seed=900 + 50 * r) for r, k in enumerate(kinds)]
    assert sum(e['count'] for e in rounds[0][1]) > 0 and not any(e['valid'] for e in rounds[1][1])
    assert (n * h * w) % 16 != 0
    d1, d2, params = _device_inputs(rounds[0][0], gpu)
    covis_boxes(d1, d2, params, masks=True)                       # loads the library's code objects
    need = int(hip_engine.load_library().oetr_covis_workspace_bytes(n))
    assert need == 64 * n
    whole1, m1 = _guarded(n * h * w, gpu)
    whole2, m2 = _guarded(n * h * w, gpu, skew=5)                  # mask 2 starts 5 bytes past a 16-byte boundary
    whole_ws, ws = _guarded(need, gpu)
    out = {'overlap_box1': torch.empty(n, 4, device=gpu), 'overlap_box2': torch.empty(n, 4, device=gpu),
           'overlap_valid': torch.empty(n, dtype=torch.bool, device=gpu),
           'overlap_count': torch.empty(n, dtype=torch.int32, device=gpu),
           'overlap_mask1': m1.view(n, h, w), 'overlap_mask2': m2.view(n, h, w), 'workspace': ws}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert covis_boxes(d1, d2, params, masks=True, out=out) is out
    assert out['workspace'] is ws and out['overlap_mask1'].data_ptr() == m1.data_ptr()
    for r, (arrays, expected) in enumerate(rounds):
        if r:
            new = _device_inputs(arrays, gpu)
            d1.copy_(new[0]); d2.copy_(new[1]); params.copy_(new[2])
        graph.replay()
        torch.cuda.synchronize()
        assert_equals({k: v for k, v in out.items() if k != 'workspace'}, expected)
        assert _guards_intact(whole1) and _guards_intact(whole2) and _guards_intact(whole_ws), r


def test_masks_larger_than_one_pass_of_the_clearing_kernel(gpu):
    """``k_clear_u8_pair`` has at most ``CLEAR_MAX_BLOCKS`` blocks of ``CLEAR_THREADS`` threads a mask, 16 bytes a
    thread and pass (both read from the source): 17 pairs of 1024 x 1024 are 17 MiB a mask, so the first threads
    store a second time.  Masks full of 0xA5 beforehand; every byte is compared."""
    import re
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd.covis import covis_boxes
    src = (Path(pkg.__file__).parent / 'csrc' / 'covis.hip').read_text()
    threads = int(re.search(r'constexpr int CLEAR_THREADS = (\d+);', src).group(1))
    blocks = int(re.search(r'constexpr unsigned CLEAR_MAX_BLOCKS = (\d+);', src).group(1))
    n, side = 17, 1024
    assert n * side * side > blocks * threads * 16
    scenes = [cvo.checked_scene(kind, side, side, 40 + k) for k, kind in enumerate(('plane', 'no_overlap'))]
    pick = [p % 2 for p in range(n)]
    tile = lambda key: torch.from_numpy(np.stack([scenes[k][0][key] for k in (0, 1)])).to(gpu)[pick].contiguous()
    params = torch.from_numpy(np.stack([cvo.param_block(scenes[k][0]) for k in pick])).to(gpu)
    d1, d2 = tile('depth1'), tile('depth2')
    out = covis_boxes(d1, d2, params, masks=True)
    for key in ('overlap_mask1', 'overlap_mask2'):
        out[key].fill_(0xA5)
    covis_boxes(d1, d2, params, masks=True, out=out)
    want1 = torch.from_numpy(np.stack([scenes[k][1]['mask1'] for k in (0, 1)])).to(gpu)[pick]
    want2 = torch.from_numpy(np.stack([scenes[k][1]['mask2'] for k in (0, 1)])).to(gpu)[pick]
    assert torch.equal(out['overlap_mask1'], want1) and torch.equal(out['overlap_mask2'], want2)
    assert out['overlap_count'].tolist() == [scenes[k][1]['count'] for k in pick] and scenes[0][1]['count'] > 50000


def test_on_a_side_stream(gpu):
    import imagematching_oetr_amd as pkg
    arrays, expected = cvo.scene_batch(('plane', 'trunc'), 192, 192, seed=700)
    side = torch.cuda.Stream(device=gpu)
    b = as_batch(arrays)
    out = pkg.overlap_boxes_from_depth(*(b[f'{k}{s}'] for s in (1, 2) for k in SIDES), masks=True, stream=side)
    side.synchronize()
    assert_equals(out, expected)


# ------------------------------------------------------------------ evaluate_dummy on the device
def _recalls_numpy(ious, thrs):
    ious = np.asarray(ious)
    return np.array([(ious >= t).sum() / float(ious.shape[0]) for t in thrs])


def _iou_numpy(a, b):
    a, b = a.astype(np.float32), b.astype(np.float32)
    wh = np.clip(np.minimum(a[:, 2:], b[:, 2:]) - np.maximum(a[:, :2], b[:, :2]), 0, None)
    ov = wh[:, 0] * wh[:, 1]
    union = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - ov
    return ov / np.maximum(union, np.float32(1e-6))


def test_evaluate_dummy_depth_and_batch_ground_truth_agree(gpu):
    """The whole chain on the device: images -> forward_dummy, depth + poses -> ground truth, IoU,
    recall.  gt='depth' and gt='batch' fed the same ground truth return identical results, and both
    equal the recall computed on the host from the same boxes."""
    import imagematching_oetr_amd as pkg
    torch.manual_seed(0)
    model = pkg.OETR(pkg.get_cfg_defaults().OETR).eval().to(gpu)
    g = torch.Generator().manual_seed(5)
    batches, truth = [], []
    for n, kinds in enumerate((('plane', 'trunc', 'no_overlap'), ('trunc', 'plane'))):
        arrays, expected = cvo.scene_batch(kinds, 320, 320, seed=800 + n)
        b = as_batch(arrays)
        b['image1'], b['image2'] = torch.rand(len(kinds), 320, 320, 3, generator=g), torch.rand(len(kinds), 320, 320, 3, generator=g)
        batches.append(b)
        truth.append(expected)
    for b in batches:                                              # warm-up: the trunk's convolution algorithms are chosen
        model.forward_dummy(b['image1'].to(gpu), b['image2'].to(gpu))
    model.hip_flush()
    low = np.array([0.01, 0.02, 0.05, 0.1, 0.2, 0.5])              # a random-weight model's boxes are poor: thresholds that tell
    with_boxes = []
    for b, expected in zip(batches, truth):
        wb = {k: v for k, v in b.items() if not k.startswith(('depth', 'pose', 'intrinsics'))}
        wb['overlap_box1'] = torch.from_numpy(np.stack([e['box1'] for e in expected]))        # int64, as the dataset's
        wb['overlap_box2'] = torch.from_numpy(np.stack([e['box2'] for e in expected]))
        wb['overlap_valid'] = torch.tensor([e['valid'] for e in expected])
        with_boxes.append(wb)
    # the host's arithmetic on the settled boxes
    ious = []
    for b, expected in zip(batches, truth):
        p1, p2 = model.forward_dummy(b['image1'].to(gpu), b['image2'].to(gpu))
        model.hip_flush()
        ious += list(_iou_numpy(np.stack([e['box1'] for e in expected]), p1.cpu().numpy()))
        ious += list(_iou_numpy(np.stack([e['box2'] for e in expected]), p2.cpu().numpy()))
    for thrs in (np.arange(0.5, 0.96, 0.05), low):
        by_depth = pkg.evaluate_dummy(model, batches, iou_thrs=thrs, gt='depth')
        by_batch = pkg.evaluate_dummy(model, with_boxes, iou_thrs=thrs, gt='batch')
        auto = pkg.evaluate_dummy(model, with_boxes, iou_thrs=thrs)      # 'auto' takes the batch's boxes (no depth there)
        print('recalls', thrs, by_depth['recalls'], 'mean_iou', by_depth['mean_iou'])
        for other in (by_batch, auto):
            assert np.array_equal(by_depth['recalls'], other['recalls'])
            assert by_depth['n'] == other['n'] == 10 and by_depth['n_valid_pairs'] == other['n_valid_pairs'] == 4
            # (the mean is compared loosely: two runs of the trunk's library convolutions need not agree to the bit)
            assert by_depth['mean_iou'] == pytest.approx(other['mean_iou'], rel=1e-5)
        assert np.array_equal(by_depth['recalls'], _recalls_numpy(ious, thrs))
        assert by_depth['mean_iou'] == pytest.approx(float(np.mean(np.asarray(ious, np.float64))), rel=1e-5) and by_depth['mean_iou'] > 0


class _FeatureModel:
    """``forward_dummy`` standing on ``boxes_from_features`` with prepared features (the images are not
    looked at): the way ``tests/test_gpu_precision.py`` feeds the module features that leave the f16
    operand range, which the range guard catches and the deferred check repairs in place."""

    def __init__(self, model, feature_batches):
        self.model, self.feature_batches, self.at = model, feature_batches, 0

    def parameters(self):
        return self.model.parameters()

    def hip_flush(self):
        self.model.hip_flush()

    def forward_dummy(self, image1, image2):
        feats = self.feature_batches[self.at]
        self.at += 1
        return self.model.boxes_from_features(*feats, (256, 320), (320, 256))


def test_evaluate_dummy_counts_settled_boxes_only(gpu):
    """A batch whose features overflow the f16 operand range: its boxes are wrong until the deferred
    check has re-run it in exact fp32.  The recalls equal those of the exact-fp32 boxes."""
    import imagematching_oetr_amd as pkg
    torch.manual_seed(0)
    model = pkg.OETR(pkg.get_cfg_defaults().OETR).eval()
    sd = model.state_dict()
    w = orc.make_hot_weights(5, sharpen=True)
    sd.update(w)
    model.load_state_dict(sd, strict=True)
    model = model.to(gpu)
    assert model.hip_defer_check and model.hip_on_overflow == 'f32'
    f1, f2 = orc.make_features(95, 2, 8, 10), orc.make_features(96, 2, 10, 8)
    p1, p2 = orc.position_table(8, 10), orc.position_table(10, 8)
    bad = [t.to(gpu) for t in (f1 * 4.0e5, f2, p1, p2)]           # trips the range guard
    good = [t.to(gpu) for t in (f1, f2, p1, p2)]
    exact = pkg.HotPathEngine(w, device=gpu, precision='f32')
    exact.set_decoder_split(1)                                     # as the module's re-run route
    e_bad = [t.clone() for t in exact.forward(*bad, (256, 320), (320, 256))]
    e_good = [t.clone() for t in model.engine().forward(*good, (256, 320), (320, 256))]
    assert model.engine().query_flags(clear=True) == 0
    raw = [t.clone() for t in model.engine().forward(*bad, (256, 320), (320, 256))]
    assert model.engine().query_flags(clear=True) & pkg.FLAG_F16_RANGE
    torch.cuda.synchronize()
    # ground truth: the exact boxes of the overflowing batch moved by a few pixels, those of the good batch as they are
    shift = torch.tensor([3.0, -2.0, 4.0, 5.0], device=gpu)
    images = torch.zeros(2, 8, 8, 3)
    batches = [dict(image1=images, image2=images, overlap_box1=e_bad[0] + shift, overlap_box2=e_bad[1] - shift),
               dict(image1=images, image2=images, overlap_box1=e_good[0], overlap_box2=e_good[1] + shift)]
    res = pkg.evaluate_dummy(_FeatureModel(model, [bad, good]), batches, gt='batch')
    thrs = np.arange(0.5, 0.96, 0.05)
    gts = [b[k].cpu().numpy() for b in batches for k in ('overlap_box1', 'overlap_box2')]
    preds = [t.cpu().numpy() for t in (e_bad[0], e_bad[1], e_good[0], e_good[1])]
    want = _recalls_numpy(np.concatenate([_iou_numpy(a, b) for a, b in zip(gts, preds)]), thrs)
    assert res['n'] == 8 and np.array_equal(res['recalls'], want), (res['recalls'], want)
    # ... which the unsettled boxes would not have given
    unsettled = [t.cpu().numpy() for t in (raw[0], raw[1], e_good[0], e_good[1])]
    with np.errstate(all='ignore'):
        wrong = _recalls_numpy(np.concatenate([_iou_numpy(a, b) for a, b in zip(gts, unsettled)]), thrs)
    assert not np.array_equal(wrong, want)
    assert want[0] > 0
