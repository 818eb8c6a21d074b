"""Ground-truth overlap boxes from depth maps, intrinsics and poses, on the device.

The reference scores ``forward_dummy``'s boxes against co-visibility boxes that its dataset
computes per sample on the CPU (``numpy_overlap_box``, ``src/datasets/utils.py:140-202``, called
from ``src/datasets/megadepth_pairs.py:158-175``): every pixel of depth map 1 that has a depth is
un-projected, moved into camera 2 with the two poses, projected, and kept when it lands inside
image 2 at a depth within 0.5 of that image's depth map; the boxes are the bounding boxes of the
surviving pixels on both sides.  ``overlap_boxes_from_depth`` is that function for a batch of
pairs as one HIP call (``oetr_covis_boxes``, ``include/oetr_covis.h``; kernel
``csrc/covis.hip``), in float64 like the reference.  There is no CPU implementation.
"""
import ctypes as C

import torch

from . import hip_engine
from ._inputs import _device_of
from .hip_engine import COVIS_PARAM_DOUBLES, _check, _stream

_SIDES = ('depth', 'intrinsics', 'pose', 'bbox', 'ratio')


def covis_params(intrinsics1, pose1, bbox1, ratio1, intrinsics2, pose2, bbox2, ratio2):
    """The per-pair parameter block of ``oetr_covis_boxes``: float64 ``[N, 40]`` on the device the
    poses live on (layout: ``include/oetr_covis.h``).  ``T = pose2 @ inverse(pose1)`` with
    ``torch.linalg.inv_ex`` in float64; ``bbox`` / ``ratio`` are ``[N,2]`` in the reference's
    (row, col) order."""
    f64 = lambda t, shape: torch.as_tensor(t).to(device=torch.as_tensor(pose1).device, dtype=torch.float64).reshape(shape)
    p1, p2 = f64(pose1, (-1, 4, 4)), f64(pose2, (-1, 4, 4))
    n = p1.shape[0]
    k1, k2 = f64(intrinsics1, (n, 3, 3)), f64(intrinsics2, (n, 3, 3))
    T = p2 @ torch.linalg.inv_ex(p1).inverse        # (inv_ex: no error check, so no synchronisation on a GPU)
    params = torch.zeros(n, COVIS_PARAM_DOUBLES, dtype=torch.float64, device=p1.device)
    params[:, 0:16] = T.reshape(n, 16)
    params[:, 16], params[:, 17], params[:, 18], params[:, 19] = k1[:, 0, 0], k1[:, 1, 1], k1[:, 0, 2], k1[:, 1, 2]
    params[:, 20:29] = k2.reshape(n, 9)
    params[:, 29:31], params[:, 31:33] = f64(bbox1, (n, 2)), f64(ratio1, (n, 2))
    params[:, 33:35], params[:, 35:37] = f64(bbox2, (n, 2)), f64(ratio2, (n, 2))
    return params


def covis_boxes(depth1, depth2, params, masks=False, out=None):
    """``oetr_covis_boxes`` on device tensors as they are: ``depth1`` / ``depth2`` contiguous float32
    ``[N,H,W]``, ``params`` contiguous float64 ``[N,40]`` (:func:`covis_params`), all on one GPU.
    Enqueues on torch's current stream of that GPU and reads nothing back, so it can be captured into
    a HIP graph.  ``out``: the result dict of an earlier call of the same shape, to write into again (its
    tensors and the workspace it carries as ``out['workspace']``)."""
    dev = depth1.device
    if dev.type != 'cuda':
        raise RuntimeError('covis_boxes needs its tensors on a GPU (HIP) device; there is no CPU implementation')
    for name, t, dt, nd in (('depth1', depth1, torch.float32, 3), ('depth2', depth2, torch.float32, 3),
                            ('params', params, torch.float64, 2)):
        if t.dtype != dt or t.dim() != nd or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'{name} must be a contiguous {dt} tensor with {nd} dimensions on {dev}')
    n, H, W = (int(v) for v in depth1.shape)
    if tuple(depth2.shape) != (n, H, W):
        raise ValueError(f'depth2 is {tuple(depth2.shape)}, depth1 {tuple(depth1.shape)}: all maps of a call share one shape')
    if tuple(params.shape) != (n, COVIS_PARAM_DOUBLES):
        raise ValueError(f'params must be [{n},{COVIS_PARAM_DOUBLES}], got {tuple(params.shape)}')
    lib = hip_engine.load_library()
    need = int(lib.oetr_covis_workspace_bytes(n))
    if out is None:
        out = {'overlap_box1': torch.empty(n, 4, device=dev), 'overlap_box2': torch.empty(n, 4, device=dev),
               'overlap_valid': torch.empty(n, dtype=torch.bool, device=dev),
               'overlap_count': torch.empty(n, dtype=torch.int32, device=dev)}
        if masks:
            out['overlap_mask1'] = torch.empty(n, H, W, dtype=torch.uint8, device=dev)
            out['overlap_mask2'] = torch.empty(n, H, W, dtype=torch.uint8, device=dev)
    workspace = out.get('workspace')
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    out['workspace'] = workspace
    m1, m2 = (out['overlap_mask1'], out['overlap_mask2']) if masks else (None, None)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        _check(lib, lib.oetr_covis_boxes(
            ptr(depth1), ptr(depth2), ptr(params), n, H, W, ptr(workspace), workspace.numel(),
            ptr(out['overlap_box1']), ptr(out['overlap_box2']), ptr(out['overlap_valid']),
            ptr(out['overlap_count']), ptr(m1), ptr(m2), _stream(dev)), 'oetr_covis_boxes')
    return out


@torch.no_grad()
def overlap_boxes_from_depth(depth1, intrinsics1, pose1, bbox1, ratio1, depth2, intrinsics2, pose2, bbox2, ratio2,
                             masks=False, stream=None):
    """Co-visibility boxes of N pairs, as the reference's ``numpy_overlap_box`` computes them.

    Inputs are batched tensors in the layout and under the names the reference's dataset emits
    (``src/datasets/megadepth_pairs.py:176-199``), on any device and of any float dtype:
    ``depthK`` ``[N,H,W]`` (0: no depth; one shape for every map of the call), ``intrinsicsK``
    ``[N,3,3]``, ``poseK`` ``[N,4,4]`` (world to camera), ``bboxK`` ``[N,2]`` (row, col offset of the
    crop) and ``ratioK`` ``[N,2]`` (row, col resize factors).

    Depth maps go to the device as float32: float16 and float32 maps are represented exactly, a
    float64 map is ROUNDED to float32 (the reference would have used the float64 values).  The
    small tensors are combined in float64 on the device they live on and moved without a
    synchronisation; the warp itself runs in float64.

    Returns device tensors: ``overlap_box1`` / ``overlap_box2`` float32 ``[N,4]`` (x1, y1, x2, y2 of the
    inlier pixels; zeros for a pair without inliers, as the reference returns), ``overlap_valid``
    bool ``[N]``, ``overlap_count`` int32 ``[N]`` and, with ``masks=True``, ``overlap_mask1`` /
    ``overlap_mask2`` uint8 ``[N,H,W]``.  ``stream``: a ``torch.cuda.Stream`` to enqueue on (default:
    the current one).  Parity with the reference holds for square maps; for ``H != W`` the landing
    test is ``i < W, j < H`` where the reference compares with the other side
    (``include/oetr_covis.h``).  Without a GPU this raises ``RuntimeError``."""
    dev = _device_of('overlap_boxes_from_depth', (depth1, depth2, pose1, pose2, intrinsics1, intrinsics2))
    d1, d2 = torch.as_tensor(depth1), torch.as_tensor(depth2)
    if d1.dim() != 3 or d1.shape != d2.shape:
        raise ValueError(f'depth1 / depth2 must be [N,H,W] of one shape, got {tuple(d1.shape)} / {tuple(d2.shape)}')
    if not (d1.is_floating_point() and d2.is_floating_point()):
        raise ValueError('depth maps must be floating-point tensors')
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        params = covis_params(intrinsics1, pose1, bbox1, ratio1, intrinsics2, pose2, bbox2, ratio2)
        if params.shape[0] != d1.shape[0]:
            raise ValueError(f'{d1.shape[0]} depth maps, {params.shape[0]} poses')
        to_dev = lambda t: t.to(dtype=torch.float32).to(dev, non_blocking=True).contiguous()
        out = covis_boxes(to_dev(d1), to_dev(d2), params.to(dev, non_blocking=True).contiguous(), masks=masks)
    del out['workspace']
    return out


def overlap_boxes_from_batch(batch, masks=False, stream=None):
    """:func:`overlap_boxes_from_depth` on a dataset-style dict with ``depth1``, ``intrinsics1``,
    ``pose1``, ``bbox1``, ``ratio1`` and the same five for ``2``."""
    missing = [f'{k}{s}' for s in (1, 2) for k in _SIDES if f'{k}{s}' not in batch]
    if missing:
        raise KeyError(f'batch lacks {missing}: ground truth from depth needs depth, intrinsics, pose, bbox and '
                       'ratio of both images')
    args = [batch[f'{k}{s}'] for s in (1, 2) for k in _SIDES]
    return overlap_boxes_from_depth(*args, masks=masks, stream=stream)
