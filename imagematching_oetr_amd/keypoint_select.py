"""Keypoints selected and descriptors sampled from an extractor network's dense maps, for all images of a call.

``match_descriptors`` and ``assemble_matches`` start from ``keypoints`` / ``scores`` / ``descriptors``.  An extractor
network delivers, per image, a dense score map ``[H,W]`` and a dense descriptor map ``[D,h,w]``; the head behind it is
:func:`select_keypoints`: non-maximum suppression, a threshold, a border, the best ``max_keypoints``, descriptors
sampled at the keypoints and normalised - for every map of a :func:`keypoint_map_table` (mixed sizes) in one HIP call
of thirteen launches (``oetr_keypoint_select``, ``include/oetr_keypoint_select.h``, ``csrc/keypoint_select.hip``).  The
network itself stays torch.

The statement is this project's own, modelled on SuperPoint's published post-processing (``simple_nms`` with its two
suppression rounds, ``remove_borders``, ``top_k_keypoints``, ``sample_descriptors``); DESIGN 9.3n writes it down and
the kernels reproduce its numpy form bit for bit.  Where ``torch.topk`` leaves the order of tied scores open, the lower
raster index wins.  There is no CPU implementation.
"""
import ctypes as C

import torch

from . import hip_engine
from ._inputs import _device_of, _is_host, _refuse_float64, _refuse_host_inputs_in_capture, _workspace
from .hip_engine import (KEYPOINT_SELECT_COUNTERS, KEYPOINT_SELECT_MAX_D, KEYPOINT_SELECT_MAX_KEYPOINTS,
                         KEYPOINT_SELECT_MAX_RADIUS, KEYPOINT_SELECT_MAX_SIDE, KEYPOINT_SELECT_MIN_D,
                         KEYPOINT_SELECT_PIXEL_ALIGN, _check, _KeypointMap, _stream)


class KeypointMapTable:
    """The device table of a keypoint-selection call (``oetr_keypoint_map[n]``) and what the host knows about it:
    ``n``, ``channels`` (D), ``max_pixels``, ``total_pixels``.  Keeps the maps alive."""

    def __init__(self, table, maps, n, channels, max_pixels, total_pixels):
        self.table, self.maps = table, maps
        self.n, self.channels, self.max_pixels, self.total_pixels = n, channels, max_pixels, total_pixels
        self.device = table.device

    def __len__(self):
        return self.n


def _map_list(name, maps, dims):
    """A batched tensor ``[B, ...]`` or a sequence of per-image tensors -> a list of ``dims``-dimensional views."""
    if torch.is_tensor(maps):
        if maps.dim() != dims + 1:
            raise ValueError(f'{name} as one tensor must have {dims + 1} dimensions (a batch), got {tuple(maps.shape)}')
        return list(maps.unbind(0))
    return list(maps)


def keypoint_map_table(scores, descriptors):
    """The map table of :func:`select_keypoints`.  ``scores``: n float32 score maps ``[H,W]`` (a list, sizes may
    differ, or one ``[n,H,W]`` tensor); ``descriptors``: n float32 descriptor maps ``[D,h,w]`` with one D (a list, or
    one ``[n,D,h,w]`` tensor).  A descriptor map is read through its three strides, so an NCHW and a channels-last
    tensor both go in without a copy; a score map whose rows are not dense is copied; host tensors are uploaded with
    blocking copies (refused inside a graph capture).  ``D % 4 == 0`` and ``4 <= D <= 512``.  The table is written on
    the host into pinned memory and goes to the device in ONE copy; it holds the maps' addresses, so new values
    written INTO the same tensors are what the next call - or the replay of a graph that holds one - reads."""
    scores, descriptors = _map_list('scores', scores, 2), _map_list('descriptors', descriptors, 3)
    n = len(scores)
    if n < 1 or len(descriptors) != n:
        raise ValueError('keypoint_map_table: one score map and one descriptor map per image, at least one image')
    for name, maps, dims in (('scores', scores, 2), ('descriptors', descriptors, 3)):
        for b, t in enumerate(maps):
            if not torch.is_tensor(t):
                raise ValueError(f'keypoint_map_table: {name} must be torch tensors')
            _refuse_float64(name, t)
            if t.dtype != torch.float32 or t.dim() != dims:
                raise ValueError(f'keypoint_map_table: {name}[{b}] must be float32 with {dims} dimensions, got '
                                 f'{t.dtype} {tuple(t.shape)}')
            if min(t.shape) < 1 or max(t.shape[-2:]) > KEYPOINT_SELECT_MAX_SIDE:
                raise ValueError(f'keypoint_map_table: {name}[{b}] is {tuple(t.shape)}: sides must lie in '
                                 f'[1, {KEYPOINT_SELECT_MAX_SIDE}]')
    D = int(descriptors[0].shape[0])
    if D % 4 or not KEYPOINT_SELECT_MIN_D <= D <= KEYPOINT_SELECT_MAX_D:
        raise ValueError(f'need D % 4 == 0 and {KEYPOINT_SELECT_MIN_D} <= D <= {KEYPOINT_SELECT_MAX_D}, got D = {D}')
    for b, f in enumerate(descriptors):
        if int(f.shape[0]) != D:
            raise ValueError(f'keypoint_map_table: descriptors[{b}] has {int(f.shape[0])} channels, the first map {D}')
    devices = {t.device for t in scores + descriptors if t.device.type != 'cpu'}
    if len(devices) > 1 or any(d.type != 'cuda' for d in devices):
        raise ValueError(f'keypoint_map_table: the maps must be on the CPU or on ONE GPU, got {sorted(map(str, devices))}')
    dev = _device_of('keypoint_map_table', scores + descriptors)
    host = sorted({name for name, maps in (('scores', scores), ('descriptors', descriptors)) if any(_is_host(t) for t in maps)})
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host)
    scores = [t.to(dev) for t in scores]                # from the host: blocking copies
    descriptors = [t.to(dev) for t in descriptors]
    rows = (_KeypointMap * n)()
    keep, max_pixels, total = [], 0, 0
    for b, (s, f) in enumerate(zip(scores, descriptors)):
        if s.stride(1) != 1 or s.stride(0) < 0:
            s = s.contiguous()
        if min(f.stride()) < 0:
            f = f.contiguous()
        keep += [s, f]
        H, W = int(s.shape[0]), int(s.shape[1])
        r = rows[b]
        r.scores, r.H, r.W, r.score_stride = s.data_ptr(), H, W, int(s.stride(0))
        r.desc, r.h, r.w = f.data_ptr(), int(f.shape[1]), int(f.shape[2])
        r.desc_stride[0], r.desc_stride[1], r.desc_stride[2] = (int(x) for x in f.stride())
        r.pixel_offset = total
        max_pixels = max(max_pixels, H * W)
        end = total + H * W
        total = -(-end // KEYPOINT_SELECT_PIXEL_ALIGN) * KEYPOINT_SELECT_PIXEL_ALIGN
    staged = torch.empty(n * C.sizeof(_KeypointMap), dtype=torch.uint8).pin_memory()
    C.memmove(staged.data_ptr(), C.addressof(rows), n * C.sizeof(_KeypointMap))
    table = staged.to(dev, non_blocking=True)
    res = KeypointMapTable(table, keep, n, D, max_pixels, total)
    res._staged = staged        # pinned source of the asynchronous copy
    return res


def _check_parameters(nms_radius, threshold, remove_borders, max_keypoints, cell):
    if max_keypoints is None:
        raise ValueError('`max_keypoints` is required: it sizes the outputs, and nothing is read back to find it')
    if not 1 <= int(max_keypoints) <= KEYPOINT_SELECT_MAX_KEYPOINTS:
        raise ValueError(f'need 1 <= max_keypoints <= {KEYPOINT_SELECT_MAX_KEYPOINTS}, got {max_keypoints}')
    if not 0 <= int(nms_radius) <= KEYPOINT_SELECT_MAX_RADIUS:
        raise ValueError(f'need 0 <= nms_radius <= {KEYPOINT_SELECT_MAX_RADIUS}, got {nms_radius}')
    if not float(threshold) >= 0:
        raise ValueError(f'need threshold >= 0, got {threshold}')
    if int(remove_borders) < 0:
        raise ValueError(f'need remove_borders >= 0, got {remove_borders}')
    if int(cell) < 1:
        raise ValueError(f'need cell >= 1, got {cell}')


@torch.no_grad()
def select_keypoints(table, nms_radius=4, threshold=0.005, remove_borders=4, max_keypoints=None, cell=8, out=None):
    """The keypoints of every map of ``table`` (:func:`keypoint_map_table`), in one device call.

    ``nms_radius`` 0..8, ``threshold`` >= 0, ``remove_borders`` >= 0, ``max_keypoints`` 1..4096 (required: it sizes
    the outputs), ``cell``: the score map's pixels per descriptor cell.  Per map: a NaN score counts as ``-inf``;
    SuperPoint's ``simple_nms`` with its two suppression rounds; the candidates are the pixels with a score above
    ``threshold`` at least ``remove_borders`` away from every edge; at most ``max_keypoints`` candidates are all kept,
    in raster order, otherwise the best ``max_keypoints`` in descending score order, a tie going to the lower raster
    index; the descriptor is SuperPoint's ``sample_descriptors`` (bilinear, ``align_corners=True``, L2-normalised).

    Returns a dict of device tensors with ``n * max_keypoints`` rows of capacity: ``keypoints`` float32 ``[rows,2]``
    (x, y), ``scores`` float32 ``[rows]``, ``descriptors`` float32 ``[rows,D]``, ``offsets`` int32 ``[n+1]`` (map ``b``
    owns rows ``offsets[b] .. offsets[b+1]-1``) and ``counts`` int32 ``[n,2]`` (candidates, kept;
    :func:`keypoint_counts` reads them).  Rows from ``offsets[n]`` on read ``-1`` / NaN / ``0``.

    ``match_descriptors(res0['descriptors'], res1['descriptors'], offsets0=res0['offsets'], offsets1=res1['offsets'],
    max_k0=max_keypoints, max_k1=max_keypoints)`` and ``assemble_matches(..., res0['keypoints'], res1['keypoints'], ...,
    offsets0=res0['offsets'], offsets1=res1['offsets'])`` take the result as it is.  Enqueues on torch's current stream
    of the table's device and reads nothing back, so it can be captured into a HIP graph.  ``out``: the result of an
    earlier call of the same table and ``max_keypoints``, written into again with no allocation."""
    _check_parameters(nms_radius, threshold, remove_borders, max_keypoints, cell)
    if not isinstance(table, KeypointMapTable):
        raise ValueError('select_keypoints takes a keypoint_map_table(...)')
    dev, n, D, k = table.device, table.n, table.channels, int(max_keypoints)
    rows = n * k
    if rows > 2 ** 31 - 1:
        raise ValueError('more than 2^31 - 1 rows of capacity (maps * max_keypoints) in one call')
    lib = hip_engine.load_library()
    need = int(lib.oetr_keypoint_select_workspace_bytes(table.total_pixels, n, k))
    if need == 0:
        raise ValueError('select_keypoints: the table is too large for one call')
    with torch.cuda.device(dev):
        if out is None:
            i32 = dict(dtype=torch.int32, device=dev)
            out = {'keypoints': torch.empty(rows, 2, device=dev), 'scores': torch.empty(rows, device=dev),
                   'descriptors': torch.empty(rows, D, device=dev), 'offsets': torch.empty(n + 1, **i32),
                   'counts': torch.empty(n, KEYPOINT_SELECT_COUNTERS, **i32)}
        elif (tuple(out['keypoints'].shape) != (rows, 2) or tuple(out['descriptors'].shape) != (rows, D)
              or tuple(out['scores'].shape) != (rows,) or tuple(out['offsets'].shape) != (n + 1,)
              or tuple(out['counts'].shape) != (n, KEYPOINT_SELECT_COUNTERS) or out['keypoints'].device != dev
              or not all(out[key].is_contiguous() for key in ('keypoints', 'scores', 'descriptors', 'offsets', 'counts'))):
            raise ValueError('`out` is the result of a call of other sizes (maps, max_keypoints, D)')
        workspace = _workspace(out, need, dev)
        _check(lib, lib.oetr_keypoint_select(
            table.table.data_ptr(), n, table.max_pixels, table.total_pixels, D, int(nms_radius), float(threshold),
            int(remove_borders), k, int(cell), workspace.data_ptr(), workspace.numel(), out['keypoints'].data_ptr(),
            out['scores'].data_ptr(), out['descriptors'].data_ptr(), out['offsets'].data_ptr(),
            out['counts'].data_ptr(), _stream(dev)), 'oetr_keypoint_select')
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = table
    return out


def keypoint_counts(result):
    """The counters of a :func:`select_keypoints` result as a host int32 array ``[n,2]`` - candidates, kept; two ``-1``
    for a map whose record is unusable.  ONE read, which synchronises the stream."""
    return result['counts'].cpu().numpy()
