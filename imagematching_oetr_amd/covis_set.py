"""Ground-truth overlap boxes for pairs given by INDEX into a set of depth maps, and pair mining.

``overlap_boxes_from_depth`` (``covis.py``) takes one stacked depth tensor per side: every pair
carries its own two maps and all maps of a call share one shape.  The jobs the boxes are used for
are pair LISTS over an image SET - scoring ``forward_pairs_indexed``, mining training pairs of a
scene as the reference's ``src/utils/megadepth_preprocess.py`` does - where a map serves many pairs
and the maps have their native, differing sizes.  A :class:`DepthSet` holds each map once, in device
memory, with its camera; :func:`overlap_boxes_indexed` computes the boxes of a pair list from it in
one HIP call that reads the maps in place (``oetr_covis_boxes_indexed``,
``include/oetr_covis_set.h``; the per-pixel arithmetic is the one copy ``oetr_covis_boxes`` runs),
and :func:`mine_pairs` applies the reference's mining criterion on the device
(``oetr_covis_select``).  There are no masks here (a mask per pair is per-pair memory again) and
there is no CPU implementation.
"""
import ctypes as C

import torch

from . import hip_engine
from ._inputs import _pair_tensor, _workspace
from .hip_engine import COVIS_MAX_SIDE, COVIS_PARAM_DOUBLES, _check, _CovisMap, _stream

# One image's float64 record, 45 values: pose [0:16], inverse(pose) [16:32], K [32:41], bbox [41:43], ratio [43:45]


class DepthSet:
    """Depth maps of an image set with their cameras, on one GPU::

        ds = DepthSet(device)
        slot = ds.add(depth, intrinsics, pose, bbox=(0, 0), ratio=(1, 1))
        out = overlap_boxes_indexed(ds, [(0, 1), (1, 0), (0, 2)])
        ds.clear()

    ``depth`` ``[H,W]`` (0: no depth; any float dtype, any device, any size up to 8192 a side) goes to
    the device as float32: float16 and float32 maps are represented exactly, a float64 map is
    ROUNDED to float32 (the reference would have used the float64 values).  ``intrinsics`` ``[3,3]``,
    ``pose`` ``[4,4]`` (world to camera), ``bbox`` / ``ratio`` (row, col) as the reference's dataset
    emits them; ``inverse(pose)`` is computed once per image, in float64 with ``torch.linalg.inv_ex``.
    Nothing is read back from the device.  The set is append-only until :meth:`clear`; the device
    table of the maps (``oetr_covis_map[n]``) is written on the host into pinned memory and uploaded
    in ONE copy at the first use after an ``add``.  Memory: the maps themselves, 16 bytes of table
    and 360 bytes of camera per image.

    Streams: ``add`` uploads the map and the camera record on the stream that is current when it is
    called, and the first use after an ``add`` uploads the table on the stream of that use; nothing
    orders a LATER call on another stream behind those copies.  Fill and use the set on one stream,
    or synchronise (an event, ``torch.cuda.synchronize()``) between filling it on one stream and
    using it on another - as for :meth:`clear`, the ordering is the caller's."""

    def __init__(self, device=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError('a DepthSet needs a GPU (HIP) device and none is present. There is no CPU implementation.')
            device = torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'a DepthSet needs a GPU (HIP) device, got {device}. There is no CPU implementation.')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        self.clear()

    def clear(self):
        """Empty the set (slots are handed out from 0 again).  The caller sees to it that no call that
        reads the old maps is still in flight on another stream."""
        self._maps, self._records = [], []
        self._table = self._cameras = self._staged = None
        self.max_pixels = 0

    def __len__(self):
        return len(self._maps)

    def shape(self, slot):
        """(H, W) of the map in ``slot``."""
        return tuple(self._maps[slot].shape)

    @property
    def map_bytes(self):
        """Bytes of device memory the maps take."""
        return sum(m.numel() * 4 for m in self._maps)

    @torch.no_grad()
    def add(self, depth, intrinsics, pose, bbox=(0.0, 0.0), ratio=(1.0, 1.0)):
        """One image -> its slot number."""
        d = torch.as_tensor(depth)
        if d.dim() != 2 or not d.is_floating_point():
            raise ValueError(f'depth must be a floating-point [H,W] map, got {tuple(d.shape)} {d.dtype}')
        H, W = int(d.shape[0]), int(d.shape[1])
        if not (1 <= H <= COVIS_MAX_SIDE and 1 <= W <= COVIS_MAX_SIDE):
            raise ValueError(f'depth map sides must be in 1..{COVIS_MAX_SIDE}, got {H}x{W}')
        p = torch.as_tensor(pose)
        f64 = lambda t, n: torch.as_tensor(t).to(device=p.device, dtype=torch.float64).reshape(n)
        p = f64(p, (4, 4))
        inv = torch.linalg.inv_ex(p).inverse          # (inv_ex: no error check, so no synchronisation on a GPU)
        rec = torch.cat([p.reshape(16), inv.reshape(16), f64(intrinsics, 9), f64(bbox, 2), f64(ratio, 2)])
        self._maps.append(d.to(dtype=torch.float32).to(self.device, non_blocking=True).contiguous())
        self._records.append(rec.to(self.device, non_blocking=True))
        self._table = self._cameras = None
        self.max_pixels = max(self.max_pixels, H * W)
        return len(self._maps) - 1

    def _commit(self):
        """The device table and the camera records ``[n,45]`` of the set as it stands."""
        if self._table is None:
            n = len(self._maps)
            if n == 0:
                raise ValueError('the DepthSet is empty')
            rows = (_CovisMap * n)()
            for k, m in enumerate(self._maps):
                rows[k].depth, rows[k].H, rows[k].W = m.data_ptr(), int(m.shape[0]), int(m.shape[1])
            staged = torch.empty(n * C.sizeof(_CovisMap), dtype=torch.uint8).pin_memory()
            C.memmove(staged.data_ptr(), C.addressof(rows), n * C.sizeof(_CovisMap))
            with torch.cuda.device(self.device):
                self._table = staged.to(self.device, non_blocking=True)
                self._cameras = torch.stack(self._records)
            self._staged = staged       # pinned source of the asynchronous copy
        return self._table, self._cameras


def pair_params(depth_set, idx1, idx2):
    """The parameter blocks of the pairs ``(idx1[p], idx2[p])``: float64 ``[P,40]`` in the layout of
    ``covis.covis_params`` (``include/oetr_covis.h``), gathered from the set's camera records and
    multiplied on the device, no host read.  ``T = pose2 @ inverse(pose1)`` is summed in a fixed order
    by elementwise kernels (capturable, the same bits on every run).  An index outside the set takes
    a clamped record: the HIP call never dereferences such a pair."""
    _, cams = depth_set._commit()
    last = cams.shape[0] - 1
    r1 = cams.index_select(0, idx1.long().clamp(0, last))
    r2 = cams.index_select(0, idx2.long().clamp(0, last))
    n = r1.shape[0]
    A, B = r2[:, 0:16].view(n, 4, 4), r1[:, 16:32].view(n, 4, 4)
    term = lambda k: A[:, :, k, None] * B[:, None, k, :]
    T = ((term(0) + term(1)) + term(2)) + term(3)
    params = torch.zeros(n, COVIS_PARAM_DOUBLES, dtype=torch.float64, device=cams.device)
    params[:, 0:16] = T.reshape(n, 16)
    params[:, 16], params[:, 17], params[:, 18], params[:, 19] = r1[:, 32], r1[:, 36], r1[:, 34], r1[:, 37]
    params[:, 20:29] = r2[:, 32:41]
    params[:, 29:33] = r1[:, 41:45]
    params[:, 33:37] = r2[:, 41:45]
    return params


def covis_boxes_indexed(table, n_maps, max_pixels, idx1, idx2, params, out=None):
    """``oetr_covis_boxes_indexed`` on device tensors as they are: ``table`` the ``oetr_covis_map[n_maps]`` bytes,
    ``idx1`` / ``idx2`` contiguous int32 ``[P]``, ``params`` contiguous float64 ``[P,40]``, all on one GPU;
    ``max_pixels`` the largest ``H * W`` vouched for.  Enqueues on torch's current stream of that GPU and reads
    nothing back.  ``out``: the result dict of an earlier call with as many pairs, to write into again (its
    tensors and the workspace it carries as ``out['workspace']``)."""
    dev = table.device
    if dev.type != 'cuda':
        raise RuntimeError('covis_boxes_indexed needs its tensors on a GPU (HIP) device; there is no CPU implementation')
    n = int(idx1.shape[0])
    for name, t, dt, shape in (('idx1', idx1, torch.int32, (n,)), ('idx2', idx2, torch.int32, (n,)),
                               ('params', params, torch.float64, (n, COVIS_PARAM_DOUBLES))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'{name} must be a contiguous {dt} tensor of shape {shape} on {dev}')
    if table.dtype != torch.uint8 or not table.is_contiguous() or table.numel() < int(n_maps) * C.sizeof(_CovisMap):
        raise ValueError(f'table must hold {n_maps} records of {C.sizeof(_CovisMap)} bytes')
    if out is None:
        out = {'overlap_box1': torch.zeros(n, 4, device=dev), 'overlap_box2': torch.zeros(n, 4, device=dev),
               'overlap_valid': torch.zeros(n, dtype=torch.bool, device=dev),
               'overlap_count': torch.zeros(n, dtype=torch.int32, device=dev)}
    elif tuple(out['overlap_box1'].shape) != (n, 4):
        raise ValueError(f"`out` holds {out['overlap_box1'].shape[0]} pairs, the call has {n}")
    if n == 0:
        return out
    lib = hip_engine.load_library()
    workspace = _workspace(out, int(lib.oetr_covis_set_workspace_bytes(n)), dev)
    with torch.cuda.device(dev):
        _check(lib, lib.oetr_covis_boxes_indexed(
            table.data_ptr(), int(n_maps), idx1.data_ptr(), idx2.data_ptr(), params.data_ptr(), n, int(max_pixels),
            workspace.data_ptr(), workspace.numel(), out['overlap_box1'].data_ptr(), out['overlap_box2'].data_ptr(),
            out['overlap_valid'].data_ptr(), out['overlap_count'].data_ptr(), _stream(dev)), 'oetr_covis_boxes_indexed')
    return out


@torch.no_grad()
def overlap_boxes_indexed(depth_set, pair_index, out=None):
    """Co-visibility boxes of the pairs ``pair_index`` over ``depth_set``: entry p is what
    ``overlap_boxes_from_depth`` gives for map ``pair_index[p][0]`` against map ``pair_index[p][1]``,
    except that the two maps may differ in size (map 1 ``H1 x W1``, map 2 ``H2 x W2``; the landing
    test is ``0 <= i < W2, 0 <= j < H2``, the departure from the reference ``include/oetr_covis.h``
    documents for non-square maps).  ``pair_index``: a host sequence of ``(i, j)`` (``(i, i)`` is
    legal) or a device int32 ``[P,2]`` tensor.

    Returns device tensors ``overlap_box1`` / ``overlap_box2`` float32 ``[P,4]``, ``overlap_valid``
    bool ``[P]`` and ``overlap_count`` int32 ``[P]``.  A pair with an index outside the set is not
    computed: zero boxes, not valid, count -1.  Enqueues on torch's current stream of the set's device
    and reads nothing back, so it can be captured into a HIP graph - with a device ``pair_index`` a
    replay computes the pairs that tensor holds at replay time.  ``out``: the result of an earlier
    call with as many pairs, to write into again (it carries the call's workspace as
    ``out['workspace']``)."""
    dev = depth_set.device
    with torch.cuda.device(dev):
        pairs = _pair_tensor(dev, pair_index, pin=True)
        if pairs.shape[0] == 0:
            return covis_boxes_indexed(torch.empty(0, dtype=torch.uint8, device=dev), 0, 0, pairs[:, 0].contiguous(),
                                       pairs[:, 1].contiguous(), torch.empty(0, COVIS_PARAM_DOUBLES, dtype=torch.float64, device=dev), out)
        table, _ = depth_set._commit()
        idx1, idx2 = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
        return covis_boxes_indexed(table, len(depth_set), depth_set.max_pixels, idx1, idx2,
                                   pair_params(depth_set, idx1, idx2), out)


def select_pairs(box1, box2, valid, min_scale_diff=2.0, limit=None):
    """``oetr_covis_select`` on device tensors: ``box1`` / ``box2`` contiguous float32 ``[P,4]``, ``valid``
    bool or uint8 ``[P]``.  Returns ``kept`` int32 ``[P]`` (the kept pair numbers in ascending order, then
    -1), ``n_kept`` int32 ``[1]`` and ``scale_diff`` float64 ``[P]``, on the device; no host read."""
    dev = box1.device
    if dev.type != 'cuda':
        raise RuntimeError('select_pairs needs its tensors on a GPU (HIP) device; there is no CPU implementation')
    n = int(box1.shape[0])
    for name, t, dt, shape in (('box1', box1, (torch.float32,), (n, 4)), ('box2', box2, (torch.float32,), (n, 4)),
                               ('valid', valid, (torch.bool, torch.uint8), (n,))):
        if t.dtype not in dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'{name} must be a contiguous {dt[0]} tensor of shape {shape} on {dev}')
    res = {'kept': torch.full((n,), -1, dtype=torch.int32, device=dev),
           'n_kept': torch.zeros(1, dtype=torch.int32, device=dev),
           'scale_diff': torch.empty(n, dtype=torch.float64, device=dev)}
    if n == 0:
        return res
    lib = hip_engine.load_library()
    with torch.cuda.device(dev):
        _check(lib, lib.oetr_covis_select(
            box1.data_ptr(), box2.data_ptr(), valid.data_ptr(), n, float(min_scale_diff),
            0 if limit is None else int(limit), res['kept'].data_ptr(), res['n_kept'].data_ptr(),
            res['scale_diff'].data_ptr(), None, 0, _stream(dev)), 'oetr_covis_select')
    return res


@torch.no_grad()
def mine_pairs(depth_set, pair_index, min_scale_diff=2.0, limit=None):
    """The reference's pair mining (``src/utils/megadepth_preprocess.py:186-200``) over candidate pairs
    of a depth-map set: the boxes of every pair, and the pairs it keeps - boxes valid, both with a
    positive coordinate, and ``scale_diff > min_scale_diff`` (the larger of the width and the height
    ratio of the two boxes, either way round).  Returns the dict of :func:`overlap_boxes_indexed`
    plus ``kept`` int32 ``[P]`` (kept pair numbers in list order, cut at ``limit``, then -1),
    ``n_kept`` int32 ``[1]`` and ``scale_diff`` float64 ``[P]``, all on the device."""
    out = overlap_boxes_indexed(depth_set, pair_index)
    out.update(select_pairs(out['overlap_box1'], out['overlap_box2'], out['overlap_valid'], min_scale_diff, limit))
    return out
