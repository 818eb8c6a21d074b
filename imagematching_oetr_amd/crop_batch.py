"""The box -> crop step for a whole chunk of pairs in one device call.

``overlap_crop`` (``hip_engine.py``) hands ONE pair to the matcher per call, as the reference does
(``evaluation.py:82-170`` is hard-wired to ``bbox[0]``): three launches, five allocations and one
geometry read-back per pair.  ``overlap_crop_batch`` is the same step for n pairs of mixed image
sizes as one HIP call (``oetr_overlap_crop_batch``, ``include/oetr_crop_batch.h``; kernels
``csrc/crop_batch.hip``): two launches (three with ``size_divisor > 1``) whatever n is, no
allocation when an earlier result is handed back as ``out``, and ONE read for all n geometry
records.  Pair k of a call is what ``overlap_crop`` gives for that pair alone, bit for bit - both are
built on one copy of the arithmetic (``csrc/crop_sample.h``).  There is no CPU implementation.
"""
import ctypes as C

import numpy as np
import torch

from . import hip_engine
from .hip_engine import OetrError, _check, _CropInfo, _CropPair, _stream

_INFO_BYTES = C.sizeof(_CropInfo)


class CropPairTable:
    """The device table of a batched crop call (``oetr_crop_pair[n]``) and what the host knows about
    it: ``n``, ``channels``, ``max_h``, ``max_w``.  Keeps the images alive."""

    def __init__(self, table, images, n, channels, max_h, max_w):
        self.table, self.images = table, images
        self.n, self.channels, self.max_h, self.max_w = n, channels, max_h, max_w
        self.device = table.device

    def __len__(self):
        return self.n


def crop_pair_table(images0, images1, scales0, scales1):
    """The pair table of :func:`overlap_crop_batch`.  ``images0`` / ``images1``: lists of n
    ``[1,C,h,w]`` float32 device tensors with one C (sizes may differ; the same tensor may serve any
    number of pairs); ``scales0`` / ``scales1``: lists of n ``(sx, sy)`` ``overlap_scales``.  The table
    is written on the host into pinned memory and goes to the device in ONE copy."""
    n = len(images0)
    if n < 1 or not (len(images1) == len(scales0) == len(scales1) == n):
        raise ValueError('crop_pair_table: four lists of one length >= 1')
    dev = images0[0].device
    if dev.type != 'cuda':
        raise OetrError(f'crop_pair_table: the images must be GPU tensors (got {dev}); the crop step has no CPU implementation')
    rows = (_CropPair * n)()
    channels = int(images0[0].shape[1]) if images0[0].dim() == 4 else 0
    max_h = max_w = 0
    for k in range(n):
        for i, (im, sc) in enumerate(((images0[k], scales0[k]), (images1[k], scales1[k]))):
            if im.dim() != 4 or im.shape[0] != 1 or im.shape[1] != channels or im.dtype != torch.float32 \
                    or im.device != dev or not im.is_contiguous():
                raise ValueError(f'crop_pair_table: image{i} of pair {k} must be a contiguous float32 [1,{channels},h,w] on {dev}')
            rows[k].image[i] = im.data_ptr()
            rows[k].h[i], rows[k].w[i] = int(im.shape[2]), int(im.shape[3])
            rows[k].scale[i][0], rows[k].scale[i][1] = float(sc[0]), float(sc[1])
            max_h, max_w = max(max_h, int(im.shape[2])), max(max_w, int(im.shape[3]))
    staged = torch.empty(n * C.sizeof(_CropPair), dtype=torch.uint8).pin_memory()
    C.memmove(staged.data_ptr(), C.addressof(rows), n * C.sizeof(_CropPair))
    table = staged.to(dev, non_blocking=True)
    res = CropPairTable(table, (list(images0), list(images1)), n, channels, max_h, max_w)
    res._staged = staged        # pinned source of the asynchronous copy
    return res


def keypoints_to_origin(kpts, ratio, bbox, scales):
    """Keypoints found in a crop, in the coordinates of the original picture: the reference's
    ``(pred['keypoints'] / ratio + pred['bbox'][:2]) * scales`` (``dloc/core/overlap_features.py:123-127``)
    with its dtypes - float32 keypoints ``[K,2]`` / the float32 ``[1,2]`` ratio + float32 ``bbox[:2]``,
    times a pair of Python floats, which makes the result float64.  Host arithmetic only."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    k = as_np(kpts).astype(np.float32, copy=False)
    r = as_np(ratio).astype(np.float32).reshape(1, 2)
    b = as_np(bbox).astype(np.float32).reshape(-1)
    return (k / r + b[:2]) * (float(scales[0]), float(scales[1]))


class OverlapCropBatch:
    """Result of :func:`overlap_crop_batch`: the output slots and the n geometry records, all on the
    device.  Nothing has touched the host yet; :meth:`geometry` reads all n records back in ONE copy
    (which synchronises the stream) and keeps them - do it when the crops are about to be consumed."""

    def __init__(self, table, out, tmp, info, capacity, params):
        self._table, self._out, self._tmp, self.info = table, out, tmp, info
        self._capacity, self._params, self._geo = capacity, params, None

    def __len__(self):
        return self._table.n

    def geometry(self, refresh=False):
        """The n ``oetr_crop_info`` records (a ctypes array), read once; ``refresh``: read them again
        (after the replay of a graph that holds the call)."""
        if self._geo is None or refresh:
            raw = self.info.cpu().numpy().tobytes()[:len(self) * _INFO_BYTES]
            self._geo = (_CropInfo * len(self)).from_buffer_copy(raw)
        return self._geo

    @property
    def valid(self):
        """Per pair: 1 - crops were made; 0 - the gate failed and the full images passed through;
        -1 - no crops, nothing written: a box outside the domain (a scaled coordinate that does not
        truncate into [0, 2^31): negative, NaN, infinite; ``include/oetr_hip.h``), an empty crop, or one
        the call's bounds do not cover."""
        return [int(g.valid) for g in self.geometry()]

    def crop(self, k, i):
        """``[1, C, out_h, out_w]`` view of pair ``k``'s image ``i`` (the reference's ``left[None]``)."""
        g = self.geometry()[k]
        if int(g.valid) < 0:
            raise OetrError(f'overlap_crop_batch: pair {k} has a box outside the domain (negative, non-finite or huge '
                            'after scaling), a degenerate crop rectangle or one larger than the capacity '
                            '(oetr_crop_info.valid == -1)')
        c, h, w = self._table.channels, int(g.out_h[i]), int(g.out_w[i])
        return self._out[k, i, :c * h * w].view(1, c, h, w)

    def bbox(self, k, i):
        """The reference's ``pred['bbox0'/'bbox1']`` of pair ``k``: the scaled float box, [1, 4]."""
        return torch.tensor([list(self.geometry()[k].sbox[i])], dtype=torch.float32)

    def ratio(self, k, i):
        """The reference's ``ratio0/ratio1`` = [[rx, ry]] (Python floats) of pair ``k``."""
        g = self.geometry()[k]
        return [[float(g.ratio[i][0]), float(g.ratio[i][1])]]

    def to_origin(self, k, i, kpts, scales):
        """:func:`keypoints_to_origin` with pair ``k``'s ratio and box of side ``i``; ``scales``: the
        reader's ``scales0`` / ``scales1`` of that picture."""
        return keypoints_to_origin(kpts, torch.tensor(self.ratio(k, i)), self.bbox(k, i)[0], scales)


def overlap_crop_batch(table, box0, box1, keep_aspect=True, size_divisor=1, pragueparks=False, out=None):
    """``oetr_overlap_crop_batch`` on a :func:`crop_pair_table`: ``box0`` / ``box1`` contiguous float32
    ``[n,4]`` on the table's device (``forward_dummy``'s outputs as they are), the modes as for
    ``overlap_crop``.  Enqueues on torch's current stream of that device and reads nothing back, so it
    can be captured into a HIP graph.  ``out``: an earlier result of the same table and modes, to write
    into again - then nothing is allocated; without it the output slots, the scratch (only with
    ``size_divisor > 1``) and the records are allocated once for the call.
    Returns an :class:`OverlapCropBatch`."""
    for name, t in (('table', table.table), ('box0', box0), ('box1', box1)):
        if not t.is_cuda:
            raise OetrError(f'overlap_crop_batch: {name} must be a GPU tensor (got {t.device}); the crop step '
                            'has no CPU implementation')
    dev, n = table.device, table.n
    for name, b in (('box0', box0), ('box1', box1)):
        if b.dtype != torch.float32 or tuple(b.shape) != (n, 4) or not b.is_contiguous() or b.device != dev:
            raise ValueError(f'overlap_crop_batch: {name} must be a contiguous float32 [{n},4] on {dev}')
    d = int(size_divisor)
    params = (int(bool(keep_aspect)), d, int(bool(pragueparks)))
    lib = hip_engine.load_library()
    cap = int(lib.oetr_crop_batch_capacity(table.channels, table.max_h, table.max_w, d, None, None))
    if cap == 0:
        raise ValueError('overlap_crop_batch: invalid crop arguments')
    if out is None:
        out = OverlapCropBatch(table, torch.empty(n, 2, cap, device=dev),
                               torch.empty(n, 2, cap, device=dev) if d > 1 else None,
                               torch.zeros(n, (_INFO_BYTES + 7) // 8, dtype=torch.float64, device=dev), cap, params)
    elif out._table is not table or out._params != params:
        raise ValueError('overlap_crop_batch: `out` must be an earlier result of the same table and modes')
    out._geo = None
    with torch.cuda.device(dev):
        _check(lib, lib.oetr_overlap_crop_batch(
            table.table.data_ptr(), n, table.channels, table.max_h, table.max_w, box0.data_ptr(), box1.data_ptr(),
            params[0], d, params[2], None if out._tmp is None else out._tmp.data_ptr(), out._out.data_ptr(),
            out._capacity, out.info.data_ptr(), _stream(dev)), 'oetr_overlap_crop_batch')
    out._keep = (box0, box1)        # inputs stay alive until the work has run
    return out
