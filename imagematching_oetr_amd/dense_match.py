"""Dense feature grids matched by a dual softmax on the device, for a whole pair list per call.

The reference's ``direct`` branch hands the two crops to a detector-free matcher (``dloc/core/matchers/loftr.py``)
whose coarse matching head works on two 1/8-resolution feature grids: a similarity matrix, a softmax along both axes,
a threshold, border removal and the mutual-maximum test.  :func:`match_dense` does that head for every pair of a call
in one HIP call (``oetr_dual_softmax_match``, ``include/oetr_dual_softmax.h``, ``csrc/dual_softmax.hip``) that never
stores a similarity or confidence matrix, and returns ``keypoints0`` / ``keypoints1`` / ``matches0`` /
``matching_scores0`` in the joined form ``assemble_matches`` takes as they are.  The network that makes the grids stays
torch.  The arithmetic is the numpy specification of DESIGN 9.3o, reproduced bit for bit: the project's own statement,
modelled on LoFTR's published coarse matching; that code lives in a ``third_party/`` tree outside the reference
checkout, so no parity with it is claimed.  There is no CPU implementation.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import math

import numpy as np
import torch

from . import hip_engine
from ._inputs import (_device_of, _host_names, _is_host, _offsets_of, _ptr, _refuse_float64,
                      _refuse_host_inputs_in_capture, _upload, _workspace)
from .hip_engine import DUAL_SOFTMAX_COUNTERS, DUAL_SOFTMAX_MAX_D, DUAL_SOFTMAX_MIN_D, _check, _stream

_OUTPUTS = ('matches0', 'matching_scores0', 'matches1', 'keypoints0', 'keypoints1', 'counts')


def _as_tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


def _rows(name, x, dev):
    """Joined token rows -> contiguous float32 ``[N,D]`` on ``dev`` whose rows start on 16 bytes."""
    x = _as_tensor(x)
    if x.dtype != torch.float32:
        raise ValueError(f'{name} must be float32, got {x.dtype}')
    if x.dim() != 2:
        raise ValueError(f'{name} must be [N,D] token rows, got {tuple(x.shape)}')
    if x.is_cuda and x.device != dev:
        raise ValueError(f'{name} is on {x.device}, the other features on {dev}')
    x = x.to(dev).contiguous()
    return x.clone() if x.data_ptr() % 16 else x


def _map_rows(name, x, dev, channels_first):
    """One map ``[h,w,D]`` (``[D,h,w]`` with ``channels_first``) -> its token rows in raster order and ``(h, w)``."""
    x = _as_tensor(x)
    if x.dtype != torch.float32:
        raise ValueError(f'{name} must be float32, got {x.dtype}')
    if x.dim() != 3:
        raise ValueError(f"{name} must be {'[D,h,w]' if channels_first else '[h,w,D]'}, got {tuple(x.shape)}")
    if x.is_cuda and x.device != dev:
        raise ValueError(f'{name} is on {x.device}, the other features on {dev}')
    x = (x.permute(1, 2, 0) if channels_first else x).to(dev)
    h, w, D = (int(v) for v in x.shape)
    return x.reshape(h * w, D), (h, w)


@torch.no_grad()
def match_dense(feat0, feat1, offsets0=None, offsets1=None, grids0=None, grids1=None, temperature=0.1, threshold=0.2,
                border_rm=2, cell=8, max_k0=None, max_k1=None, channels_first=False, out=None):
    """Dual-softmax matches of the coarse feature grids of all pairs of a call, in one device call.

    Features come in one of the two forms ``match_descriptors`` takes:

    * joined token rows with ``offsets0`` / ``offsets1``: ``feat0`` ``[N0,D]``, ``feat1`` ``[N1,D]``, device int32
      ``[P+1]`` non-decreasing offsets and ``grids0`` / ``grids1`` int32 ``[P,2]`` = ``(h, w)`` with ``h * w`` the pair's
      row count on that side; the tokens of a grid are in raster order.  This is the form a graph can capture.
      ``max_k0`` / ``max_k1`` are then required: the largest per-pair row counts the caller vouches for (they size
      the grid; nothing is read back to find them).  A pair with more rows, or whose grid does not multiply to its
      rows, is not matched and never dereferenced: its counters read four ``-1``, its rows ``-1`` / ``0`` / NaN;
    * sequences with one map per pair and side, ``feat0[p]`` ``[h0_p,w0_p,D]`` (``[D,h,w]`` with
      ``channels_first=True``): grids, lengths and ``max_k*`` come from the shapes, the rows are joined on the device.

    Features are float32 (float64 is refused); ``D % 4 == 0`` and ``4 <= D <= 512``.  Pairs of one call may have
    different grids on the two sides and from pair to pair.  ``temperature > 0``: the similarity is divided by
    ``D * temperature`` - as ONE float32 factor ``float32(1 / (D * temperature))``; ``threshold >= 0``; ``border_rm``
    cells at every edge of either grid match nothing; ``cell``: the pixels per token of the keypoints.

    Returns a dict of device tensors: ``matches0`` int32 ``[N0]`` (token ``a`` of pair ``p``: an index within side 1 of
    pair ``p``, or ``-1``), ``matching_scores0`` float32 ``[N0]`` (the row's maximum confidence BEFORE the tests, 0
    without a candidate - as ``match_descriptors``' scores come from before the mutual check), ``matches1`` int32
    ``[N1]`` (direction 1's argmax before the tests), ``keypoints0`` / ``keypoints1`` float32 ``[N,2]`` =
    ``(col * cell, row * cell)`` of every token, and ``counts`` int32 ``[P,4]``: ``L``, ``S``, rows over the threshold
    and off the border, rows matched; :func:`dense_match_counts` reads them.  Rows no pair owns read ``-1`` / ``0`` /
    NaN.

    ``assemble_matches(crops, scales, res['keypoints0'], res['keypoints1'], res['matches0'],
    res['matching_scores0'], offsets0=..., offsets1=...)`` takes the result as it is.  Enqueues on torch's current
    stream of the features' device and reads nothing back.  ``out``: the result of an earlier call of the same sizes,
    written into again with no allocation (it carries the call's workspace)."""
    temperature, threshold = float(temperature), float(threshold)
    if not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f'need a finite temperature > 0, got {temperature}')
    if not (math.isfinite(threshold) and threshold >= 0):
        raise ValueError(f'need a finite threshold >= 0, got {threshold}')
    if int(border_rm) != border_rm or border_rm < 0:
        raise ValueError(f'need an integer border_rm >= 0, got {border_rm}')
    if int(cell) != cell or cell < 1:
        raise ValueError(f'need an integer cell >= 1, got {cell}')
    joined = torch.is_tensor(feat0) or isinstance(feat0, np.ndarray)
    if joined:
        if offsets0 is None or offsets1 is None:
            raise ValueError('joined token rows need `offsets0` and `offsets1` (int32 [P+1]); or give one map per pair')
        if grids0 is None or grids1 is None:
            raise ValueError('joined token rows need `grids0` and `grids1` (int32 [P,2] = (h, w))')
        if max_k0 is None or max_k1 is None:
            raise ValueError('joined token rows need `max_k0` and `max_k1`: the largest per-pair row counts you vouch '
                             'for (nothing is read back to find them)')
        parts0, parts1 = [feat0], [feat1]
    else:
        if any(x is not None for x in (offsets0, offsets1, grids0, grids1)):
            raise ValueError('`offsets0` / `offsets1` / `grids0` / `grids1` go with joined token rows, not with one map '
                             'per pair')
        parts0, parts1 = list(feat0), list(feat1)
        if not parts0 or len(parts0) != len(parts1):
            raise ValueError('feat0 and feat1 must hold one map per pair')
    for name, parts in (('feat0', parts0), ('feat1', parts1)):
        for t in parts:
            _refuse_float64(name, t)
    dev = _device_of('match_dense', parts0 + parts1 + [offsets0, offsets1, grids0, grids1])
    host_inputs = _host_names([('offsets0', offsets0), ('offsets1', offsets1), ('grids0', grids0), ('grids1', grids1)])
    host_inputs += [n for n, parts in (('feat0', parts0), ('feat1', parts1)) if any(_is_host(t) for t in parts)]
    if not joined:
        host_inputs.append('per-pair grids')
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        if joined:
            feat0, feat1 = _rows('feat0', feat0, dev), _rows('feat1', feat1, dev)
            P = int(offsets0.shape[0] if hasattr(offsets0, 'shape') else len(offsets0)) - 1
            offsets0 = _upload('offsets0', offsets0, torch.int32, (P + 1,), dev)
            offsets1 = _upload('offsets1', offsets1, torch.int32, (P + 1,), dev)
            grids0 = _upload('grids0', grids0, torch.int32, (P, 2), dev)
            grids1 = _upload('grids1', grids1, torch.int32, (P, 2), dev)
        else:
            maps0 = [_map_rows('feat0', t, dev, channels_first) for t in parts0]
            maps1 = [_map_rows('feat1', t, dev, channels_first) for t in parts1]
            feat0 = _rows('feat0', torch.cat([r for r, _ in maps0]), dev)
            feat1 = _rows('feat1', torch.cat([r for r, _ in maps1]), dev)
            P = len(maps0)
            len0, len1 = [g[0] * g[1] for _, g in maps0], [g[0] * g[1] for _, g in maps1]
            offsets0, offsets1 = _offsets_of(len0, dev), _offsets_of(len1, dev)
            grids0 = torch.as_tensor(np.array([g for _, g in maps0], np.int32).reshape(P, 2)).to(dev)
            grids1 = torch.as_tensor(np.array([g for _, g in maps1], np.int32).reshape(P, 2)).to(dev)
            max_k0 = max(len0) if max_k0 is None else max_k0
            max_k1 = max(len1) if max_k1 is None else max_k1
        if P < 1:
            raise ValueError('match_dense needs at least one pair')
        D = int(feat0.shape[1])
        if int(feat1.shape[1]) != D:
            raise ValueError('every feature tensor must have the same D')
        if D % 4 or not DUAL_SOFTMAX_MIN_D <= D <= DUAL_SOFTMAX_MAX_D:
            raise ValueError(f'need D % 4 == 0 and {DUAL_SOFTMAX_MIN_D} <= D <= {DUAL_SOFTMAX_MAX_D}, got D = {D}')
        N0, N1 = int(feat0.shape[0]), int(feat1.shape[0])
        if max(N0, N1) > 2 ** 31 - 1:
            raise ValueError('more than 2^31 - 1 tokens on a side in one call')
        scale = float(np.float32(1.0 / (D * temperature)))
        if out is None:
            i32 = dict(dtype=torch.int32, device=dev)
            out = {'matches0': torch.empty(N0, **i32), 'matching_scores0': torch.empty(N0, device=dev),
                   'matches1': torch.empty(N1, **i32), 'keypoints0': torch.empty(N0, 2, device=dev),
                   'keypoints1': torch.empty(N1, 2, device=dev), 'counts': torch.empty(P, DUAL_SOFTMAX_COUNTERS, **i32)}
        elif (tuple(out['matches0'].shape) != (N0,) or tuple(out['matches1'].shape) != (N1,)
              or tuple(out['counts'].shape) != (P, DUAL_SOFTMAX_COUNTERS) or out['matches0'].device != dev):
            raise ValueError('`out` is the result of a call of other sizes (tokens, pairs)')
        lib = hip_engine.load_library()
        need = int(lib.oetr_dual_softmax_workspace_bytes(N0, N1))
        workspace = _workspace(out, max(need, 1), dev)
        _check(lib, lib.oetr_dual_softmax_match(
            _ptr(feat0), offsets0.data_ptr(), grids0.data_ptr(), N0, _ptr(feat1), offsets1.data_ptr(),
            grids1.data_ptr(), N1, P, D, int(max_k0), int(max_k1), scale, threshold, int(border_rm), int(cell),
            workspace.data_ptr(), need, _ptr(out['matches0']), _ptr(out['matching_scores0']), _ptr(out['matches1']),
            _ptr(out['keypoints0']), _ptr(out['keypoints1']), out['counts'].data_ptr(), _stream(dev)),
            'oetr_dual_softmax_match')
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = (feat0, feat1, offsets0, offsets1, grids0, grids1)
    return out


def dense_match_counts(result):
    """The counters of a :func:`match_dense` result as a host int32 array ``[P,4]`` - ``L``, ``S``, rows over the
    threshold and off the border, rows matched; four ``-1`` for a pair that was not matched (beyond ``max_k*``, or a
    grid that does not multiply to its rows).  ONE read, which synchronises the stream."""
    return result['counts'].cpu().numpy()
