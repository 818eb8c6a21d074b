"""Descriptor sets matched by nearest neighbours on the device, for a whole pair list per call.

``assemble_matches`` starts from a matcher's ``matches0``.  The reference's own matcher is
``dloc/core/matchers/nearest_neighbor.py`` (``find_nn``, ``mutual_check``, ``NearestNeighbor``):
``sim = einsum('bdn,bdm->bnm')``, ``topk(2)`` per row and per column, the ratio test and the distance
threshold on ``2 * (1 - sim)``, the mutual check.  :func:`match_descriptors` does that for every pair of
a call in one HIP call (``oetr_nn_match``, ``include/oetr_nn_match.h``, ``csrc/nn_match.hip``) that never
stores a similarity matrix, and returns ``matches0`` / ``matching_scores0`` in the joined form
``assemble_matches`` takes as they are.  The arithmetic is the numpy specification of DESIGN 9.3k,
reproduced bit for bit: the similarity is one float32 ``fmaf`` chain over ascending ``d``, a tied maximum
goes to the LOWEST index (torch's ``topk`` leaves it open), and a side of one row passes the ratio test
(the reference's ``topk(2)`` raises there).  There is no CPU implementation.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import numpy as np
import torch

from . import hip_engine
from ._inputs import (_device_of, _host_names, _is_host, _offsets_of, _ptr, _refuse_float64,
                      _refuse_host_inputs_in_capture, _upload)
from .hip_engine import (NN_MATCH_COUNTERS, NN_MATCH_DISTANCE, NN_MATCH_MAX_D, NN_MATCH_MIN_D, NN_MATCH_MUTUAL,
                         NN_MATCH_RATIO, _check, _stream)


def _squared(threshold):
    """``threshold ** 2`` formed in double and rounded to float32 once; ``None`` or 0: the test is off, as the
    reference's ``if ratio_thresh:``."""
    return float(np.float32(float(threshold) * float(threshold))) if threshold else None


def _as_tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


def _descriptors(name, x, dev, channels_first):
    """``x`` -> contiguous float32 ``[K,D]`` on ``dev`` whose rows start on 16 bytes; float16 widened; a host array is
    uploaded (blocking); ``channels_first``: ``x`` is ``[D,K]``."""
    x = _as_tensor(x)
    if x.dtype not in (torch.float32, torch.float16):
        raise ValueError(f'{name} must be float32 or float16, got {x.dtype}')
    if x.dim() != 2:
        raise ValueError(f"{name} must be {'[D,K]' if channels_first else '[K,D]'}, got {tuple(x.shape)}")
    if x.is_cuda and x.device != dev:
        raise ValueError(f'{name} is on {x.device}, the other descriptors on {dev}')
    x = (x.t() if channels_first else x).to(device=dev, dtype=torch.float32).contiguous()
    return x.clone() if x.data_ptr() % 16 else x


@torch.no_grad()
def match_descriptors(desc0, desc1, offsets0=None, offsets1=None, ratio_threshold=None, distance_threshold=None,
                      do_mutual_check=True, max_k0=None, max_k1=None, channels_first=False, out=None):
    """Nearest-neighbour matches of all pairs of a call, in one device call.

    Descriptors come in one of the two forms ``assemble_matches`` takes for keypoints:

    * joined, with ``offsets0`` / ``offsets1``: ``desc0`` ``[N0,D]``, ``desc1`` ``[N1,D]`` and device int32
      ``[P+1]`` non-decreasing offsets; side ``i`` of pair ``p`` owns rows ``offsets_i[p] .. offsets_i[p+1]-1``.
      This is the form a graph can capture.  ``max_k0`` / ``max_k1`` are then required: the largest
      per-pair row counts the caller vouches for (they size the grid; nothing is read back to find them).
      A pair with more rows is not matched: its counters read four ``-1``, its rows ``-1`` / ``0``;
    * sequences with one tensor per pair, ``desc0[p]`` ``[K0_p,D]`` and ``desc1[p]`` ``[K1_p,D]``: the lengths
      and ``max_k*`` come from the shapes, the tensors are joined on the device.

    ``channels_first=True``: every tensor is ``[D,K]``, the reference's layout.  Descriptors are float32
    (float16 is widened; float64 is refused); ``D % 4 == 0`` and ``4 <= D <= 512``.  ``ratio_threshold`` /
    ``distance_threshold``: ``None`` or 0 switch the test off.

    Returns a dict of device tensors: ``matches0`` int32 ``[N0]`` (row ``a`` of pair ``p``: an index within
    side 1 of pair ``p``, or ``-1``), ``matching_scores0`` float32 ``[N0]`` (direction 0's scores BEFORE the
    mutual check, as the reference returns them), ``matches1`` int32 ``[N1]`` (direction 1 before any mutual
    check) and ``counts`` int32 ``[P,4]``: ``K0``, ``K1``, rows of side 0 that pass ``find_nn``, rows matched
    after the mutual check; :func:`match_counts` reads them.  Rows no pair owns read ``-1`` / ``0``.

    ``assemble_matches(crops, scales, kp0, kp1, res['matches0'], res['matching_scores0'], offsets0=...,
    offsets1=...)`` takes the result as it is.  Enqueues on torch's current stream of the descriptors'
    device and reads nothing back.  ``out``: the result of an earlier call of the same sizes, written into
    again with no allocation."""
    joined = torch.is_tensor(desc0) or isinstance(desc0, np.ndarray)
    if joined:
        if offsets0 is None or offsets1 is None:
            raise ValueError('joined descriptors need `offsets0` and `offsets1` (int32 [P+1]); or give one tensor per '
                             'pair')
        if max_k0 is None or max_k1 is None:
            raise ValueError('joined descriptors need `max_k0` and `max_k1`: the largest per-pair row counts you vouch '
                             'for (nothing is read back to find them)')
        parts0, parts1 = [desc0], [desc1]
    else:
        if offsets0 is not None or offsets1 is not None:
            raise ValueError('`offsets0` / `offsets1` go with joined descriptors, not with one tensor per pair')
        parts0, parts1 = list(desc0), list(desc1)
        if not parts0 or len(parts0) != len(parts1):
            raise ValueError('desc0 and desc1 must hold one tensor per pair')
    for name, parts in (('desc0', parts0), ('desc1', parts1)):
        for t in parts:
            _refuse_float64(name, t)
    dev = _device_of('match_descriptors', parts0 + parts1 + [offsets0, offsets1])
    host_inputs = _host_names([('offsets0', offsets0), ('offsets1', offsets1)])
    host_inputs += [n for n, parts in (('desc0', parts0), ('desc1', parts1)) if any(_is_host(t) for t in parts)]
    if not joined:
        host_inputs.append('per-pair lengths')
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        parts0 = [_descriptors('desc0', t, dev, channels_first) for t in parts0]
        parts1 = [_descriptors('desc1', t, dev, channels_first) for t in parts1]
        D = int(parts0[0].shape[1])
        if any(int(t.shape[1]) != D for t in parts0 + parts1):
            raise ValueError('every descriptor tensor must have the same D')
        if D % 4 or not NN_MATCH_MIN_D <= D <= NN_MATCH_MAX_D:
            raise ValueError(f'need D % 4 == 0 and {NN_MATCH_MIN_D} <= D <= {NN_MATCH_MAX_D}, got D = {D}')
        if joined:
            desc0, desc1 = parts0[0], parts1[0]
            P = int(offsets0.shape[0] if hasattr(offsets0, 'shape') else len(offsets0)) - 1
            offsets0 = _upload('offsets0', offsets0, torch.int32, (P + 1,), dev)
            offsets1 = _upload('offsets1', offsets1, torch.int32, (P + 1,), dev)
        else:
            len0, len1 = [int(t.shape[0]) for t in parts0], [int(t.shape[0]) for t in parts1]
            desc0, desc1 = torch.cat(parts0), torch.cat(parts1)
            P = len(len0)
            offsets0, offsets1 = _offsets_of(len0, dev), _offsets_of(len1, dev)
            max_k0 = max(len0) if max_k0 is None else max_k0
            max_k1 = max(len1) if max_k1 is None else max_k1
        if P < 1:
            raise ValueError('match_descriptors needs at least one pair')
        N0, N1 = int(desc0.shape[0]), int(desc1.shape[0])
        if max(N0, N1) > 2 ** 31 - 1:
            raise ValueError('more than 2^31 - 1 descriptors on a side in one call')
        ratio_sq, distance_sq = _squared(ratio_threshold), _squared(distance_threshold)
        flags = ((NN_MATCH_RATIO if ratio_sq is not None else 0) | (NN_MATCH_DISTANCE if distance_sq is not None else 0)
                 | (NN_MATCH_MUTUAL if do_mutual_check else 0))
        if out is None:
            i32 = dict(dtype=torch.int32, device=dev)
            out = {'matches0': torch.empty(N0, **i32), 'matching_scores0': torch.empty(N0, device=dev),
                   'matches1': torch.empty(N1, **i32), 'counts': torch.empty(P, NN_MATCH_COUNTERS, **i32)}
        elif (tuple(out['matches0'].shape) != (N0,) or tuple(out['matches1'].shape) != (N1,)
              or tuple(out['counts'].shape) != (P, NN_MATCH_COUNTERS) or out['matches0'].device != dev):
            raise ValueError('`out` is the result of a call of other sizes (descriptors, pairs)')
        lib = hip_engine.load_library()
        _check(lib, lib.oetr_nn_match(
            _ptr(desc0), offsets0.data_ptr(), N0, _ptr(desc1), offsets1.data_ptr(), N1, P, D, int(max_k0), int(max_k1),
            ratio_sq or 0.0, distance_sq or 0.0, flags, None, 0, _ptr(out['matches0']), _ptr(out['matching_scores0']),
            _ptr(out['matches1']), out['counts'].data_ptr(), _stream(dev)), 'oetr_nn_match')
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = (desc0, desc1, offsets0, offsets1)
    return out


def match_counts(result):
    """The counters of a :func:`match_descriptors` result as a host int32 array ``[P,4]`` - ``K0``, ``K1``, rows of
    side 0 that pass ``find_nn``, rows matched after the mutual check; four ``-1`` for a pair beyond ``max_k*``.  ONE
    read, which synchronises the stream."""
    return result['counts'].cpu().numpy()
