"""Scoring matches against depth and pose on the device, by index over a depth-map set.

The chain boxes -> crops -> matcher -> ``keypoints_to_origin`` is judged by whether its matches are
correct: the reference's ``validation_error`` / ``compute_epipolar_error`` (thresholded at 5e-4),
``get_episym`` and ``pose_evaluate`` -> ``get_projected_kp`` / ``get_truesym``.
:func:`score_matches` computes those for MANY match lists - one per pair of a pair list over a
:class:`~imagematching_oetr_amd.covis_set.DepthSet` - in one HIP call that reads the depth maps in
place (``oetr_match_score``, ``include/oetr_match_score.h``, ``csrc/match_score.hip``): per match
four float64 values and a flag byte, per pair five counters.  The arithmetic is the float64
specification of DESIGN 9.3e (the numpy restatement the tests hold), reproduced bit for bit.  There
is no CPU implementation.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import math

import torch

from . import hip_engine
from ._inputs import (_host_names, _match_keypoints, _match_list_args, _match_offsets, _pair_blocks, _pair_tensor,
                      _ptr, _refuse_host_inputs_in_capture)
from .covis_set import pair_params
from .hip_engine import MATCH_SCORE_COUNTERS, _check, _stream

FLAG_DEPTH1, FLAG_DEPTH2, FLAG_EPI, FLAG_EPISYM, FLAG_REPROJ = 1, 2, 4, 8, 16
VALUES = ('epi_ref', 'episym', 'reproj12_sq', 'reproj21_sq')


def match_params(depth_set, idx1, idx2):
    """The parameter blocks of the pairs ``(idx1[p], idx2[p])`` for :func:`score_matches`: float64
    ``[P,20]`` on the set's device - ``fx fy cx cy`` of camera 1, of camera 2, ``R`` (row major) and
    ``t`` of ``T_1to2`` - sliced out of ``covis_set.pair_params`` (the one copy of the
    ``pose2 @ inverse(pose1)`` product).  No host read."""
    full = pair_params(depth_set, idx1, idx2)
    n = full.shape[0]
    T = full[:, 0:16].view(n, 4, 4)
    K2 = full[:, 20:29]
    return torch.cat([full[:, 16:20], K2[:, 0:1], K2[:, 4:5], K2[:, 2:3], K2[:, 5:6],
                      T[:, :3, :3].reshape(n, 9), T[:, :3, 3]], dim=1).contiguous()


@torch.no_grad()
def score_matches(depth_set, pair_index, k1, k2, lengths=None, offsets=None, params=None, epi_thr=5e-4, sym_thr=None,
                  px_thr=None, values=True, out=None):
    """Score the match lists of the pairs ``pair_index`` over ``depth_set``, all in one device call.

    ``pair_index``: a host sequence of ``(i, j)`` or a device int32 ``[P,2]`` tensor.  ``k1`` / ``k2``:
    the lists concatenated, ``[M,2]`` ``(u, v)`` in the ORIGINAL pictures (what ``keypoints_to_origin``
    returns), float32 or float16 (widened; exact) - device tensors are taken as they are, host arrays
    are uploaded; float64 is refused.  Exactly one of ``lengths`` (a host sequence, one length per
    pair, summing to ``M``) and ``offsets`` (a device int32 ``[P+1]`` tensor: list p is the rows
    ``offsets[p] .. offsets[p+1]-1``; non-decreasing; rows outside every list are left unscored).
    ``params``: float64 ``[P,20]`` blocks (``match_params``'s layout); ``None``: ``match_params`` of the
    set's cameras.  ``epi_thr`` / ``sym_thr`` / ``px_thr``: ``None`` switches that threshold off.

    Returns a dict of device tensors: ``epi_ref``, ``episym``, ``reproj12_sq``, ``reproj21_sq`` (views
    of ``values``, one float64 ``[4,M]`` tensor; absent with ``values=False``), ``flags`` uint8
    ``[M]`` (1: depth under keypoint 1, 2: under keypoint 2, 4: ``epi_ref < epi_thr``, 8:
    ``episym < sym_thr``, 16: both depths and ``reproj21_sq < px_thr^2``) and ``counts`` int32
    ``[P,5]`` (matches, epi, episym, both depths, reproj; -1 for a threshold that is off).  A pair with
    an index outside the set is not scored: flags 0, NaN values, all five counters -1.

    Enqueues on torch's current stream of the set's device and reads nothing back, so it can be
    captured into a HIP graph when every input is a device tensor (a replay scores what the keypoint,
    offset, index and parameter tensors hold at replay time); use the set once before the capture, so
    that its table is uploaded outside it.  ``out``: the result of an earlier call
    of the same sizes, written into again with no allocation."""
    _match_list_args(k1, k2, lengths, offsets)
    dev = torch.device(depth_set.device)
    if dev.type != 'cuda':
        raise RuntimeError(f'score_matches needs a depth-map set on a GPU (HIP) device, got {dev}. There is no CPU '
                           'implementation.')
    host_inputs = _host_names((('pair_index', pair_index), ('k1', k1), ('k2', k2), ('offsets', offsets),
                               ('params', params)), lengths)
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        k1, k2, M = _match_keypoints(k1, k2, dev, 'depth-map set')
        pair_index = _pair_tensor(dev, pair_index)
        P = int(pair_index.shape[0])
        offsets = _match_offsets(lengths, offsets, P, M, dev)
        if out is None:
            out = {'flags': torch.zeros(M, dtype=torch.uint8, device=dev),
                   'counts': torch.zeros(P, MATCH_SCORE_COUNTERS, dtype=torch.int32, device=dev)}
            if values:
                out['values'] = torch.full((len(VALUES), M), math.nan, dtype=torch.float64, device=dev)
                out.update({name: out['values'][k] for k, name in enumerate(VALUES)})
        elif (tuple(out['flags'].shape) != (M,) or tuple(out['counts'].shape) != (P, MATCH_SCORE_COUNTERS)
              or ('values' in out) != bool(values)):
            raise ValueError('`out` is the result of a call of other sizes (matches, pairs, values)')
        if P == 0:                                   # nothing to score: every row is outside every list
            out['flags'].zero_()
            if values:
                out['values'].fill_(math.nan)
            return out
        idx1, idx2, table, params = _pair_blocks(depth_set, pair_index, params, match_params)
        thr = [math.nan if t is None else float(t) for t in (epi_thr, sym_thr, px_thr)]
        lib = hip_engine.load_library()
        _check(lib, lib.oetr_match_score(
            table.data_ptr(), len(depth_set), idx1.data_ptr(), idx2.data_ptr(), params.data_ptr(), offsets.data_ptr(), P,
            _ptr(k1), _ptr(k2), M, thr[0], thr[1], thr[2], _ptr(out['values']) if values else None, _ptr(out['flags']),
            out['counts'].data_ptr(), _stream(dev)), 'oetr_match_score')
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = (table, idx1, idx2, params, offsets, k1, k2)
    return out
