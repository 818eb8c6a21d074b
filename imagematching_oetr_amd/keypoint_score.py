"""Keypoint repeatability against depth and pose on the device, by index over a depth-map set.

``match_score.score_matches`` says what share of a matcher's matches is correct; a matcher that
returns three correct matches scores 100 %.  The counterpart - of the keypoints that COULD have been
matched, how many have a partner in the other picture at all - is the reference's repeatability
(``pose_evaluate`` -> ``get_projected_kp`` / ``unnormalize_keypoints`` / ``get_repeatability``).
:func:`score_keypoints` computes it for MANY pairs of a pair list over a
:class:`~imagematching_oetr_amd.covis_set.DepthSet` and the keypoints of its pictures, both
directions, in one HIP call that reads the depth maps in place (``oetr_keypoint_repeatability``,
``include/oetr_keypoint_score.h``, ``csrc/keypoint_score.hip``): per pair and direction ``2 + T``
counters, and per keypoint its nearest neighbour in the other picture and the squared distance to it.
The arithmetic is the float64 specification of DESIGN 9.3g (the numpy restatement the tests hold),
reproduced bit for bit.  There is no CPU implementation.

:func:`ground_truth_matches` turns the nearest neighbours into the ground-truth correspondences
between the two keypoint sets of every pair (the reference's ``get_matching_score`` is ``pass``).

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import ctypes
import math

import numpy as np
import torch

from . import hip_engine
from ._inputs import (_host_names, _is_host, _keypoints, _offsets_of, _pair_blocks, _pair_tensor, _ptr,
                      _refuse_float64, _refuse_host_inputs_in_capture, _upload)
from .hip_engine import KEYPOINT_SCORE_HEAD_COUNTERS, KEYPOINT_SCORE_MAX_THRESHOLDS, _check, _stream
from .match_score import match_params


def _is_concatenated(keypoints):
    return (isinstance(keypoints, tuple) and len(keypoints) == 3 and isinstance(keypoints[2], (int, np.integer))
            and not isinstance(keypoints[2], bool))


@torch.no_grad()
def score_keypoints(depth_set, pair_index, keypoints, thresholds=(1, 2, 3, 5), nearest=True, out=None, params=None):
    """Score the keypoint sets of the pairs ``pair_index`` over ``depth_set``, all in one device call.

    ``pair_index``: a host sequence of ``(i, j)`` or a device int32 ``[P,2]`` tensor.  ``keypoints``:
    a sequence with one ``[n_k,2]`` tensor or array per slot of the set - ``(u, v)`` in the ORIGINAL
    pictures, float32 or float16 (widened; exact), on the device or on the host (uploaded); float64 is
    refused, as in ``score_matches``.  The counts come from the shapes: nothing is read from the
    device.  Alternatively ``keypoints=(cat, kp_offsets, max_kp)``: the sets concatenated as a device
    float32 ``[N,2]`` tensor, a device int32 ``[len(depth_set) + 1]`` tensor (picture k owns the rows
    ``kp_offsets[k] .. kp_offsets[k+1]-1``) and a host int, the largest count per picture the caller
    vouches for - the form for a capturable call.  ``thresholds``: at most 8, in pixels.  ``params``:
    float64 ``[P,20]`` blocks (``match_params``'s layout); ``None``: ``match_params`` of the set's
    cameras.

    Returns a dict of device tensors.  ``counts`` int32 ``[P,2,2+T]``: per pair and direction (0: picture
    i -> picture j, 1: j -> i) the source picture's keypoints, the KEPT ones - those with a depth whose
    projection has ``u < W`` and ``v < H`` of the other picture: the reference's test, without a lower
    bound - and per threshold the kept ones whose nearest keypoint of the other picture is closer than
    it.  ``nearest`` int32 and ``dist_sq`` float64 ``[P,2,max_kp]`` (absent with ``nearest=False``): per
    source keypoint the index of that nearest keypoint within its picture (the lowest index on a tie; a
    keypoint with a non-finite coordinate is never it) and the SQUARED distance; -1 / NaN for keypoints
    that are not kept and past a picture's count, -1 / +inf when the other picture has no keypoint.
    ``thresholds``: the tuple used.  A pair with an index outside the set, or with a picture of more
    than ``max_kp`` keypoints, is not scored: -1 / NaN rows, all counters -1.

    Enqueues on torch's current stream of the set's device and reads nothing back, so it can be
    captured into a HIP graph when every input is a device tensor (a replay scores what the keypoint,
    offset, index and parameter tensors hold at replay time); use the set once before the capture, so
    that its table is uploaded outside it.  ``out``: the result of an earlier call of the same sizes,
    written into again with no allocation."""
    thresholds = tuple(float(t) for t in thresholds)
    T = len(thresholds)
    if T > KEYPOINT_SCORE_MAX_THRESHOLDS:
        raise ValueError(f'at most {KEYPOINT_SCORE_MAX_THRESHOLDS} thresholds, got {T}')
    concatenated = _is_concatenated(keypoints)
    if concatenated:
        _refuse_float64('keypoints[0]', keypoints[0])
    else:
        keypoints = list(keypoints)
        for k, kp in enumerate(keypoints):
            _refuse_float64(f'keypoints[{k}]', kp)
    dev = torch.device(depth_set.device)
    if dev.type != 'cuda':
        raise RuntimeError(f'score_keypoints needs a depth-map set on a GPU (HIP) device, got {dev}. There is no CPU '
                           'implementation.')
    n_maps = len(depth_set)
    host_inputs = _host_names((('pair_index', pair_index), ('params', params)))
    if concatenated:
        host_inputs += [n for n, x in (('keypoints[0]', keypoints[0]), ('keypoints[1]', keypoints[1])) if _is_host(x)]
    else:
        if len(keypoints) != n_maps:
            raise ValueError(f'{len(keypoints)} keypoint sets, {n_maps} depth maps: slot k of the set must hold the '
                             'depth map of the picture of keypoints[k]')
        host_inputs.append('keypoints (a sequence: its offsets are uploaded)')
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        if concatenated:
            cat, kp_offsets, max_kp = keypoints
            if _is_host(cat) or _is_host(kp_offsets):
                raise ValueError('keypoints=(cat, kp_offsets, max_kp): cat and kp_offsets must be device tensors')
            if cat.dtype != torch.float32:
                raise ValueError(f'keypoints[0] must be float32, got {cat.dtype}')
            cat = _keypoints('keypoints[0]', cat, dev, 'depth-map set')
            kp_offsets = _upload('keypoints[1]', kp_offsets, torch.int32, (n_maps + 1,), dev)
            max_kp = int(max_kp)
            if max_kp < 0:
                raise ValueError(f'max_kp must be >= 0, got {max_kp}')
        else:
            sets = [_keypoints(f'keypoints[{k}]', kp, dev, 'depth-map set') for k, kp in enumerate(keypoints)]
            lengths = [int(kp.shape[0]) for kp in sets]
            cat = torch.cat(sets) if sets else torch.zeros(0, 2, dtype=torch.float32, device=dev)
            kp_offsets = _offsets_of(lengths, dev)
            max_kp = max(lengths, default=0)
        N = int(cat.shape[0])
        if N > 2 ** 31 - 1:
            raise ValueError('more than 2^31 - 1 keypoints in one call')
        pair_index = _pair_tensor(dev, pair_index)
        P = int(pair_index.shape[0])
        if out is None:
            out = {'counts': torch.zeros(P, 2, KEYPOINT_SCORE_HEAD_COUNTERS + T, dtype=torch.int32, device=dev)}
            if nearest:
                out['nearest'] = torch.full((P, 2, max_kp), -1, dtype=torch.int32, device=dev)
                out['dist_sq'] = torch.full((P, 2, max_kp), math.nan, dtype=torch.float64, device=dev)
        elif (tuple(out['counts'].shape) != (P, 2, KEYPOINT_SCORE_HEAD_COUNTERS + T) or ('nearest' in out) != bool(nearest)
              or (nearest and tuple(out['nearest'].shape) != (P, 2, max_kp))):
            raise ValueError('`out` is the result of a call of other sizes (pairs, thresholds, max_kp, nearest)')
        out['thresholds'] = thresholds
        if P == 0 or n_maps == 0:                    # nothing to score; without a map no pair is vouched for
            out['counts'].fill_(-1)
            if nearest:
                out['nearest'].fill_(-1)
                out['dist_sq'].fill_(math.nan)
            return out
        idx1, idx2, table, params = _pair_blocks(depth_set, pair_index, params, match_params)
        lib = hip_engine.load_library()
        thr = (ctypes.c_double * max(T, 1))(*thresholds)
        _check(lib, lib.oetr_keypoint_repeatability(
            table.data_ptr(), n_maps, _ptr(cat), N, kp_offsets.data_ptr(), idx1.data_ptr(), idx2.data_ptr(),
            params.data_ptr(), P, thr if T else None, T, max_kp, out['counts'].data_ptr(),
            _ptr(out['nearest']) if nearest else None, _ptr(out['dist_sq']) if nearest else None, _stream(dev)),
            'oetr_keypoint_repeatability')
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = (table, idx1, idx2, params, kp_offsets, cat)
    return out


@torch.no_grad()
def ground_truth_matches(result, px_thr):
    """The ground-truth correspondences of a :func:`score_keypoints` result (with ``nearest=True``): int32
    ``[P,max_kp]`` on the device, entry ``a`` of pair p holding ``b`` when keypoint ``a`` of picture i and
    keypoint ``b`` of picture j are MUTUAL nearest neighbours - ``nearest[p,0,a] == b`` and
    ``nearest[p,1,b] == a`` - and both squared distances are below ``px_thr * px_thr`` (compared in
    float64); -1 otherwise.  Torch gathers on the device; nothing is read back.  Not a hot path."""
    if 'nearest' not in result:
        raise ValueError('ground_truth_matches needs the per-keypoint outputs: score_keypoints(..., nearest=True)')
    near, dist = result['nearest'], result['dist_sq']
    n12, n21 = near[:, 0].long(), near[:, 1].long()
    if near.shape[2] == 0:
        return near[:, 0].clone()
    limit = float(px_thr) * float(px_thr)
    b = n12.clamp(min=0)
    back = torch.gather(n21, 1, b)
    back_dist = torch.gather(dist[:, 1], 1, b)
    a = torch.arange(near.shape[2], device=near.device)[None, :]
    mutual = (n12 >= 0) & (back == a) & (dist[:, 0] < limit) & (back_dist < limit)
    return torch.where(mutual, near[:, 0], torch.full_like(near[:, 0], -1))
