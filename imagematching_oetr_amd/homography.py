"""Scoring matches and overlap boxes against a homography on the device: the planar evaluation protocol.

Every other ground truth of the evaluation chain comes from depth maps and poses.  The reference's second
protocol needs neither: on HPatches, ``dloc/evaluate/eval_hpatches.py`` computes
``h_evaluate(H_gt, kpts0, kpts1, matches)`` per pair and accumulates ``mean(dist <= thr)`` for
``thr = 1 .. 15``, split into illumination and viewpoint sequences.  :func:`score_matches_homography`
computes those distances (SQUARED - the project's standing departure) and the per-threshold counters for
MANY match lists in one HIP call (``oetr_homography_match_score``), :func:`homography_accuracy` is the
reference's summary from one read of the counters, and :func:`overlap_boxes_from_homography` gives the
ground-truth overlap boxes of pairs of pictures related by a homography (``oetr_homography_boxes``; the
project's own statement - the reference has none) under the keys ``overlap_boxes_from_batch`` returns.
``include/oetr_homography.h`` has the contract, ``csrc/homography.hip`` the kernels; the arithmetic is the
float64 specification of DESIGN 9.3i, reproduced bit for bit.  There is no CPU implementation.

``H`` maps pixel coordinates of picture 1 to picture 2; pixel centres sit at integer coordinates (the
convention of HPatches' ``H_1_k`` files and of ``h_evaluate``).

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import ctypes
import math

import numpy as np
import torch

from . import hip_engine
from ._inputs import (NO_CPU, _device_of, _host_names, _is_host, _match_keypoints, _match_list_args, _match_offsets,
                      _ptr, _refuse_host_inputs_in_capture, _shape_of, _upload, _workspace)
from .hip_engine import COVIS_MAX_SIDE, HOMOGRAPHY_MAX_THRESHOLDS, HOMOGRAPHY_PARAM_DOUBLES, _check, _stream

def _f64(x, dev):
    """``x`` as a float64 tensor on ``dev``: a device tensor converted there, a host array uploaded (blocking)."""
    if _is_host(x):
        x = torch.as_tensor(np.asarray(x, dtype=np.float64) if not torch.is_tensor(x) else x)
    return x.to(device=dev, dtype=torch.float64)


def _sizes(name, size, n, dev):
    """``(h, w)`` or ``[P,2]`` -> float64 ``[n,2]`` on ``dev``."""
    s = _f64(size, dev).reshape(-1, 2)
    if s.shape[0] not in (1, n):
        raise ValueError(f'{name} must be (h, w) or [{n},2], got {tuple(s.shape)}')
    return s.expand(n, 2)


def homography_params(H, size1, size2, device=None):
    """The parameter blocks of ``oetr_homography_match_score`` / ``oetr_homography_boxes``: float64
    ``[P,16]`` on the device - ``H`` row major, then ``W1, H1, W2, H2``, three reserved zeros
    (``include/oetr_homography.h``).  ``H``: ``[P,3,3]`` or ``[3,3]``, from the host or the device, any
    float dtype (used as float64).  ``size1`` / ``size2``: the pictures' ``(h, w)``, one for all pairs or
    ``[P,2]``.  Composed on the device (``device``, else ``H``'s GPU, else the current GPU); nothing is
    read back."""
    dev = torch.device(device) if device is not None else _device_of('homography_params', (H, size1, size2))
    if dev.type != 'cuda':
        raise RuntimeError(f'homography_params needs a GPU (HIP) device, got {dev}. ' + NO_CPU)
    Hd = _f64(H, dev)
    if Hd.dim() not in (2, 3) or tuple(Hd.shape[-2:]) != (3, 3):
        raise ValueError(f'H must be [P,3,3] or [3,3], got {tuple(Hd.shape)}')
    Hd = Hd.reshape(-1, 9)
    n = int(Hd.shape[0])
    params = torch.zeros(n, HOMOGRAPHY_PARAM_DOUBLES, dtype=torch.float64, device=dev)
    params[:, 0:9] = Hd
    for at, (name, size) in ((9, ('size1', size1)), (11, ('size2', size2))):
        if size is not None:
            s = _sizes(name, size, n, dev)
            params[:, at], params[:, at + 1] = s[:, 1], s[:, 0]
    return params


def rescale_homography(H, scale1, scale2):
    """``H`` between the ORIGINAL pictures -> ``H`` between their RESIZED images:
    ``diag(1/s2x, 1/s2y, 1) . H . diag(s1x, s1y, 1)``.

    ``scale1`` / ``scale2`` are the reader's ``scales = original / resized`` as ``(sx, sy)`` (one pair, or
    ``[P,2]``), in the plain multiplicative convention of the reference's ``kpts * scales``: a point
    ``p`` of the resized image is ``p * scales`` in the original one, with no half-pixel term.  Works on
    whatever holds ``H`` (host arrays give a float64 numpy array, tensors a float64 tensor on their
    device); two elementwise float64 operations per entry, ``(H * s1) / s2``, no matrix product."""
    if torch.is_tensor(H):
        f = lambda x: (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))).to(
            device=H.device, dtype=torch.float64)                 # (a Python float is float64, not torch's float32)
        ones, cat = torch.ones_like, (lambda parts: torch.cat(parts, -1))
    else:
        f = lambda x: np.asarray(x.cpu() if torch.is_tensor(x) else x, dtype=np.float64)
        ones, cat = np.ones_like, (lambda parts: np.concatenate(parts, -1))
    Hm, s1, s2 = f(H), f(scale1), f(scale2)
    col = cat([s1, ones(s1[..., :1])])[..., None, :]          # [...,1,3]: scales the columns
    row = cat([s2, ones(s2[..., :1])])[..., :, None]          # [...,3,1]: divides the rows
    return (Hm * col) / row


def _blocks(params_or_H, dev, size1=None, size2=None):
    """float64 ``[P,16]`` blocks on ``dev`` of either form of the first argument."""
    x = params_or_H
    shape = _shape_of(x)
    if len(shape) == 2 and shape[1] == HOMOGRAPHY_PARAM_DOUBLES:
        return _upload('params', x, torch.float64, shape, dev)
    return homography_params(x, size1, size2, device=dev)


@torch.no_grad()
def score_matches_homography(params_or_H, k1, k2, lengths=None, offsets=None, thresholds=range(1, 16), values=True,
                             out=None):
    """Score the match lists of ``P`` pairs against their homographies, all in one device call.

    ``params_or_H``: float64 ``[P,16]`` blocks (:func:`homography_params`) or ``H`` itself, ``[P,3,3]``
    or ``[3,3]`` (the scoring does not need the sizes).  ``k1`` / ``k2``: the lists concatenated,
    ``[M,2]`` ``(x, y)``, float32 or float16 (widened; exact) - device tensors are taken as they are,
    host arrays are uploaded; float64 is refused.  Exactly one of ``lengths`` (a host sequence, one
    length per pair, summing to ``M``) and ``offsets`` (a device int32 ``[P+1]`` tensor: list p is the
    rows ``offsets[p] .. offsets[p+1]-1``; non-decreasing; rows outside every list are left unscored) -
    ``assemble_matches``' ``k1``, ``k2`` and ``offsets`` are taken as they are.  ``thresholds``: at most
    16, in pixels; they are read on the host during the call, so a captured graph keeps its own.

    Returns ``{'dist_sq': float64 [M] (the SQUARED distance of ``k2`` from ``H k1``; NaN for a row in
    no list; absent with values=False), 'counts': int32 [P, 1+T] (the list's length, then its rows with
    ``dist_sq <= thr * thr``), 'thresholds': the tuple used}``.  ``P == 0`` and ``M == 0`` are legal.

    Enqueues on torch's current stream and reads nothing back, so it can be captured into a HIP graph
    when every input is a device tensor (a replay scores what the keypoint, offset and parameter
    tensors hold at replay time).  ``out``: the result of an earlier call of the same sizes, written
    into again with no allocation."""
    _match_list_args(k1, k2, lengths, offsets)
    thresholds = tuple(thresholds)
    T = len(thresholds)
    if T > HOMOGRAPHY_MAX_THRESHOLDS:
        raise ValueError(f'at most {HOMOGRAPHY_MAX_THRESHOLDS} thresholds, got {T}')
    dev = _device_of('score_matches_homography', (params_or_H, k1, k2, offsets))
    host_inputs = _host_names((('params_or_H', params_or_H), ('k1', k1), ('k2', k2), ('offsets', offsets)), lengths)
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        k1, k2, M = _match_keypoints(k1, k2, dev, 'other inputs')
        params = _blocks(params_or_H, dev)
        P = int(params.shape[0])
        offsets = _match_offsets(lengths, offsets, P, M, dev)
        if out is None:
            out = {'counts': torch.zeros(P, 1 + T, dtype=torch.int32, device=dev)}
            if values:
                out['dist_sq'] = torch.full((M,), math.nan, dtype=torch.float64, device=dev)
        elif tuple(out['counts'].shape) != (P, 1 + T) or ('dist_sq' in out) != bool(values) or (
                values and tuple(out['dist_sq'].shape) != (M,)):
            raise ValueError('`out` is the result of a call of other sizes (matches, pairs, thresholds, values)')
        out['thresholds'] = thresholds
        if P == 0:                                   # nothing to score: every row is outside every list
            if values:
                out['dist_sq'].fill_(math.nan)
            return out
        lib = hip_engine.load_library()
        thr = (ctypes.c_double * max(T, 1))(*(float(t) for t in thresholds))
        _check(lib, lib.oetr_homography_match_score(
            params.data_ptr(), offsets.data_ptr(), P, _ptr(k1), _ptr(k2), M, thr, T,
            _ptr(out['dist_sq']) if values else None, out['counts'].data_ptr(), _stream(dev)),
            'oetr_homography_match_score')
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = (params, offsets, k1, k2)
    return out


def homography_accuracy(result, seq_type=None):
    """The reference's ``benchmark_features`` summary (``dloc/evaluate/eval_hpatches.py``) of a
    :func:`score_matches_homography` result, from ONE device read of its ``counts`` int32 ``[P,1+T]`` (a
    tensor or an array of that shape is taken as well; the thresholds then default to ``1 .. T``).

    Returns ``{'accuracy': float64 [P,T] - per pair the share of its matches with ``dist <= thr``, the
    reference's ``mean(dist <= thr)``, 0 for an empty list as its ``dist = [inf]`` substitute gives -,
    'sum': float64 [T], the shares added up pair after pair, 'n_matches': int64 [P], 'thresholds':
    tuple}``.  With ``seq_type`` - one name per pair; its first letter decides, ``'i'`` for an
    illumination sequence and anything else for a viewpoint one, as there - also ``'i_err'`` /
    ``'v_err'``: dicts keyed by threshold of the shares added up over each kind, which the reference
    returns and divides by the number of sequences."""
    counts = result['counts'] if isinstance(result, dict) else result
    thresholds = result.get('thresholds') if isinstance(result, dict) else None
    counts = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] < 1:
        raise ValueError(f'counts must be [P,1+T], got {counts.shape}')
    counts = counts.astype(np.int64)
    T = counts.shape[1] - 1
    thresholds = tuple(range(1, T + 1)) if thresholds is None else tuple(thresholds)
    if len(thresholds) != T:
        raise ValueError(f'{len(thresholds)} thresholds for counts of shape {counts.shape}')
    n = counts[:, 0]
    share = np.where(n[:, None] > 0, counts[:, 1:] / np.maximum(n, 1)[:, None], 0.0)
    # added up in pair order, one addition per pair, as the reference's `+=` does
    total = lambda rows: np.cumsum(rows, axis=0)[-1] if rows.shape[0] else np.zeros(T)
    res = {'accuracy': share, 'sum': total(share), 'n_matches': n, 'thresholds': thresholds}
    if seq_type is not None:
        names = [str(s) for s in seq_type]
        if len(names) != counts.shape[0]:
            raise ValueError(f'{len(names)} sequence names for {counts.shape[0]} pairs')
        illum = np.array([s[:1] == 'i' for s in names], bool)
        i_sum, v_sum = total(share[illum]), total(share[~illum])
        res['i_err'] = {thr: float(i_sum[t]) for t, thr in enumerate(thresholds)}
        res['v_err'] = {thr: float(v_sum[t]) for t, thr in enumerate(thresholds)}
    return res


@torch.no_grad()
def overlap_boxes_from_homography(params_or_H, size1=None, size2=None, out=None, max_size1=None):
    """Ground-truth overlap boxes of ``P`` pairs of pictures related by homographies, in one device call.

    ``params_or_H``: float64 ``[P,16]`` blocks (:func:`homography_params`), or ``H`` ``[P,3,3]`` /
    ``[3,3]`` together with ``size1`` / ``size2``, the pictures' ``(h, w)`` (one for all pairs, or
    ``[P,2]``).  Every pixel of picture 1 is mapped by ``H``; it is kept when it lies on picture 2's side
    of the horizon line (``a2 > 0``) and lands, rounded half to even, on a pixel of picture 2.

    Returns device tensors under the keys of ``overlap_boxes_from_batch``: ``overlap_box1`` /
    ``overlap_box2`` float32 ``[P,4]`` (x1, y1, x2, y2 over the kept pixels and over their landing
    pixels; zeros for a pair that keeps none), ``overlap_valid`` bool ``[P]``, ``overlap_count`` int32
    ``[P]`` and ``count``, the same tensor.  A pair whose sizes are not whole numbers in 1..8192, or
    whose picture 1 exceeds the bound below, is not evaluated: count -1, not valid, zero boxes.

    The grid is set by a HOST bound on picture 1's size: ``max_size1 = (max_h1, max_w1)``; ``None``
    takes it from a host ``size1``, and otherwise reads the largest ``H1`` / ``W1`` of the blocks back
    once (the only read; refused inside a graph capture).  ``out``: the result of an earlier call with as
    many pairs, written into again with no allocation - it carries the call's workspace as
    ``out['workspace']``, as ``covis.covis_boxes`` keeps it."""
    dev = _device_of('overlap_boxes_from_homography', (params_or_H, size1, size2))
    with torch.cuda.device(dev):
        params = _blocks(params_or_H, dev, size1, size2)
        n = int(params.shape[0])
        if max_size1 is None and size1 is not None and _is_host(size1):
            s = np.asarray(size1.cpu() if torch.is_tensor(size1) else size1, dtype=np.float64).reshape(-1, 2)
            max_size1 = (s[:, 0].max(), s[:, 1].max()) if s.size else (1, 1)
        if max_size1 is None and n:
            if torch.cuda.is_current_stream_capturing():
                raise ValueError('inside a graph capture give max_size1 = (max_h1, max_w1): it cannot be read back')
            top = params[:, 9:11].nan_to_num(nan=1.0).amax(0).cpu()
            max_size1 = (float(top[1]), float(top[0]))
        if out is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
            out = {'overlap_box1': torch.empty(n, 4, device=dev), 'overlap_box2': torch.empty(n, 4, device=dev),
                   'overlap_valid': torch.empty(n, dtype=torch.bool, device=dev), 'overlap_count': count,
                   'count': count}
        elif tuple(out['overlap_box1'].shape) != (n, 4):
            raise ValueError('`out` is the result of a call with another number of pairs')
        if n == 0:
            return out
        clamp = lambda v: int(min(max(math.ceil(v) if math.isfinite(v) else 1, 1), COVIS_MAX_SIDE))
        max_h1, max_w1 = clamp(float(max_size1[0])), clamp(float(max_size1[1]))
        lib = hip_engine.load_library()
        workspace = _workspace(out, int(lib.oetr_homography_workspace_bytes(n)), dev)
        _check(lib, lib.oetr_homography_boxes(
            params.data_ptr(), n, max_h1, max_w1, workspace.data_ptr(), workspace.numel(),
            out['overlap_box1'].data_ptr(), out['overlap_box2'].data_ptr(), out['overlap_valid'].data_ptr(),
            out['overlap_count'].data_ptr(), _stream(dev)), 'oetr_homography_boxes')
        out['_inputs'] = (params,)
    return out
