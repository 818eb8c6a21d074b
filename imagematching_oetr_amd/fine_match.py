"""Dense matches refined to sub-pixel on the device: the two stages that bracket the fine network.

:func:`match_dense` leaves every match on a cell corner of the 1/8-resolution grid.  The matcher the reference calls in
its ``direct`` branch (``dloc/core/matchers/loftr.py``) returns the fine-level result: per coarse match a ``W x W``
window of 1/2-resolution features around both cells, a small network on the windows, the correlation of window 0's
centre with window 1, a softmax over the ``W * W`` positions and its spatial expectation.  :func:`fine_windows` builds
the match list of a :func:`match_dense` result and gathers the windows (``oetr_fine_windows``) - no ``unfold`` of the
whole fine maps, no ``nonzero``, nothing read back - and :func:`refine_matches` is the expectation head
(``oetr_fine_refine``; ``include/oetr_fine_match.h``, ``csrc/fine_match.hip``).  The network between them stays torch.
The head's arithmetic is the numpy specification of DESIGN 9.3p, reproduced bit for bit: the project's own statement,
modelled on LoFTR's published fine matching; that code lives in a ``third_party/`` tree outside the reference
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
from .dense_match import _map_rows, _rows
from .hip_engine import (FINE_MATCH_COUNTERS, FINE_MATCH_MAX_C, FINE_MATCH_MAX_STRIDE, FINE_MATCH_MIN_C,
                         FINE_MATCH_WINDOW_COUNTERS, FINE_MATCH_WINDOWS, _check, _stream)


def _coarse_side(coarse):
    """``matches0`` and the offsets / grids a :func:`match_dense` result keeps of its call."""
    if not isinstance(coarse, dict) or 'matches0' not in coarse:
        raise ValueError('`coarse` must be a match_dense result (a dict with `matches0`)')
    kept = coarse.get('_inputs')
    return coarse['matches0'], (kept[2:6] if kept is not None and len(kept) >= 6 else (None,) * 4)


@torch.no_grad()
def fine_windows(coarse, fine0, fine1, offsets0=None, offsets1=None, grids0=None, grids1=None, fine_offsets0=None,
                 fine_offsets1=None, fine_grids0=None, fine_grids1=None, window=5, stride=4, max_matches=None,
                 max_k0=None, channels_first=False, out=None):
    """The match list of a :func:`match_dense` result and the fine-feature windows of its matches, in one device call.

    ``coarse`` is the :func:`match_dense` result; ``offsets0`` / ``offsets1`` / ``grids0`` / ``grids1`` are the coarse
    call's and default to the ones the result keeps.  The fine maps come in one of two forms:

    * joined token rows ``fine0`` ``[F0,C]``, ``fine1`` ``[F1,C]`` in raster order with ``fine_offsets0`` /
      ``fine_offsets1`` int32 ``[P+1]`` and ``fine_grids0`` / ``fine_grids1`` int32 ``[P,2]`` = ``(hf, wf)``: the form
      a graph can capture;
    * sequences with one map per pair and side, ``fine0[p]`` ``[hf,wf,C]`` (``[C,hf,wf]`` with
      ``channels_first=True``): grids and offsets come from the shapes, the rows are joined on the device.  Channels
      last is the only layout of the kernel; a ``[C,hf,wf]`` map pays a permuting copy here.

    Features are float32 (float64 is refused); ``C % 4 == 0`` and ``4 <= C <= 512``.  ``window`` ``W`` is 3, 5 or 7;
    ``stride`` (1 .. 8) the fine cells per coarse cell.  ``max_matches`` is required: the capacity of the list, which
    sizes the outputs (nothing is read back to find the number of matches); a match beyond it is dropped and counted.
    ``max_k0``: the largest per-pair row count of side 0 the caller vouches for (default: all rows).  A pair whose
    grids do not multiply to its rows - coarse or fine, either side - or beyond ``max_k0`` is never dereferenced; its
    counters read ``-1``.  The fine grid need not be ``stride`` times the coarse one: what lies outside it reads zero.

    Returns a dict of device tensors: ``rows`` int32 ``[M,3]`` = (pair, index within side 0, index within side 1) of
    every match, pair after pair in ascending token order; ``moffsets`` int32 ``[P+1]``; ``counts`` int32 ``[P,2]`` =
    matched, kept; ``win0`` / ``win1`` float32 ``[M,W*W,C]``: element ``ky * W + kx`` of a token at coarse ``(row, col)``
    is fine token ``(row * stride + ky - W // 2, col * stride + kx - W // 2)``, ``+0`` outside the map -
    ``unfold(kernel W, stride, padding W // 2)``.  Rows from ``moffsets[P]`` on read ``-1`` / ``+0``.

    Enqueues on torch's current stream of the features' device and reads nothing back.  ``out``: the result of an
    earlier call of the same sizes, written into again with no allocation (it carries the call's workspace)."""
    if window not in FINE_MATCH_WINDOWS:
        raise ValueError(f'need window in {FINE_MATCH_WINDOWS}, got {window}')
    if int(stride) != stride or not 1 <= stride <= FINE_MATCH_MAX_STRIDE:
        raise ValueError(f'need an integer stride in 1 .. {FINE_MATCH_MAX_STRIDE}, got {stride}')
    if max_matches is None:
        raise ValueError('`max_matches` is required: the capacity of the match list (nothing is read back to find it)')
    if int(max_matches) != max_matches or max_matches < 0:
        raise ValueError(f'need an integer max_matches >= 0, got {max_matches}')
    if max_matches > (2 ** 31 - 1) // (window * window):
        raise ValueError(f'need max_matches <= {(2 ** 31 - 1) // (window * window)} (INT32_MAX / window^2); split the call')
    matches0, kept = _coarse_side(coarse)
    offsets0, offsets1, grids0, grids1 = (given if given is not None else k
                                          for given, k in zip((offsets0, offsets1, grids0, grids1), kept))
    for name, x in (('offsets0', offsets0), ('offsets1', offsets1), ('grids0', grids0), ('grids1', grids1)):
        if x is None:
            raise ValueError(f'`{name}` is neither given nor kept by `coarse`')
    joined = torch.is_tensor(fine0) or isinstance(fine0, np.ndarray)
    fine_args = (fine_offsets0, fine_offsets1, fine_grids0, fine_grids1)
    if joined:
        for name, x in zip(('fine_offsets0', 'fine_offsets1', 'fine_grids0', 'fine_grids1'), fine_args):
            if x is None:
                raise ValueError(f'joined fine token rows need `{name}`; or give one map per pair')
        parts0, parts1 = [fine0], [fine1]
    else:
        if any(x is not None for x in fine_args):
            raise ValueError('`fine_offsets*` / `fine_grids*` go with joined token rows, not with one map per pair')
        parts0, parts1 = list(fine0), list(fine1)
        if not parts0 or len(parts0) != len(parts1):
            raise ValueError('fine0 and fine1 must hold one map per pair')
    for name, parts in (('fine0', parts0), ('fine1', parts1)):
        for t in parts:
            _refuse_float64(name, t)
    dev = _device_of('fine_windows', [matches0] + parts0 + parts1)
    host_inputs = _host_names([('matches0', matches0), ('offsets0', offsets0), ('offsets1', offsets1), ('grids0', grids0),
                               ('grids1', grids1), ('fine_offsets0', fine_offsets0), ('fine_offsets1', fine_offsets1),
                               ('fine_grids0', fine_grids0), ('fine_grids1', fine_grids1)])
    host_inputs += [n for n, parts in (('fine0', parts0), ('fine1', parts1)) if any(_is_host(t) for t in parts)]
    if not joined:
        host_inputs.append('per-pair fine grids')
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        P = int(offsets0.shape[0] if hasattr(offsets0, 'shape') else len(offsets0)) - 1
        if P < 1:
            raise ValueError('fine_windows needs at least one pair')
        offsets0 = _upload('offsets0', offsets0, torch.int32, (P + 1,), dev)
        offsets1 = _upload('offsets1', offsets1, torch.int32, (P + 1,), dev)
        grids0 = _upload('grids0', grids0, torch.int32, (P, 2), dev)
        grids1 = _upload('grids1', grids1, torch.int32, (P, 2), dev)
        N0 = int(matches0.shape[0] if hasattr(matches0, 'shape') else len(matches0))
        matches0 = _upload('matches0', matches0, torch.int32, (N0,), dev)
        if joined:
            fine0, fine1 = _rows('fine0', fine0, dev), _rows('fine1', fine1, dev)
            foff0 = _upload('fine_offsets0', fine_offsets0, torch.int32, (P + 1,), dev)
            foff1 = _upload('fine_offsets1', fine_offsets1, torch.int32, (P + 1,), dev)
            fgrids0 = _upload('fine_grids0', fine_grids0, torch.int32, (P, 2), dev)
            fgrids1 = _upload('fine_grids1', fine_grids1, torch.int32, (P, 2), dev)
        else:
            if len(parts0) != P:
                raise ValueError(f'`coarse` has {P} pairs, fine0 {len(parts0)} maps')
            maps0 = [_map_rows('fine0', t, dev, channels_first) for t in parts0]
            maps1 = [_map_rows('fine1', t, dev, channels_first) for t in parts1]
            fine0 = _rows('fine0', torch.cat([r for r, _ in maps0]), dev)
            fine1 = _rows('fine1', torch.cat([r for r, _ in maps1]), dev)
            foff0 = _offsets_of([g[0] * g[1] for _, g in maps0], dev)
            foff1 = _offsets_of([g[0] * g[1] for _, g in maps1], dev)
            fgrids0 = torch.as_tensor(np.array([g for _, g in maps0], np.int32).reshape(P, 2)).to(dev)
            fgrids1 = torch.as_tensor(np.array([g for _, g in maps1], np.int32).reshape(P, 2)).to(dev)
        C = int(fine0.shape[1])
        if int(fine1.shape[1]) != C:
            raise ValueError('every fine feature tensor must have the same C')
        if C % 4 or not FINE_MATCH_MIN_C <= C <= FINE_MATCH_MAX_C:
            raise ValueError(f'need C % 4 == 0 and {FINE_MATCH_MIN_C} <= C <= {FINE_MATCH_MAX_C}, got C = {C}')
        F0, F1 = int(fine0.shape[0]), int(fine1.shape[0])
        N1 = int(coarse['keypoints1'].shape[0]) if 'keypoints1' in coarse else 2 ** 31 - 1
        if max(F0, F1, N0) > 2 ** 31 - 1:
            raise ValueError('more than 2^31 - 1 rows on a side in one call')
        M, WW = int(max_matches), window * window
        max_k0 = N0 if max_k0 is None else int(max_k0)
        if out is None:
            i32 = dict(dtype=torch.int32, device=dev)
            out = {'rows': torch.empty(M, 3, **i32), 'moffsets': torch.empty(P + 1, **i32),
                   'counts': torch.empty(P, FINE_MATCH_WINDOW_COUNTERS, **i32),
                   'win0': torch.empty(M, WW, C, device=dev), 'win1': torch.empty(M, WW, C, device=dev)}
        elif (tuple(out['rows'].shape) != (M, 3) or tuple(out['moffsets'].shape) != (P + 1,)
              or tuple(out['win0'].shape) != (M, WW, C) or out['rows'].device != dev):
            raise ValueError('`out` is the result of a call of other sizes (matches, pairs, window, channels)')
        lib = hip_engine.load_library()
        need = int(lib.oetr_fine_match_workspace_bytes(P))
        workspace = _workspace(out, max(need, 1), dev)
        _check(lib, lib.oetr_fine_windows(
            _ptr(matches0), offsets0.data_ptr(), offsets1.data_ptr(), grids0.data_ptr(), grids1.data_ptr(), N0, N1, P,
            max_k0, _ptr(fine0), foff0.data_ptr(), fgrids0.data_ptr(), F0, _ptr(fine1), foff1.data_ptr(),
            fgrids1.data_ptr(), F1, C, int(window), int(stride), M, workspace.data_ptr(), need, _ptr(out['rows']),
            out['moffsets'].data_ptr(), out['counts'].data_ptr(), _ptr(out['win0']), _ptr(out['win1']), _stream(dev)),
            'oetr_fine_windows')
        out['window'], out['stride'] = int(window), int(stride)
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = (matches0, offsets0, offsets1, grids0, grids1, fine0, fine1, foff0, foff1, fgrids0, fgrids1)
    return out


@torch.no_grad()
def refine_matches(windows, coarse, win0=None, win1=None, fine_cell=2.0, out=None):
    """The expectation head on the windows of a match list: every match's sub-pixel position, in one device call.

    ``windows`` is a :func:`fine_windows` result and ``coarse`` the :func:`match_dense` result it came from.
    ``win0`` / ``win1`` float32 ``[M,W*W,C]``: what a network made of ``windows['win0']`` / ``windows['win1']``
    (default: the gathered windows themselves).  ``fine_cell``: the pixels per fine token (``cell / stride``).

    Per match: the correlation of window 0's centre with window 1's ``W * W`` positions, scaled by ``1 / sqrt(C)``, a
    softmax, its expectation ``(x, y)`` in ``[-1, 1]`` and the expectation's standard deviation; the refined keypoint
    is ``keypoints1[j] + (x, y) * (W // 2) * fine_cell`` (DESIGN 9.3p states every rounding).

    Returns a dict of device tensors: ``expec`` float32 ``[M,3]`` = (x, y, std); ``mkpts0`` / ``mkpts1`` float32
    ``[M,2]``, the form the reference's ``loftr.py`` returns; ``keypoints1`` float32 ``[N1,2]``: the coarse
    ``keypoints1`` with the refined position at every matched token, so that ``assemble_matches(crops, scales,
    coarse['keypoints0'], fine['keypoints1'], coarse['matches0'], coarse['matching_scores0'], ...)`` works on refined
    matches; ``keypoints0`` (the coarse one); ``counts`` int32 ``[P,3]`` = matched, kept, without a candidate (every
    correlation non-finite: ``x = y = 0``, ``std`` NaN); ``rows`` / ``moffsets`` of ``windows``.  Rows past the list
    read NaN.  Enqueues only; ``out``: an earlier result of the same sizes, written into again with no allocation."""
    fine_cell = float(fine_cell)
    if not (math.isfinite(fine_cell) and fine_cell > 0):
        raise ValueError(f'need a finite fine_cell > 0, got {fine_cell}')
    if not isinstance(windows, dict) or 'rows' not in windows or 'window' not in windows:
        raise ValueError('`windows` must be a fine_windows result')
    if not isinstance(coarse, dict) or 'keypoints0' not in coarse or 'keypoints1' not in coarse:
        raise ValueError('`coarse` must be a match_dense result (a dict with `keypoints0` and `keypoints1`)')
    win0 = windows['win0'] if win0 is None else win0
    win1 = windows['win1'] if win1 is None else win1
    _refuse_float64('win0', win0)
    _refuse_float64('win1', win1)
    rows, moffsets, W = windows['rows'], windows['moffsets'], int(windows['window'])
    dev = rows.device
    M, P = int(rows.shape[0]), int(moffsets.shape[0]) - 1
    host_inputs = _host_names([('win0', win0), ('win1', win1), ('keypoints0', coarse['keypoints0']),
                               ('keypoints1', coarse['keypoints1'])])
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        for name, w in (('win0', win0), ('win1', win1)):
            if not torch.is_tensor(w) or w.dtype != torch.float32 or w.device != dev or w.dim() != 3 \
                    or tuple(w.shape[:2]) != (M, W * W):
                raise ValueError(f'{name} must be a float32 [{M},{W * W},C] tensor on {dev}')
        C = int(win0.shape[2])
        if int(win1.shape[2]) != C or C % 4 or not FINE_MATCH_MIN_C <= C <= FINE_MATCH_MAX_C:
            raise ValueError(f'need the same C in win0 and win1, C % 4 == 0 and {FINE_MATCH_MIN_C} <= C <= '
                             f'{FINE_MATCH_MAX_C}')
        win0, win1 = win0.contiguous(), win1.contiguous()
        win0 = win0.clone() if win0.data_ptr() % 16 else win0
        win1 = win1.clone() if win1.data_ptr() % 16 else win1
        offsets0, offsets1 = windows['_inputs'][1], windows['_inputs'][2]
        kp0, kp1 = coarse['keypoints0'], coarse['keypoints1']
        N0, N1 = int(kp0.shape[0]), int(kp1.shape[0])
        kp0 = _upload('keypoints0', kp0, torch.float32, (N0, 2), dev)
        kp1 = _upload('keypoints1', kp1, torch.float32, (N1, 2), dev)
        if out is None:
            out = {'expec': torch.empty(M, 3, device=dev), 'mkpts0': torch.empty(M, 2, device=dev),
                   'mkpts1': torch.empty(M, 2, device=dev), 'keypoints1': torch.empty(N1, 2, device=dev),
                   'counts': torch.empty(P, FINE_MATCH_COUNTERS, dtype=torch.int32, device=dev)}
        elif (tuple(out['expec'].shape) != (M, 3) or tuple(out['keypoints1'].shape) != (N1, 2)
              or tuple(out['counts'].shape) != (P, FINE_MATCH_COUNTERS) or out['expec'].device != dev):
            raise ValueError('`out` is the result of a call of other sizes (matches, tokens, pairs)')
        lib = hip_engine.load_library()
        _check(lib, lib.oetr_fine_refine(
            _ptr(win0), _ptr(win1), _ptr(rows), moffsets.data_ptr(), windows['counts'].data_ptr(), P, M, _ptr(kp0),
            offsets0.data_ptr(), N0, _ptr(kp1), offsets1.data_ptr(), N1, C, W, fine_cell, _ptr(out['expec']),
            _ptr(out['mkpts0']), _ptr(out['mkpts1']), _ptr(out['keypoints1']), out['counts'].data_ptr(), _stream(dev)),
            'oetr_fine_refine')
        out['keypoints0'], out['rows'], out['moffsets'] = kp0, rows, moffsets
        out['_inputs'] = (win0, win1, rows, moffsets, windows['counts'], kp0, kp1, offsets0, offsets1)
    return out


def fine_match_counts(result):
    """The counters of a :func:`refine_matches` result as a host int32 array ``[P,3]`` - matched, kept (matched minus
    those dropped at ``max_matches``), kept matches without a candidate - or of a :func:`fine_windows` result
    ``[P,2]``; ``-1`` for a pair that was not vouched for.  ONE read, which synchronises the stream."""
    return result['counts'].cpu().numpy()
