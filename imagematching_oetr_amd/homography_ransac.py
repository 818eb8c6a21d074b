"""Homographies from match lists by RANSAC with a refit on the device: the estimating half of the planar protocol.

``score_matches_homography`` / ``overlap_boxes_from_homography`` need a homography given from outside.  The
reference's ``pr_evaluate`` / ``pr_evaluate_cv`` (``dloc/evaluate/utils/evaluation.py``) fit a planar transform
to the matches per pair on the host (``skimage.measure.ransac`` / ``cv2.estimateAffine*``) and carry landmarks
across with ``homo_trans``.  :func:`estimate_homographies` estimates a full homography for MANY match lists in
one HIP call (``oetr_homography_ransac``), refits it on its inliers and leaves the four squared corner distances
to ``H_gt`` on the device; ``evaluate.homography_errors`` / ``homography_auc`` / ``match_homography_auc`` turn
them into a mean corner error and its AUC from one read, and :func:`transfer_points` is ``homo_trans``.
``include/oetr_homography_ransac.h`` has the contract, ``csrc/homography_ransac.hip`` the kernels; the
arithmetic is the float64 specification of DESIGN 9.3l, reproduced bit for bit.  It is the project's own
statement - a 4-point solver, a fixed number of hypotheses, a least-squares refit with a specified summation
order - and claims no parity with skimage or OpenCV.  There is no CPU implementation of the estimator.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import math

import numpy as np
import torch

from . import hip_engine
from ._inputs import (_device_of, _host_names, _match_keypoints, _match_list_args, _match_offsets, _ptr,
                      _refuse_host_inputs_in_capture, _shape_of, _upload, _workspace)
from .hip_engine import (HOMOGRAPHY_PARAM_DOUBLES, HOMOGRAPHY_RANSAC_COUNTERS, HOMOGRAPHY_RANSAC_MAX_HYPOTHESES,
                         HOMOGRAPHY_RANSAC_MAX_MODELS, HOMOGRAPHY_RANSAC_MAX_REFIT, _check, _stream)


@torch.no_grad()
def estimate_homographies(params, k1, k2, lengths=None, offsets=None, n_hyp=256, px_thr=3.0, refit_iters=2, seed=0,
                          pair_ids=None, models=None, inliers=True, out=None):
    """Estimate the homography of ``P`` pairs from their match lists, all in one device call.

    ``params``: float64 ``[P,16]`` blocks as ``homography_params`` builds them (``H_gt`` row major, then
    ``W1, H1, W2, H2``); the estimate needs the sizes only - a block whose ``H_gt`` is NaN means "no ground
    truth".  ``k1`` / ``k2``: the lists concatenated, ``[M,2]`` ``(u, v)`` in the original pictures, float32
    or float16 (widened; exact) - device tensors are taken as they are, host arrays are uploaded; float64
    is refused.  Exactly one of ``lengths`` (a host sequence, one length per pair, summing to ``M``) and
    ``offsets`` (a device int32 ``[P+1]`` tensor) - ``assemble_matches``' ``k1``, ``k2`` and ``offsets``
    are taken as they are.  ``n_hyp``: hypotheses per pair, 1..4096, each a 4-point sample that gives one
    model; all are scored.  ``px_thr``: the inlier threshold in pixels of picture 2.  ``refit_iters``:
    least-squares rounds on the inliers of the selected model, 0..4.  ``seed`` and ``pair_ids`` (int32
    ``[P]``; default: the pair's position) feed the stateless sampler.  ``models``: float64 ``[P,n,9]``
    models of the caller's in NORMALISED coordinates, ``n`` in 1..4096 - sampling and solving are skipped.

    Returns device tensors: ``H`` float64 ``[P,9]`` (pixel coordinates of picture 1 to picture 2, unit
    Frobenius norm - taken as it is by ``score_matches_homography``, ``overlap_boxes_from_homography`` and
    ``rescale_homography`` after ``.reshape(-1, 3, 3)``), ``model`` ``[P,9]`` (the same in the normalised
    coordinates that were scored), ``corner_sq`` ``[P,4]`` (squared distances of the four corners of
    picture 1 under ``H`` and ``H_gt``), ``counts`` int32 ``[P,6]`` (list length, finite models, number of
    the selected model or -1, its inliers, the inliers of the delivered model, refit rounds accepted; all
    -1 for a pair whose sizes are not whole numbers in 1..8192), ``inliers`` uint8 ``[M]`` of the DELIVERED
    models (absent with ``inliers=False``), and ``workspace`` (all models float64 ``[P,n_models,9]``, then
    their inlier counts int32 ``[P,n_models]``).  A pair without a homography - fewer than 4 matches, or no
    finite model - has NaN ``H``, ``model`` and ``corner_sq``.

    Enqueues on torch's current stream and reads nothing back, so it can be captured into a HIP graph when
    every input is a device tensor.  ``out``: the result of an earlier call of the same sizes, written into
    again with no allocation."""
    _match_list_args(k1, k2, lengths, offsets)
    if models is None and not 1 <= int(n_hyp) <= HOMOGRAPHY_RANSAC_MAX_HYPOTHESES:
        raise ValueError(f'n_hyp must be in 1..{HOMOGRAPHY_RANSAC_MAX_HYPOTHESES}, got {n_hyp}')
    if not (math.isfinite(float(px_thr)) and float(px_thr) > 0):
        raise ValueError(f'px_thr must be finite and > 0, got {px_thr}')
    if int(refit_iters) != refit_iters or not 0 <= int(refit_iters) <= HOMOGRAPHY_RANSAC_MAX_REFIT:
        raise ValueError(f'refit_iters must be in 0..{HOMOGRAPHY_RANSAC_MAX_REFIT}, got {refit_iters}')
    if models is not None:
        shape = _shape_of(models)
        if len(shape) != 3 or shape[2] != 9 or not 1 <= shape[1] <= HOMOGRAPHY_RANSAC_MAX_MODELS:
            raise ValueError(f'models must be [P,n,9] with n in 1..{HOMOGRAPHY_RANSAC_MAX_MODELS}, got {shape}')
    dev = _device_of('estimate_homographies', (params, k1, k2, offsets, pair_ids, models))
    host_inputs = _host_names((('params', params), ('k1', k1), ('k2', k2), ('offsets', offsets),
                               ('pair_ids', pair_ids), ('models', models)), lengths)
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        k1, k2, M = _match_keypoints(k1, k2, dev, 'other inputs')
        pshape = _shape_of(params)
        if len(pshape) != 2 or pshape[1] != HOMOGRAPHY_PARAM_DOUBLES:
            raise ValueError(f'params must be [P,{HOMOGRAPHY_PARAM_DOUBLES}], got {pshape}')
        P = int(pshape[0])
        params = _upload('params', params, torch.float64, (P, HOMOGRAPHY_PARAM_DOUBLES), dev)
        offsets = _match_offsets(lengths, offsets, P, M, dev)
        if pair_ids is not None:
            pair_ids = _upload('pair_ids', pair_ids, torch.int32, (P,), dev)
        if models is not None:
            models = _upload('models', models, torch.float64, (P, _shape_of(models)[1], 9), dev)
        n_models = int(models.shape[1]) if models is not None else int(n_hyp)
        if P * n_models > 2 ** 31 - 1:
            raise ValueError('more than 2^31 - 1 models in one call')
        if out is None:
            nan = lambda *shape: torch.full(shape, math.nan, dtype=torch.float64, device=dev)
            out = {'H': nan(P, 9), 'model': nan(P, 9), 'corner_sq': nan(P, 4),
                   'counts': torch.zeros(P, HOMOGRAPHY_RANSAC_COUNTERS, dtype=torch.int32, device=dev)}
            if inliers:
                out['inliers'] = torch.zeros(M, dtype=torch.uint8, device=dev)
        elif tuple(out['model'].shape) != (P, 9) or ('inliers' in out) != bool(inliers) or (
                inliers and tuple(out['inliers'].shape) != (M,)) or out.get('n_models') != n_models:
            raise ValueError('`out` is the result of a call of other sizes (matches, pairs, models, inliers)')
        out['n_models'] = n_models
        if P == 0:
            if inliers:
                out['inliers'].zero_()
            return out
        lib = hip_engine.load_library()
        workspace = _workspace(out, int(lib.oetr_homography_ransac_workspace_bytes(P, n_models)), dev)
        _check(lib, lib.oetr_homography_ransac(
            params.data_ptr(), offsets.data_ptr(), _ptr(pair_ids), P, _ptr(k1), _ptr(k2), M,
            int(n_hyp) if models is None else 0, int(seed) & 0xFFFFFFFF, float(px_thr), int(refit_iters),
            _ptr(models), n_models if models is not None else 0, workspace.data_ptr(), workspace.numel(),
            out['model'].data_ptr(), out['H'].data_ptr(), out['corner_sq'].data_ptr(), out['counts'].data_ptr(),
            _ptr(out['inliers']) if inliers else None, _stream(dev)), 'oetr_homography_ransac')
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = (params, offsets, k1, k2, pair_ids, models)
    return out


def workspace_views(result):
    """``(models float64 [P,n_models,9], model_counts int32 [P,n_models])``: views of a result's workspace."""
    P, n = int(result['model'].shape[0]), int(result['n_models'])
    ws = result['workspace']
    models = ws[:P * n * 72].view(torch.float64).reshape(P, n, 9)
    counts = ws[P * n * 72:P * n * 76].view(torch.int32).reshape(P, n)
    return models, counts


def transfer_points(H, points, offsets=None, inverse=False):
    """The reference's ``homo_trans`` (``pr_evaluate_directly``) for landmarks, in float64: ``points``
    ``[N,2]`` ``(x, y)`` through ``H`` - ``a_r = (h_r0 x + h_r1 y) + h_r2``, ``(a0 / a2, a1 / a2)``.  ``H``:
    ``[3,3]`` / ``[9]`` for all points, or ``[P,3,3]`` / ``[P,9]`` with ``offsets`` (int ``[P+1]``: points
    ``offsets[p] .. offsets[p+1]-1`` go through ``H[p]``; points outside every list give NaN).
    ``inverse``: through the ADJUGATE of ``H`` - its inverse up to scale, which is all a homography needs,
    so no determinant is divided by.  Tensors stay on their device (torch operations: this is not a hot
    path); host arrays give a numpy array."""
    tensor = torch.is_tensor(H) or torch.is_tensor(points)
    dev = next((t.device for t in (H, points) if torch.is_tensor(t)), torch.device('cpu'))
    f = lambda x: (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))).to(
        device=dev, dtype=torch.float64)
    h, pts = f(H).reshape(-1, 9), f(points).reshape(-1, 2)
    if inverse:
        a = h
        h = torch.stack([a[:, 4] * a[:, 8] - a[:, 5] * a[:, 7], a[:, 2] * a[:, 7] - a[:, 1] * a[:, 8],
                         a[:, 1] * a[:, 5] - a[:, 2] * a[:, 4], a[:, 5] * a[:, 6] - a[:, 3] * a[:, 8],
                         a[:, 0] * a[:, 8] - a[:, 2] * a[:, 6], a[:, 2] * a[:, 3] - a[:, 0] * a[:, 5],
                         a[:, 3] * a[:, 7] - a[:, 4] * a[:, 6], a[:, 1] * a[:, 6] - a[:, 0] * a[:, 7],
                         a[:, 0] * a[:, 4] - a[:, 1] * a[:, 3]], 1)
    n = int(pts.shape[0])
    if offsets is None:
        if h.shape[0] != 1:
            raise ValueError('several homographies need `offsets`')
        rows = h.expand(n, 9)
        listed = None
    else:
        off = (offsets if torch.is_tensor(offsets) else torch.as_tensor(np.asarray(offsets))).to(dev).to(torch.int64)
        if off.numel() != h.shape[0] + 1:
            raise ValueError(f'offsets must hold {h.shape[0] + 1} entries, got {off.numel()}')
        at = torch.arange(n, device=dev)
        pair = torch.searchsorted(off, at, right=True) - 1
        listed = (pair >= 0) & (pair < h.shape[0])
        rows = h[pair.clamp(0, max(h.shape[0] - 1, 0))] if h.shape[0] else h.new_zeros(n, 9)
    x, y = pts[:, 0], pts[:, 1]
    a0 = (rows[:, 0] * x + rows[:, 1] * y) + rows[:, 2]
    a1 = (rows[:, 3] * x + rows[:, 4] * y) + rows[:, 5]
    a2 = (rows[:, 6] * x + rows[:, 7] * y) + rows[:, 8]
    res = torch.stack([a0 / a2, a1 / a2], 1)
    if listed is not None:
        res = torch.where(listed[:, None], res, torch.full_like(res, math.nan))
    return res if tensor else res.numpy()
