"""Relative pose from match lists by RANSAC on the device: the step before the reference's AUC@5/10/20.

The reference's ``validation_error`` -> ``estimate_pose`` -> ``compute_pose_error``
(``dloc/evaluate/utils/evaluation.py``) runs ``cv2.findEssentialMat(RANSAC)`` and ``cv2.recoverPose`` per
pair on the host.  :func:`estimate_poses` estimates the relative pose of MANY match lists in one HIP call
(``oetr_pose_ransac``) and leaves the two cosines of the pose error on the device;
``evaluate.pose_errors`` / ``pose_auc`` / ``match_pose_auc`` turn them into the reference's numbers from
one read.  ``include/oetr_pose_ransac.h`` has the contract, ``csrc/pose_ransac.hip`` the kernels; the
arithmetic is the float64 specification of DESIGN 9.3j, reproduced bit for bit.  It is the project's own
statement - a 7-point solver, a fixed number of hypotheses, no refinement - and claims no parity with
OpenCV.  There is no CPU implementation.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import math

import torch

from . import hip_engine
from ._inputs import (_device_of, _host_names, _match_keypoints, _match_list_args, _match_offsets, _ptr,
                      _refuse_host_inputs_in_capture, _shape_of, _upload, _workspace)
from .hip_engine import (MATCH_SCORE_PARAM_DOUBLES, POSE_RANSAC_COUNTERS, POSE_RANSAC_MAX_HYPOTHESES,
                         POSE_RANSAC_MAX_MODELS, _check, _stream)


@torch.no_grad()
def estimate_poses(params, k1, k2, lengths=None, offsets=None, n_hyp=256, px_thr=1.0, seed=0, pair_ids=None,
                   models=None, inliers=True, out=None):
    """Estimate the relative pose of ``P`` pairs from their match lists, all in one device call.

    ``params``: float64 ``[P,20]`` blocks (``match_params``: fx fy cx cy of both cameras, ``R`` and ``t`` of
    ``T_1to2``).  ``k1`` / ``k2``: the lists concatenated, ``[M,2]`` ``(u, v)`` in the original pictures,
    float32 or float16 (widened; exact) - device tensors are taken as they are, host arrays are uploaded;
    float64 is refused.  Exactly one of ``lengths`` (a host sequence, one length per pair, summing to ``M``)
    and ``offsets`` (a device int32 ``[P+1]`` tensor) - ``assemble_matches``' ``k1``, ``k2`` and ``offsets``
    are taken as they are.  ``n_hyp``: hypotheses per pair, 1..4096, each a 7-point sample that gives up to
    3 models; all are scored.  ``px_thr``: the inlier threshold in pixels (the reference's ``thresh``).
    ``seed`` and ``pair_ids`` (int32 ``[P]``; default: the pair's position) feed the stateless sampler: a
    caller who shards or orders the pair list differently gets the same poses by passing the same ids.
    ``models``: float64 ``[P,n,9]`` models of the caller's, ``n`` in 1..12288 - sampling and solving are
    skipped, the models are scored, selected and decomposed.

    Returns device tensors: ``model`` float64 ``[P,9]`` (the selected fundamental matrix of the normalised
    coordinates), ``pose`` ``[P,12]`` (``R`` row major, then the unit ``t``), ``cosines`` ``[P,2]``
    (``(trace(R_gt^T R) - 1) / 2`` and ``t . t_gt / (|t| |t_gt|)``, unclipped), ``counts`` int32 ``[P,5]``
    (list length, finite models, number of the selected model or -1, its inliers, the cheirality votes of
    the chosen candidate), ``inliers`` uint8 ``[M]`` (absent with ``inliers=False``), and ``workspace``
    (all models float64 ``[P,n_models,9]``, then their inlier counts int32 ``[P,n_models]``).  A pair
    without a pose - fewer than 7 matches, or no finite model - has NaN ``model``, ``pose`` and ``cosines``.

    Enqueues on torch's current stream and reads nothing back, so it can be captured into a HIP graph when
    every input is a device tensor.  ``out``: the result of an earlier call of the same sizes, written into
    again with no allocation."""
    _match_list_args(k1, k2, lengths, offsets)
    if models is None and not 1 <= int(n_hyp) <= POSE_RANSAC_MAX_HYPOTHESES:
        raise ValueError(f'n_hyp must be in 1..{POSE_RANSAC_MAX_HYPOTHESES}, got {n_hyp}')
    if not (math.isfinite(float(px_thr)) and float(px_thr) > 0):
        raise ValueError(f'px_thr must be finite and > 0, got {px_thr}')
    if models is not None:
        shape = _shape_of(models)
        if len(shape) != 3 or shape[2] != 9 or not 1 <= shape[1] <= POSE_RANSAC_MAX_MODELS:
            raise ValueError(f'models must be [P,n,9] with n in 1..{POSE_RANSAC_MAX_MODELS}, got {shape}')
    dev = _device_of('estimate_poses', (params, k1, k2, offsets, pair_ids, models))
    host_inputs = _host_names((('params', params), ('k1', k1), ('k2', k2), ('offsets', offsets),
                               ('pair_ids', pair_ids), ('models', models)), lengths)
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        k1, k2, M = _match_keypoints(k1, k2, dev, 'other inputs')
        pshape = _shape_of(params)
        if len(pshape) != 2 or pshape[1] != MATCH_SCORE_PARAM_DOUBLES:
            raise ValueError(f'params must be [P,{MATCH_SCORE_PARAM_DOUBLES}], got {pshape}')
        P = int(pshape[0])
        params = _upload('params', params, torch.float64, (P, MATCH_SCORE_PARAM_DOUBLES), dev)
        offsets = _match_offsets(lengths, offsets, P, M, dev)
        if pair_ids is not None:
            pair_ids = _upload('pair_ids', pair_ids, torch.int32, (P,), dev)
        if models is not None:
            models = _upload('models', models, torch.float64, (P, _shape_of(models)[1], 9), dev)
        n_models = int(models.shape[1]) if models is not None else 3 * int(n_hyp)
        if P * n_models > 2 ** 31 - 1:
            raise ValueError('more than 2^31 - 1 models in one call')
        if out is None:
            nan = lambda *shape: torch.full(shape, math.nan, dtype=torch.float64, device=dev)
            out = {'model': nan(P, 9), 'pose': nan(P, 12), 'cosines': nan(P, 2),
                   'counts': torch.zeros(P, POSE_RANSAC_COUNTERS, dtype=torch.int32, device=dev)}
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
        workspace = _workspace(out, int(lib.oetr_pose_ransac_workspace_bytes(P, n_models)), dev)
        _check(lib, lib.oetr_pose_ransac(
            params.data_ptr(), offsets.data_ptr(), _ptr(pair_ids), P, _ptr(k1), _ptr(k2), M,
            int(n_hyp) if models is None else 0, int(seed) & 0xFFFFFFFF, float(px_thr), _ptr(models),
            n_models if models is not None else 0, workspace.data_ptr(), workspace.numel(), out['model'].data_ptr(),
            out['pose'].data_ptr(), out['cosines'].data_ptr(), out['counts'].data_ptr(),
            _ptr(out['inliers']) if inliers else None, _stream(dev)), 'oetr_pose_ransac')
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
