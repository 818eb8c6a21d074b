"""A least-squares refit of relative poses on their inliers, on the device: the step between ``estimate_poses``
and the reference's AUC@5/10/20.

``estimate_poses`` (``oetr_pose_ransac``) delivers the bare model of a minimal 7-point sample; at an inlier
threshold near the noise level that model usually has fewer inliers than the true essential matrix.
:func:`refine_poses` takes such models - ``estimate_poses(...)['model']``, or any others - and the same match
lists, runs a fixed number of least-squares rounds on each model's inliers in one HIP call (``oetr_pose_refit``,
ONE kernel, no workspace) and returns what ``estimate_poses`` returns, so ``evaluate.pose_errors`` /
``pose_auc`` / ``match_pose_auc`` take its result as it is.  ``estimate_poses`` and its results do not change.
``include/oetr_pose_refit.h`` has the contract, ``csrc/pose_refit.hip`` the kernel; the arithmetic is the
float64 specification of DESIGN 9.3m, reproduced bit for bit.  It is the project's own statement - an 8-unknown
linear least-squares fit with a specified summation order, accepted only when it loses no inlier - and claims no
parity with OpenCV.  There is no CPU implementation.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import math

import torch

from . import hip_engine
from ._inputs import (_device_of, _host_names, _match_keypoints, _match_list_args, _match_offsets, _ptr,
                      _refuse_host_inputs_in_capture, _shape_of, _upload)
from .hip_engine import MATCH_SCORE_PARAM_DOUBLES, POSE_REFIT_COUNTERS, POSE_REFIT_MAX_ITERS, _check, _stream


@torch.no_grad()
def refine_poses(params, k1, k2, models, lengths=None, offsets=None, px_thr=1.0, refit_iters=4, inliers=True,
                 out=None):
    """Refit the models of ``P`` pairs on their inliers and decompose them, all in one device call.

    ``params``: float64 ``[P,20]`` blocks (``match_params``).  ``k1`` / ``k2``: the lists concatenated,
    ``[M,2]`` ``(u, v)`` in the original pictures, float32 or float16 (widened; exact) - device tensors are
    taken as they are, host arrays are uploaded; float64 is refused.  ``models``: float64 ``[P,9]``, one
    fundamental matrix of the NORMALISED coordinates per pair, e.g. ``estimate_poses(...)['model']`` as it
    is; a pair whose model is not finite gets no pose.  Exactly one of ``lengths`` (a host sequence, one
    length per pair, summing to ``M``) and ``offsets`` (a device int32 ``[P+1]`` tensor) -
    ``assemble_matches``' ``k1``, ``k2`` and ``offsets`` are taken as they are.  ``px_thr``: the inlier
    threshold in pixels, ``estimate_poses``' test.  ``refit_iters``: least-squares rounds, 0..8; a round's
    candidate replaces the model only if it is finite and has at least as many inliers, otherwise the
    rounds stop - the delivered model never has fewer inliers than the one given.  ``refit_iters=0``
    decomposes the models as they are.

    Returns device tensors: ``model`` float64 ``[P,9]`` (the delivered model), ``pose`` ``[P,12]`` (``R`` row
    major, then the unit ``t``), ``cosines`` ``[P,2]`` (as ``estimate_poses``), ``counts`` int32 ``[P,5]``
    (list length, inliers of the model given, rounds accepted or -1 without a pose, inliers of the
    delivered model, the cheirality votes of the chosen candidate), ``inliers`` uint8 ``[M]`` of the
    DELIVERED models (absent with ``inliers=False``).  A pair without a pose - a list of 0 rows, or a model
    that is not finite - has NaN ``model``, ``pose`` and ``cosines`` and ``counts[:, 2] == -1``.

    Enqueues on torch's current stream and reads nothing back, so it can be captured into a HIP graph when
    every input is a device tensor.  ``out``: the result of an earlier call of the same sizes, written into
    again with no allocation."""
    _match_list_args(k1, k2, lengths, offsets)
    if not (math.isfinite(float(px_thr)) and float(px_thr) > 0):
        raise ValueError(f'px_thr must be finite and > 0, got {px_thr}')
    if int(refit_iters) != refit_iters or not 0 <= int(refit_iters) <= POSE_REFIT_MAX_ITERS:
        raise ValueError(f'refit_iters must be in 0..{POSE_REFIT_MAX_ITERS}, got {refit_iters}')
    mshape = _shape_of(models)
    if len(mshape) != 2 or mshape[1] != 9:
        raise ValueError(f'models must be [P,9], got {mshape}')
    dev = _device_of('refine_poses', (params, k1, k2, offsets, models))
    host_inputs = _host_names((('params', params), ('k1', k1), ('k2', k2), ('offsets', offsets), ('models', models)),
                              lengths)
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        k1, k2, M = _match_keypoints(k1, k2, dev, 'other inputs')
        pshape = _shape_of(params)
        if len(pshape) != 2 or pshape[1] != MATCH_SCORE_PARAM_DOUBLES:
            raise ValueError(f'params must be [P,{MATCH_SCORE_PARAM_DOUBLES}], got {pshape}')
        P = int(pshape[0])
        params = _upload('params', params, torch.float64, (P, MATCH_SCORE_PARAM_DOUBLES), dev)
        offsets = _match_offsets(lengths, offsets, P, M, dev)
        models = _upload('models', models, torch.float64, (P, 9), dev)
        if out is None:
            nan = lambda *shape: torch.full(shape, math.nan, dtype=torch.float64, device=dev)
            out = {'model': nan(P, 9), 'pose': nan(P, 12), 'cosines': nan(P, 2),
                   'counts': torch.zeros(P, POSE_REFIT_COUNTERS, dtype=torch.int32, device=dev)}
            if inliers:
                out['inliers'] = torch.zeros(M, dtype=torch.uint8, device=dev)
        elif tuple(out['model'].shape) != (P, 9) or ('inliers' in out) != bool(inliers) or (
                inliers and tuple(out['inliers'].shape) != (M,)):
            raise ValueError('`out` is the result of a call of other sizes (matches, pairs, inliers)')
        if out['model'].data_ptr() == models.data_ptr() and P:
            raise ValueError('`models` is the `model` of `out`: an output may not overlap an input')
        if P == 0:
            if inliers:
                out['inliers'].zero_()
            return out
        lib = hip_engine.load_library()
        _check(lib, lib.oetr_pose_refit(
            params.data_ptr(), offsets.data_ptr(), P, _ptr(k1), _ptr(k2), M, models.data_ptr(), float(px_thr),
            int(refit_iters), out['model'].data_ptr(), out['pose'].data_ptr(), out['cosines'].data_ptr(),
            out['counts'].data_ptr(), _ptr(out['inliers']) if inliers else None, _stream(dev)), 'oetr_pose_refit')
        # what the enqueued kernel reads stays referenced as long as the result does
        out['_inputs'] = (params, offsets, k1, k2, models)
    return out
