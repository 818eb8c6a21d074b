"""Recall of ``forward_dummy``'s boxes against ground-truth overlap boxes: the reference's
``evaluate_dummy`` (``src/utils/validation.py:111-146``, ``_recalls`` ``:20-25``).

For every batch the model predicts two boxes per pair; each is scored against the pair's
ground-truth co-visibility box by aligned IoU (or by the overlap's share of the ground-truth box,
``oiou``).  All ``2N`` values count - pairs without any co-visible pixel (a zero ground-truth box)
included, as in the reference - and the recall at a threshold is the share of values at or above it.

The ground truth comes from the batch (``overlap_box1`` / ``overlap_box2``, what the reference's
dataset emits) or is computed on the device from depth maps, intrinsics and poses
(``covis.overlap_boxes_from_batch``) or from a homography
(``homography.overlap_boxes_from_homography``).  ``evaluate_indexed`` scores the feature-bank route the same
way: a pair list over an image set, the ground truth by index from a ``covis_set.DepthSet``.
``match_precision`` summarises ``match_score.score_matches``: the reference's ``validation_error``
precision per pair, from one read of the counters.  ``keypoint_repeatability`` summarises
``keypoint_score.score_keypoints`` the same way: the reference's repeatability per pair and threshold.
``pose_errors`` / ``pose_auc`` / ``match_pose_auc`` summarise ``pose_ransac.estimate_poses``: the reference's
``compute_pose_error`` per pair and its AUC of the pose error.
"""
import numpy as np
import torch

from .covis import overlap_boxes_from_batch
from .covis_set import overlap_boxes_indexed
from .homography import overlap_boxes_from_homography
from .losses import bbox_iou_aligned, bbox_oiou
from .pipeline import _model_device, forward_pairs_indexed

DEFAULT_IOU_THRS = np.arange(0.5, 0.96, 0.05)


def count_recalls(ious, iou_thrs):
    """``ious`` [M] (any float dtype, any device) -> int64 [len(iou_thrs)] on that device: how many
    values are ``>= thr``, compared in float64 as numpy compares a float32 array with a float64
    threshold.  No host read."""
    thrs = torch.as_tensor(np.asarray(iou_thrs, dtype=np.float64), device=ious.device)
    return (ious.to(torch.float64)[:, None] >= thrs[None, :]).sum(0)


def score_boxes(produced, iou_thrs, oiou=False, logger=None):
    """The scoring tail both evaluators share.  ``produced``: a list of ``(gt_box1, gt_box2, valid or None,
    pred_box1, pred_box2)`` with SETTLED float32 ``[n,4]`` boxes on one device -> the result dict of
    :func:`evaluate_dummy`.  IoUs and the per-threshold counts stay on the device; one read."""
    thrs = np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    if not produced:
        return {'recalls': np.zeros(thrs.size), 'n': 0, 'mean_iou': float('nan'), 'n_valid_pairs': 0}
    score = bbox_oiou if oiou else bbox_iou_aligned
    ious, n_valid = [], 0
    for gt1, gt2, valid, pred1, pred2 in produced:
        ious += [score(gt1, pred1), score(gt2, pred2)]
        if valid is None:
            valid = (gt1 != 0).any(1) | (gt2 != 0).any(1)
        n_valid = n_valid + valid.sum()
    ious = torch.cat(ious)
    n = int(ious.numel())
    # counts, the IoU sum and the valid pairs in ONE float64 tensor (exact for these integers): one read
    packed = torch.cat([count_recalls(ious, thrs).to(torch.float64), ious.to(torch.float64).nansum()[None],
                        n_valid.to(torch.float64)[None]]).cpu().numpy()
    recalls = packed[:thrs.size] / float(n)
    if logger is not None and thrs.size > 8:
        logger.info('Validation results:')
        logger.info('Recalls\t R0.5\t R0.75\t R0.9\t')
        logger.info('Values\t {:.5f}\t {:.5f}\t {:.5f}\t'.format(recalls[0], recalls[5], recalls[8]))
    return {'recalls': recalls, 'n': n, 'mean_iou': float(packed[thrs.size] / n),
            'n_valid_pairs': int(packed[thrs.size + 1])}


@torch.no_grad()
def evaluate_dummy(model, batches, iou_thrs=DEFAULT_IOU_THRS, oiou=False, gt='auto', logger=None):
    """``batches``: an iterable of dataset-style dicts with ``image1`` / ``image2`` ``[N,H,W,3]`` in
    [0,1] and the ground truth: ``overlap_box1`` / ``overlap_box2`` ``[N,4]`` (``gt='batch'``), or
    ``depth1``, ``intrinsics1``, ``pose1``, ``bbox1``, ``ratio1`` and the same for ``2`` (``gt='depth'``:
    the boxes are computed on the device), or ``homography`` ``[N,3,3]`` (``gt='homography'``: the
    homography from ``image1`` to ``image2`` in the frame of the two images AS GIVEN, pixel centres at
    integer coordinates; the boxes are ``homography.overlap_boxes_from_homography``'s, computed on the
    device).  ``gt='auto'`` takes the batch's boxes where it has them, else the depth route.

    Returns ``{'recalls': ndarray[len(iou_thrs)], 'n': number of scored boxes (2 per pair),
    'mean_iou': float (a NaN score - ``oiou`` against a zero box - counts as 0, as it fails every
    threshold), 'n_valid_pairs': int}`` - pairs whose ground truth is valid: ``overlap_valid``
    where the ground truth carries it (always for ``gt='depth'`` and ``gt='homography'``), otherwise pairs with a non-zero
    ground-truth box.  With a ``logger`` the reference's table (R0.5, R0.75, R0.9: entries 0, 5, 8 of
    the default thresholds) is logged.

    Boxes are scored only once SETTLED: ``forward_dummy`` defers its range check
    (``OETR.hip_defer_check``) and corrects a tripped batch in place later, so the batches' box
    tensors are kept and scored after one ``model.hip_flush()`` at the end, as
    ``pipeline.forward_pairs_raw`` does.  IoUs and the per-threshold counts stay on the device; the
    whole evaluation reads the device once."""
    if gt not in ('auto', 'batch', 'depth', 'homography'):
        raise ValueError(f"gt must be 'auto', 'batch', 'depth' or 'homography', got {gt!r}")
    thrs = np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    device = _model_device(model)
    produced = []          # (gt_box1, gt_box2, valid or None, pred_box1, pred_box2) per batch
    for batch in batches:
        image1 = batch['image1'].to(device, non_blocking=True)
        image2 = batch['image2'].to(device, non_blocking=True)
        pred1, pred2 = model.forward_dummy(image1, image2)
        has_boxes = 'overlap_box1' in batch and 'overlap_box2' in batch
        if gt == 'batch' and not has_boxes:
            raise KeyError("gt='batch': the batch has no overlap_box1 / overlap_box2")
        if gt == 'homography':
            if 'homography' not in batch:
                raise KeyError("gt='homography': the batch has no homography")
            truth = overlap_boxes_from_homography(batch['homography'], size1=tuple(image1.shape[1:3]),
                                                  size2=tuple(image2.shape[1:3]))
        elif gt == 'depth' or not has_boxes:
            truth = overlap_boxes_from_batch(batch)
        else:
            truth = batch
        box = lambda t: torch.as_tensor(t).to(device=pred1.device, dtype=torch.float32, non_blocking=True)
        valid = truth.get('overlap_valid')
        if valid is not None:
            valid = torch.as_tensor(valid).to(pred1.device, non_blocking=True).reshape(-1) != 0
        produced.append((box(truth['overlap_box1']), box(truth['overlap_box2']), valid, pred1, pred2))
    flush = getattr(model, 'hip_flush', None)
    if flush is not None:
        flush()
    return score_boxes(produced, thrs, oiou, logger)


@torch.no_grad()
def evaluate_indexed(model, images, depth_set, pair_index, iou_thrs=DEFAULT_IOU_THRS, oiou=False, max_batch=8,
                     logger=None):
    """:func:`evaluate_dummy` for a pair LIST over an image SET: the boxes by
    ``pipeline.forward_pairs_indexed(model, images, pair_index, max_batch)`` (trunk and neck once per
    image, mixed sizes), the ground truth by ``covis_set.overlap_boxes_indexed(depth_set, pair_index)``
    - slot k of ``depth_set`` holds the depth map and camera of ``images[k]``, read in place.
    ``pair_index``: a host sequence of ``(i, j)``.  Returns the same dict with the same counting (all
    ``2 * len(pair_index)`` boxes count; ``n_valid_pairs`` from ``overlap_valid``).  The boxes are scored
    settled - ``forward_pairs_indexed`` ends with its one ``model.hip_flush()`` - and the scoring reads the
    device once."""
    thrs = np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    pair_index = [(int(i), int(j)) for i, j in pair_index]
    if not pair_index:
        return score_boxes([], thrs, oiou, logger)
    if len(images) != len(depth_set):
        raise ValueError(f'{len(images)} images, {len(depth_set)} depth maps: slot k of the set must hold the depth '
                         'map of images[k]')
    truth = overlap_boxes_indexed(depth_set, pair_index)
    pred1, pred2 = forward_pairs_indexed(model, images, pair_index, max_batch=max_batch)
    to = lambda t: t.to(pred1.device, non_blocking=True)
    return score_boxes([(to(truth['overlap_box1']), to(truth['overlap_box2']), to(truth['overlap_valid']), pred1, pred2)],
                       thrs, oiou, logger)


def match_precision(result):
    """The reference's ``validation_error`` summary (``dloc/evaluate/utils/evaluation.py``) of a
    ``match_score.score_matches`` result, from ONE device read of its ``counts`` int32 ``[P,5]``
    (a tensor or an array of that shape is taken as well).  Per pair ``precision`` = the matches with
    ``epi_ref < epi_thr`` over the matches, 0 for an empty list as in the reference; pairs the set did
    not vouch for (all counters -1) are EXCLUDED - NaN in the per-pair arrays - and counted in
    ``n_not_scored``.  ``reproj_precision`` is the same for the re-projection counter over the matches
    with both depths (``counts[:,4] / counts[:,3]``).  A summary whose threshold was off is ``None``.

    Returns ``{'precision': float64 [P] or None, 'mean_precision': float or None, 'reproj_precision':
    float64 [P] or None, 'mean_reproj_precision': float or None, 'n_pairs': scored pairs,
    'n_not_scored': int, 'n_matches': matches of the scored pairs, 'n_both_depths': int}``; a mean over
    no scored pair is NaN."""
    counts = result['counts'] if isinstance(result, dict) else result
    counts = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    counts = counts.reshape(-1, 5).astype(np.int64)
    scored = counts[:, 0] >= 0

    def share(hit, of):
        if scored.any() and (hit[scored] < 0).any():          # that threshold was off
            return None, None
        per_pair = np.full(counts.shape[0], np.nan)
        some = scored & (of > 0)
        per_pair[scored] = 0.0
        per_pair[some] = hit[some] / of[some]
        return per_pair, float(per_pair[scored].mean()) if scored.any() else float('nan')

    precision, mean_precision = share(counts[:, 1], counts[:, 0])
    reproj, mean_reproj = share(counts[:, 4], counts[:, 3])
    return {'precision': precision, 'mean_precision': mean_precision, 'reproj_precision': reproj,
            'mean_reproj_precision': mean_reproj, 'n_pairs': int(scored.sum()), 'n_not_scored': int((~scored).sum()),
            'n_matches': int(counts[scored, 0].sum()), 'n_both_depths': int(counts[scored, 3].sum())}


def keypoint_repeatability(result):
    """The reference's repeatability (``pose_evaluate``, ``dloc/evaluate/utils/evaluation.py:170-179``;
    ``get_repeatability``, ``utils.py:214-236``) of a ``keypoint_score.score_keypoints`` result, from ONE
    device read of its ``counts`` int32 ``[P,2,2+T]`` (a tensor or an array of that shape is taken as
    well).  Per pair and threshold ``repeatability`` = ``(c12 / kept12 + c21 / kept21) / 2``: per
    direction the kept keypoints with a keypoint of the other picture closer than the threshold over
    the kept keypoints, a direction that kept nothing contributing 0 as in the reference.  Pairs that
    were not vouched for (all counters -1) are EXCLUDED - NaN rows - and counted in ``n_not_scored``.

    Returns ``{'repeatability': float64 [P,T], 'mean_repeatability': float64 [T] (NaN over no scored
    pair), 'thresholds': the result's (None for a bare array), 'n_pairs': scored pairs, 'n_not_scored':
    int, 'n_keypoints': keypoints of the scored pairs, both directions, 'n_kept': int}``."""
    counts = result['counts'] if isinstance(result, dict) else result
    thresholds = result.get('thresholds') if isinstance(result, dict) else None
    counts = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if counts.ndim != 3 or counts.shape[1] != 2 or counts.shape[2] < 2:
        raise ValueError(f'counts must be [P,2,2+T], got {counts.shape}')
    counts = counts.astype(np.int64)
    scored = counts[:, 0, 0] >= 0
    kept = counts[:, :, 1:2]
    share = np.where(kept > 0, counts[:, :, 2:] / np.maximum(kept, 1), 0.0)
    per_pair = (share[:, 0] + share[:, 1]) / 2
    per_pair[~scored] = np.nan
    mean = per_pair[scored].mean(0) if scored.any() else np.full(counts.shape[2] - 2, np.nan)
    return {'repeatability': per_pair, 'mean_repeatability': mean, 'thresholds': thresholds,
            'n_pairs': int(scored.sum()), 'n_not_scored': int((~scored).sum()),
            'n_keypoints': int(counts[scored, :, 0].sum()), 'n_kept': int(counts[scored, :, 1].sum())}


def pose_errors(result):
    """The reference's ``compute_pose_error`` (``dloc/evaluate/utils/evaluation.py``: ``angle_error_mat``,
    ``angle_error_vec``) of a ``pose_ransac.estimate_poses`` result, from ONE device read of its
    ``cosines`` and ``counts``: the cosines clipped to +-1, ``arccos`` - the one transcendental of the
    route, left to the host - in degrees, ``err_t = min(e, 180 - e)``.  A pair without a pose (selected
    model -1, or cosines that are not finite) gives ``inf``, as ``validation_error`` does.

    Returns ``{'err_R', 'err_t', 'pose_error': float64 [P]}`` with ``pose_error = max(err_t, err_R)`` as
    ``eval_megadepth.py`` forms it."""
    cos, counts = result['cosines'], result['counts']
    if torch.is_tensor(cos):
        # both in ONE float64 tensor (exact for these integers): one read
        packed = torch.cat([cos.reshape(-1, 2), counts.reshape(-1, 5).to(torch.float64)], 1).cpu().numpy()
        cos, counts = packed[:, :2], packed[:, 2:]
    cos, counts = np.asarray(cos, np.float64).reshape(-1, 2), np.asarray(counts).reshape(-1, 5)
    none = ~np.isfinite(cos).all(1) | (counts[:, 2] < 0)
    with np.errstate(all='ignore'):
        c = np.clip(np.where(none[:, None], 1.0, cos), -1.0, 1.0)
        err_R = np.rad2deg(np.abs(np.arccos(c[:, 0])))
        e = np.rad2deg(np.arccos(c[:, 1]))
        err_t = np.minimum(e, 180 - e)
    err_R, err_t = np.where(none, np.inf, err_R), np.where(none, np.inf, err_t)
    return {'err_R': err_R, 'err_t': err_t, 'pose_error': np.maximum(err_t, err_R)}


def pose_auc(errors, thresholds=(5, 10, 20)):
    """The area under the recall curve of the pose errors up to each threshold, over the threshold - what
    the reference's ``pose_auc`` (``dloc/evaluate/utils/utils.py``) computes.  The curve rises from (0, 0)
    through ``(e_i, i / n)`` for the errors in ascending order (degrees; ``inf`` for a pair without a pose);
    the ``k`` errors strictly below a threshold ``t`` each close one trapezoid, and a flat piece at ``k / n``
    runs from the last of them to ``t``.  ``errors``: an array, or the dict :func:`pose_errors` returns.
    -> a list, one value in [0, 1] per threshold; NaN for no pairs."""
    errors = errors['pose_error'] if isinstance(errors, dict) else errors
    ascending = np.sort(np.asarray(errors, np.float64).reshape(-1))
    n = len(ascending)
    if n == 0:
        return [float('nan') for _ in thresholds]
    aucs = []
    for t in thresholds:
        below = int(np.count_nonzero(ascending < t))
        area, at_e, at_r = 0.0, 0.0, 0.0
        for i in range(below):                            # added in ascending order
            share = (i + 1) / n
            area = area + (ascending[i] - at_e) * (share + at_r) / 2.0
            at_e, at_r = ascending[i], share
        area = area + (t - at_e) * (at_r + at_r) / 2.0
        aucs.append(float(area / t))
    return aucs


def match_pose_auc(result, thresholds=(5, 10, 20)):
    """:func:`pose_errors` and :func:`pose_auc` together, times 100, as ``eval_megadepth.py`` prints it:
    ``{'auc': [AUC@5, AUC@10, AUC@20], 'thresholds', 'pose_error', 'err_R', 'err_t', 'n_pairs', 'n_no_pose'}``."""
    errs = pose_errors(result)
    return {'auc': [100.0 * a for a in pose_auc(errs['pose_error'], thresholds)], 'thresholds': tuple(thresholds),
            'n_pairs': int(errs['pose_error'].size), 'n_no_pose': int(np.isinf(errs['pose_error']).sum()), **errs}


def homography_errors(result):
    """The mean corner error per pair of a ``homography_ransac.estimate_homographies`` result, from ONE device
    read of its ``corner_sq`` and ``counts``: the square roots of the four squared corner distances - left to
    the host, the project's standing departure - added in corner order, over 4, in pixels of picture 2.  A pair
    without a homography (selected model -1), without ground truth, or with a corner on the horizon line (a
    distance that is not finite) gives ``inf``.  -> float64 ``[P]``."""
    sq, counts = result['corner_sq'], result['counts']
    if torch.is_tensor(sq):
        # both in ONE float64 tensor (exact for these integers): one read
        packed = torch.cat([sq.reshape(-1, 4), counts.reshape(-1, 6).to(torch.float64)], 1).cpu().numpy()
        sq, counts = packed[:, :4], packed[:, 4:]
    sq, counts = np.asarray(sq, np.float64).reshape(-1, 4), np.asarray(counts).reshape(-1, 6)
    none = ~np.isfinite(sq).all(1) | (counts[:, 2] < 0)
    with np.errstate(all='ignore'):
        d = np.sqrt(np.where(none[:, None], 0.0, sq))
        mean = (((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]) / 4.0
    return np.where(none, np.inf, mean)


def homography_auc(errors, thresholds=(3, 5, 10)):
    """:func:`pose_auc` of mean corner errors in pixels: the area under the recall curve up to each threshold,
    over the threshold.  ``errors``: an array as :func:`homography_errors` returns it."""
    return pose_auc(np.asarray(errors, np.float64), thresholds)


def match_homography_auc(result, thresholds=(3, 5, 10)):
    """:func:`homography_errors` and :func:`homography_auc` together, times 100:
    ``{'auc': [AUC@3, AUC@5, AUC@10], 'thresholds', 'corner_error', 'n_pairs', 'n_no_homography'}``."""
    errs = homography_errors(result)
    return {'auc': [100.0 * a for a in homography_auc(errs, thresholds)], 'thresholds': tuple(thresholds),
            'corner_error': errs, 'n_pairs': int(errs.size), 'n_no_homography': int(np.isinf(errs).sum())}
