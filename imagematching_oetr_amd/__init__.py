"""MI355X-native OETR overlap-estimation hot path.

Drop-in for the inference half of TencentYoutuResearch/ImageMatching-OETR's
``src/model.py``: same ``OETR`` constructor, checkpoint keys and
``forward_dummy`` signature; the feature-correlation transformer and the
centre/size regression heads run as hand-written HIP kernels for gfx950
behind the C ABI in ``include/oetr_hip.h``.
"""
import os as _os

# Streams and hardware queues: the HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES
# hardware queues (default 4), and work of two streams that share a queue is serialised.  The throughput
# mode (model.hip_streams = 3) uses three side streams + the caller's stream = four; a fifth stream (an
# asynchronous collective on the process group's stream) halved the overlapped rate (30.5 k -> 14.7 k
# pairs/s), which is why parallel.BoxGatherer issues a BLOCKING collective on the batch's own side stream
# in that mode.  More queues are not a fix: with 8 the stream -> queue assignment depends on the order in
# which torch / RCCL / this package create their streams (28-32 k by order; profiles/r5_pg_streams.txt).

from .config import Cfg, get_cfg_defaults  # noqa: F401
from .model import OETR, build_detectors  # noqa: F401
from .pipeline import crop_pairs, forward_pairs, forward_pairs_indexed, forward_pairs_raw, forward_pairs_sharded  # noqa: F401
from .bank import FeatureBank  # noqa: F401
from .covis import overlap_boxes_from_batch, overlap_boxes_from_depth  # noqa: F401
from .covis_set import DepthSet, mine_pairs, overlap_boxes_indexed  # noqa: F401
from .crop_batch import OverlapCropBatch, crop_pair_table, keypoints_to_origin, overlap_crop_batch  # noqa: F401
from .evaluate import (evaluate_dummy, evaluate_indexed, homography_auc, homography_errors, keypoint_repeatability,  # noqa: F401
                       match_homography_auc, match_pose_auc, match_precision, pose_auc, pose_errors)
from .match_score import match_params, score_matches  # noqa: F401
from .keypoint_score import ground_truth_matches, score_keypoints  # noqa: F401
from .match_assembly import assemble_matches, few_match_pairs  # noqa: F401
from .homography import (homography_accuracy, homography_params, overlap_boxes_from_homography,  # noqa: F401
                         rescale_homography, score_matches_homography)
from .pose_ransac import estimate_poses  # noqa: F401
from .pose_refit import refine_poses  # noqa: F401
from .homography_ransac import estimate_homographies, transfer_points  # noqa: F401
from .nn_match import match_counts, match_descriptors  # noqa: F401
from .dense_match import dense_match_counts, match_dense  # noqa: F401
from .fine_match import fine_match_counts, fine_windows, refine_matches  # noqa: F401
from .keypoint_select import keypoint_counts, keypoint_map_table, select_keypoints  # noqa: F401
from .reader import overlap_frame, read_overlap_images  # noqa: F401
from .hip_engine import (FLAG_EXCHANGE, FLAG_F16_RANGE, FLAG_INDEX, FLAG_INVALID, FULL_ATTENTION_VARIANTS, HotPathEngine, KernelTrace, NeckEngine, OetrError,  # noqa: F401
                         OetrExchangeError, OetrRangeError,
                         box_tlbr_to_xyxy, full_attention, hot_path_keys,
                         linear_attention, load_library, neck_keys, overlap_crop)

__all__ = ['Cfg', 'get_cfg_defaults', 'OETR', 'build_detectors',
           'HotPathEngine', 'KernelTrace', 'NeckEngine', 'neck_keys', 'OetrError', 'OetrExchangeError', 'OetrRangeError', 'FLAG_F16_RANGE', 'FLAG_EXCHANGE', 'FLAG_INVALID', 'box_tlbr_to_xyxy', 'full_attention',
           'linear_attention', 'FULL_ATTENTION_VARIANTS', 'hot_path_keys', 'load_library', 'overlap_crop', 'forward_pairs',
           'forward_pairs_sharded', 'forward_pairs_raw', 'forward_pairs_indexed', 'FeatureBank', 'FLAG_INDEX', 'overlap_frame', 'read_overlap_images',
           'overlap_boxes_from_depth', 'overlap_boxes_from_batch', 'evaluate_dummy',
           'DepthSet', 'overlap_boxes_indexed', 'mine_pairs', 'evaluate_indexed',
           'crop_pair_table', 'overlap_crop_batch', 'OverlapCropBatch', 'keypoints_to_origin', 'crop_pairs',
           'score_matches', 'match_params', 'match_precision',
           'score_keypoints', 'keypoint_repeatability', 'ground_truth_matches',
           'assemble_matches', 'few_match_pairs',
           'homography_params', 'rescale_homography', 'score_matches_homography', 'homography_accuracy',
           'overlap_boxes_from_homography',
           'estimate_poses', 'refine_poses', 'pose_errors', 'pose_auc', 'match_pose_auc',
           'match_descriptors', 'match_counts',
           'keypoint_map_table', 'select_keypoints', 'keypoint_counts',
           'match_dense', 'dense_match_counts',
           'fine_windows', 'refine_matches', 'fine_match_counts',
           'estimate_homographies', 'transfer_points', 'homography_errors', 'homography_auc', 'match_homography_auc']
