"""The pinned calls of keypoint selection: what ``tools/gen_golden_keypoint_select.py`` records in
``tests/keypoint_select_expected.json`` and ``tests/test_keypoint_select_cpu.py`` regenerates.  numpy only.

Every score map holds pairwise distinct positive scores (a permutation of an arithmetic sequence), so ``torch.topk``
and ``nonzero`` have one answer and the torch restatement can be compared for equality."""
import hashlib

import numpy as np

import keypoint_select_oracle as kso

F32 = np.float32

# name, (H, W), D, (h, w), nms_radius, threshold, remove_borders, max_keypoints, cell, seed
PINNED = (
    ('all_kept_raster', (40, 56), 8, (5, 7), 4, 0.005, 4, 4096, 8, 1),
    ('top_16', (40, 56), 8, (5, 7), 4, 0.005, 4, 16, 8, 1),
    ('taps_outside_d68', (50, 70), 68, (5, 7), 2, 0.3, 0, 64, 8, 2),
    ('radius_0', (24, 31), 4, (3, 4), 0, 0.5, 1, 4096, 8, 3),
    ('radius_1_cell_4', (24, 31), 4, (6, 8), 1, 0.005, 2, 50, 4, 4),
    ('radius_8', (37, 45), 256, (5, 6), 8, 0.005, 0, 4096, 8, 5),
    ('single_row', (1, 64), 4, (1, 8), 3, 0.005, 0, 7, 8, 6),
)


def distinct_scores(seed, H, W):
    """``[H,W]`` float32, pairwise distinct, in (0, 1]: a permutation of ``(i + 1) / (H * W)``."""
    rng = np.random.default_rng(seed)
    return ((rng.permutation(H * W) + 1).astype(np.float64) / (H * W)).astype(F32).reshape(H, W)


def descriptor_map(seed, D, h, w):
    return np.random.default_rng(1000 + seed).standard_normal((D, h, w)).astype(F32)


def inputs(case):
    _, (H, W), D, (h, w), _, _, _, _, _, seed = case
    return distinct_scores(seed, H, W), descriptor_map(seed, D, h, w)


def parameters(case):
    _, _, _, _, r, thr, border, k, cell, _ = case
    return dict(nms_radius=r, threshold=thr, remove_borders=border, max_keypoints=k, cell=cell)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(case):
    """What the fixture holds of one pinned call: the counters, the kept raster indices in output order, the scores'
    bit patterns and a digest of the descriptors' bytes."""
    S, F = inputs(case)
    res = kso.select_image(S, F, **parameters(case))
    kp = res['keypoints'].astype(np.int64)
    return dict(name=case[0], counts=[int(c) for c in res['counts']],
                raster=[int(v) for v in kp[:, 1] * S.shape[1] + kp[:, 0]],
                score_bits=[int(v) for v in res['scores'].view(np.uint32)],
                descriptors_sha256=digest(res['descriptors']))
