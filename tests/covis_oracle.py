"""float64 numpy restatement of the co-visibility boxes (``include/oetr_covis.h``), written from the
specification, and the synthetic scenes the covis tests, the generator of the pinned scenes
(``tools/gen_golden_covis.py``) and the probe (``tools/covis_probe.py``) share.

``overlap_box`` also reports a pair's DECISION MARGIN: the smallest distance of any tested quantity
to its threshold (``u2`` / ``v2`` to the nearest integer, ``|Zc - depth2|`` to 0.5).  The decisions are
discontinuous, and ``pose2 @ inv(pose1)`` or a sum evaluated by another library differs in the last
bits, so exact equality of integer boxes is a fair demand only where the margin is far above float64
rounding.  Every scene used anywhere has margin >= ``MIN_MARGIN``: ``checked_scene`` asserts it and
re-draws a scene that fails (no pair is ever left out of a comparison on this ground).
"""
import hashlib
import math

import numpy as np

MIN_MARGIN = 1e-9          # a thousand times float64 rounding at these magnitudes (|u2| < 1e4)
PARAM_DOUBLES = 40         # OETR_COVIS_PARAM_DOUBLES


def overlap_box(K1, depth1, pose1, bbox1, ratio1, K2, depth2, pose2, bbox2, ratio2, T=None):
    """-> dict(box1, box2 int64 [4], valid bool, count int, mask1, mask2 uint8 [H,W], margin float).
    ``depth1`` / ``depth2`` are used as float64.  ``T``: ``pose2 @ inv(pose1)`` when the caller has it.
    Inside test ``i < W, j < H`` (the reference's ``i < h, j < w`` for square maps)."""
    d1, d2 = np.asarray(depth1, np.float64), np.asarray(depth2, np.float64)
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    b1, r1, b2, r2 = (np.asarray(a, np.float64) for a in (bbox1, ratio1, bbox2, ratio2))
    H, W = d2.shape
    assert d1.shape == d2.shape
    if T is None:
        T = np.asarray(pose2, np.float64) @ np.linalg.inv(np.asarray(pose1, np.float64))
    v1, u1 = np.nonzero(d1 > 0)
    Z = d1[v1, u1]
    with np.errstate(all='ignore'):
        x = (u1 + b1[1] + 0.5) / r1[1]
        y = (v1 + b1[0] + 0.5) / r1[0]
        X = (x - K1[0, 2]) * (Z / K1[0, 0])
        Y = (y - K1[1, 2]) * (Z / K1[1, 1])
        q = [((T[r, 0] * X + T[r, 1] * Y) + T[r, 2] * Z) + T[r, 3] for r in range(4)]
        Xc, Yc, Zc = q[0] / q[3], q[1] / q[3], q[2] / q[3]
        a = [(K2[r, 0] * Xc + K2[r, 1] * Yc) + K2[r, 2] * Zc for r in range(3)]
        u2 = (a[0] / a[2]) * r2[1] - b2[1] - 0.5
        v2 = (a[1] / a[2]) * r2[0] - b2[0] - 0.5
        inside = (u2 > -1.0) & (u2 < W) & (v2 > -1.0) & (v2 < H)          # trunc() in range; False for NaN
        # every projection near the image takes part in the margin, inside or just outside
        near = np.isfinite(u2) & np.isfinite(v2) & (u2 > -2.0) & (u2 < W + 1.0) & (v2 > -2.0) & (v2 < H + 1.0)
    margin = np.inf
    if near.any():
        un, vn = u2[near], v2[near]
        margin = min(np.abs(un - np.round(un)).min(), np.abs(vn - np.round(vn)).min())
    i = np.trunc(u2[inside]).astype(np.int64)
    j = np.trunc(v2[inside]).astype(np.int64)
    dz = np.abs(Zc[inside] - d2[j, i])
    if dz.size:
        margin = min(margin, np.abs(dz - 0.5).min())
    inl = dz < 0.5
    uu, vv, ii, jj = u1[inside][inl], v1[inside][inl], i[inl], j[inl]
    count = int(inl.sum())
    mask1, mask2 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    box1 = box2 = np.zeros(4, np.int64)
    if count:
        box1 = np.array([uu.min(), vv.min(), uu.max(), vv.max()], np.int64)
        box2 = np.array([ii.min(), jj.min(), ii.max(), jj.max()], np.int64)
        mask1[vv, uu] = 1
        mask2[jj, ii] = 1
    return dict(box1=box1, box2=box2, valid=count > 0, count=count, mask1=mask1, mask2=mask2, margin=float(margin))


def param_block(scene):
    """The float64 [40] parameter block of a scene (layout: ``include/oetr_covis.h``), with numpy's ``T``."""
    p = np.zeros(PARAM_DOUBLES, np.float64)
    p[0:16] = (scene['pose2'] @ np.linalg.inv(scene['pose1'])).reshape(16)
    K1 = scene['intrinsics1']
    p[16:20] = K1[0, 0], K1[1, 1], K1[0, 2], K1[1, 2]
    p[20:29] = scene['intrinsics2'].reshape(9)
    p[29:31], p[31:33] = scene['bbox1'], scene['ratio1']
    p[33:35], p[35:37] = scene['bbox2'], scene['ratio2']
    return p


def scene_args(scene):
    """A scene as the reference's positional arguments (float64 depth maps)."""
    return tuple(np.asarray(scene[k + s], np.float64) for s in ('1', '2')
                 for k in ('intrinsics', 'depth', 'pose', 'bbox', 'ratio'))


def restate(scene):
    return overlap_box(*scene_args(scene))


# ------------------------------------------------------------------ synthetic scenes
# Scenes are drawn with elementwise float64 arithmetic, libm's scalar sin / cos / sqrt and numpy's seeded
# generator only - no BLAS, no vectorised transcendental - so a (kind, size, seed) recipe gives the same bytes on
# every machine, and tests/covis_expected.json can pin them by hash.
def _matmul3(A, B):
    return np.array([[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)])


def _matvec3(A, x):
    return np.array([(A[i][0] * x[0] + A[i][1] * x[1]) + A[i][2] * x[2] for i in range(3)])


def _rot(axis, angle):
    c, s = math.cos(float(angle)), math.sin(float(angle))
    R = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R[i, i] = R[j, j] = c
    R[i, j], R[j, i] = -s, s
    return R


def _pose(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


def render_plane(K, P, h, w, normal, d, bbox, ratio):
    """Depth of the world plane ``normal . X = d`` in camera ``P`` (world to camera) at the pixel centres
    the reference assumes (``x = (u + bbox[1] + 0.5) / ratio[1]``); 0 where the ray misses it."""
    R, t = P[:3, :3], P[:3, 3]
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = (u + bbox[1] + 0.5) / ratio[1], (v + bbox[0] + 0.5) / ratio[0]
    rx, ry = (x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1]         # the ray (rx, ry, 1)
    nr = _matvec3(R, normal)
    with np.errstate(all='ignore'):
        z = (d + ((nr[0] * t[0] + nr[1] * t[1]) + nr[2] * t[2])) / ((rx * nr[0] + ry * nr[1]) + nr[2])
    z[~np.isfinite(z) | (z <= 0)] = 0
    return z


KINDS = ('plane', 'no_overlap', 'behind', 'trunc')


def make_scene(kind, h, w, seed):
    """One pair: a tilted world plane seen by two cameras with differing intrinsics, crop offsets and
    ratios; holes in both depth maps and a region of depth map 2 pushed back by 3 (an occluder's
    shadow: rejected inliers).  ``kind``:
      'plane'       the two views overlap;
      'no_overlap'  camera 2 sees another part of the plane: no inlier, valid = False;
      'behind'      camera 2 looks away: every point is behind it;
      'trunc'       camera 2 is camera 1 moved by a fraction of a pixel: landings with -1 < u2 < 0 and
                    -1 < v2 < 0 at the left and top edges, which truncation puts on column / row 0."""
    rng = np.random.default_rng(seed)
    s = min(h, w) / 640.0
    K1 = np.array([[700.0 * s, 0, 0.62 * w], [0, 700.0 * s, 0.47 * h], [0, 0, 1]])
    K2 = np.array([[650.0 * s, 0, 0.59 * w], [0, 660.0 * s, 0.49 * h], [0, 0, 1]])
    normal = np.array([0.1, 0.05, 1.0]) + 0.05 * rng.standard_normal(3)
    normal = normal / math.sqrt(float((normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2]))
    d = 10.0 + rng.uniform(-1, 1)
    b1, r1 = np.array([12.0, 40.0]) * s, np.array([0.9, 0.9])
    b2, r2 = np.array([30.0, 5.0]) * s, np.array([1.1, 1.1])
    P1 = _pose(_rot(1, 0.05 + 0.02 * rng.standard_normal()), [0.1, 0.0, 0.0])
    if kind == 'plane':
        P2 = _pose(_matmul3(_rot(1, -0.35 + 0.05 * rng.standard_normal()), _rot(0, 0.1)),
                   np.array([2.5, 0.3, 1.0]) + 0.1 * rng.standard_normal(3))
    elif kind == 'no_overlap':
        P2 = _pose(_rot(1, 0.05), [-60.0, 0.0, 0.0])          # 60 units to the side: another part of the plane
    elif kind == 'behind':
        P2 = _pose(_rot(1, math.pi - 0.1), [0.0, 0.0, 1.0])
    elif kind == 'trunc':
        K2, b2, r2 = K1.copy(), b1.copy(), r1.copy()
        K2[0, 2] -= 0.3 / r1[1]
        K2[1, 2] -= 0.4 / r1[0]
        P2 = P1.copy()
    else:
        raise ValueError(kind)
    d1 = render_plane(K1, P1, h, w, normal, d, b1, r1)
    d2 = render_plane(K2, P2, h, w, normal, d, b2, r2)
    d1[rng.random(d1.shape) < 0.2] = 0                          # holes, 80 % coverage
    d2[int(0.31 * h):int(0.47 * h), int(0.16 * w):int(0.55 * w)] = 0
    d2[int(0.62 * h):, int(0.78 * w):] += 3.0                   # pushed back: depth test fails there
    return dict(depth1=d1.astype(np.float32), intrinsics1=K1, pose1=P1, bbox1=b1, ratio1=r1,
                depth2=d2.astype(np.float32), intrinsics2=K2, pose2=P2, bbox2=b2, ratio2=r2)


def checked_scene(kind, h, w, seed):
    """``make_scene`` re-drawn (seed + 1000, ...) until its decision margin is >= MIN_MARGIN, and its
    restatement.  -> (scene, result of ``overlap_box``)."""
    for attempt in range(20):
        scene = make_scene(kind, h, w, seed + 1000 * attempt)
        res = restate(scene)
        if res['margin'] >= MIN_MARGIN:
            return scene, res
    raise AssertionError(f'no {kind} scene of {h}x{w} with margin >= {MIN_MARGIN} in 20 draws from seed {seed}')


def scene_batch(kinds, h, w, seed):
    """A batch of checked scenes -> (dict of stacked arrays under the dataset's names, list of results)."""
    drawn = [checked_scene(k, h, w, seed + 17 * n) for n, k in enumerate(kinds)]
    batch = {key: np.stack([sc[key] for sc, _ in drawn]) for key in drawn[0][0]}
    return batch, [res for _, res in drawn]


# ------------------------------------------------------------------ pinned scenes (tests/covis_expected.json)
def sha(a):
    """sha256 of an array's bytes (C order)."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def result_record(res):
    """A result of ``overlap_box`` as JSON-able recorded values (masks by hash and sum)."""
    return dict(box1=[int(x) for x in res['box1']], box2=[int(x) for x in res['box2']], valid=bool(res['valid']),
                count=int(res['count']), mask1_sha256=sha(res['mask1']), mask2_sha256=sha(res['mask2']),
                mask2_sum=int(res['mask2'].sum()))


# ------------------------------------------------------------------ the evaluator's box table
def recall_table():
    """-> (gt, pred) float32 [2, 24, 4]: ground-truth and predicted boxes of 24 pairs, integers and multiples of
    0.37 from a seeded integer generator; pairs 0-3 predicted exactly, pair 4 with IoUs exactly 0.5 and 0.75,
    pairs 5-7 with a zero ground-truth box (no co-visible pixel)."""
    rng = np.random.default_rng(11)
    n = 24
    xy = rng.integers(0, 200, (2, n, 2)).astype(np.float32)
    wh = rng.integers(40, 300, (2, n, 2)).astype(np.float32)
    gt = np.concatenate([xy, xy + wh], axis=2)
    pred = gt + rng.integers(-60, 60, (2, n, 4)).astype(np.float32) * np.float32(0.37)
    pred[:, :4] = gt[:, :4]
    gt[0, 4], pred[0, 4] = (0, 0, 100, 100), (0, 0, 100, 50)
    gt[1, 4], pred[1, 4] = (0, 0, 100, 100), (0, 0, 75, 100)
    gt[:, 5:8] = 0
    return gt, pred


def box_scores(gt, pred, oiou=False, eps=1e-6):
    """float32 [2n]: aligned IoU (or overlap over the ground-truth box's area) of every box, image 1's then image 2's."""
    gt, pred = gt.reshape(-1, 4).astype(np.float32), pred.reshape(-1, 4).astype(np.float32)
    wh = np.clip(np.minimum(gt[:, 2:], pred[:, 2:]) - np.maximum(gt[:, :2], pred[:, :2]), 0, None)
    overlap = wh[:, 0] * wh[:, 1]
    area_gt = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    with np.errstate(all='ignore'):
        if oiou:
            return overlap / area_gt
        area_pred = (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1])
        return overlap / np.maximum(area_gt + area_pred - overlap, np.float32(eps))


def recalls(scores, thrs):
    """Share of scores >= each threshold, compared in float64 as numpy compares a float32 array with a float64
    threshold (NaN fails every threshold)."""
    scores, thrs = np.asarray(scores, np.float64), np.asarray(thrs, np.float64)
    with np.errstate(all='ignore'):
        return np.array([(scores >= t).sum() / float(scores.shape[0]) for t in thrs])
