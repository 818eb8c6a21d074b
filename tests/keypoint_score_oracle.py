"""Keypoint repeatability against depth and pose, as a float64 numpy program: the SPECIFICATION of what
the reference's ``pose_evaluate`` computes with ``get_projected_kp`` / ``unnormalize_keypoints`` / ``get_repeatability``
(``dloc/evaluate/utils/evaluation.py:135-179``, ``utils.py:214-236``) for one pair of pictures and their two keypoint
SETS, written with elementwise numpy operations only (every product and sum is one IEEE float64 operation, in the order
written here), and the synthetic keypoint sets its tests and the generator of the pinned sets
(``tools/gen_golden_keypoint_score.py``) share.

``direction`` projects the keypoints of one picture into the other and finds, for every keypoint that is kept, the
nearest keypoint of the other picture; ``score`` is both directions of a pair; ``repeatability`` the reference's summary
of the counters; ``margins`` measures how far a set is from every decision a last-bit difference could flip.  The scenes,
the depth look-up and the parameter blocks are those of ``match_score_oracle``.
"""
import numpy as np

import covis_oracle as cvo
import match_score_oracle as mso

MAX_THRESHOLDS = 8
THRESHOLDS = (1.0, 2.0, 3.0, 5.0)
MIN_THRESHOLD_MARGIN = mso.MIN_THRESHOLD_MARGIN      # relative distance of every dist_sq from every th * th
MIN_TIE_MARGIN = mso.MIN_TIE_MARGIN


def project(depth_src, P, kp_src, reverse=False):
    """The keypoints of the source picture in the other picture -> ``(d, pu, pv)`` float64 ``[n]``.  ``reverse=False``
    is direction 1 -> 2 (the expressions of ``match_score_oracle.score`` lines 53 and 68-72), ``reverse=True`` direction
    2 -> 1 (lines 74-81: ``R^T`` and ``R^T t``, recomputed with the same operations)."""
    P = np.asarray(P, np.float64)
    k = np.asarray(kp_src, np.float64).reshape(-1, 2)
    u, v = k[:, 0], k[:, 1]
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = P[:8]
    (R00, R01, R02), (R10, R11, R12), (R20, R21, R22) = P[8:17].reshape(3, 3)
    t0, t1, t2 = P[17:20]
    with np.errstate(all='ignore'):
        d = mso.depth_at(depth_src, u, v)
        if not reverse:
            x1, y1 = (u - cx1) / fx1, (v - cy1) / fy1
            X1, Y1 = x1 * d, y1 * d
            p0 = ((R00 * X1 + R01 * Y1) + R02 * d) + t0
            p1 = ((R10 * X1 + R11 * Y1) + R12 * d) + t1
            p2 = ((R20 * X1 + R21 * Y1) + R22 * d) + t2
            pu, pv = fx2 * (p0 / p2) + cx2, fy2 * (p1 / p2) + cy2
        else:
            x2, y2 = (u - cx2) / fx2, (v - cy2) / fy2
            m0 = (R00 * t0 + R10 * t1) + R20 * t2
            m1 = (R01 * t0 + R11 * t1) + R21 * t2
            m2 = (R02 * t0 + R12 * t1) + R22 * t2
            X2, Y2 = x2 * d, y2 * d
            q0 = ((R00 * X2 + R10 * Y2) + R20 * d) - m0
            q1 = ((R01 * X2 + R11 * Y2) + R21 * d) - m1
            q2 = ((R02 * X2 + R12 * Y2) + R22 * d) - m2
            pu, pv = fx1 * (q0 / q2) + cx1, fy1 * (q1 / q2) + cy1
    return d, pu, pv


def nearest_neighbour(pu, pv, kp_dst):
    """For every projected point the nearest target keypoint -> ``(nearest int32 [n], dist_sq float64 [n])``.  It is the
    loop ``best = +inf, nearest = -1; for b ascending: d = (pu - u[b]) * (pu - u[b]) + (pv - v[b]) * (pv - v[b]);
    if d < best: best, nearest = d, b`` - the lowest index wins a tie, a NaN distance never wins, and neither does an
    infinite one - written over the whole ``n x m`` table: NaN entries are replaced by ``+inf`` and the first minimum
    taken."""
    k = np.asarray(kp_dst, np.float64).reshape(-1, 2)
    n = len(pu)
    if len(k) == 0:
        return np.full(n, -1, np.int32), np.full(n, np.inf)
    with np.errstate(all='ignore'):
        du, dv = pu[:, None] - k[None, :, 0], pv[:, None] - k[None, :, 1]
        D = du * du + dv * dv
    D[np.isnan(D)] = np.inf
    best = D.min(1)
    nearest = np.where(best < np.inf, D.argmin(1), -1).astype(np.int32)
    return nearest, best


def direction(depth_src, shape_dst, P, kp_src, kp_dst, thresholds=THRESHOLDS, reverse=False):
    """One direction of one pair -> dict(d, pu, pv, kept bool [n], nearest int32 [n], dist_sq float64 [n], counts int32
    [2 + T]: keypoints, kept, and per threshold the kept rows with ``dist_sq < th * th``).  Rows that are not kept hold
    ``nearest = -1``, ``dist_sq = NaN``."""
    assert len(thresholds) <= MAX_THRESHOLDS
    H, W = shape_dst
    d, pu, pv = project(depth_src, P, kp_src, reverse)
    with np.errstate(all='ignore'):
        kept = (d != 0.0) & (pu < float(W)) & (pv < float(H))          # the reference's test: no lower bound
    nearest = np.full(len(pu), -1, np.int32)
    dist_sq = np.full(len(pu), np.nan)
    nearest[kept], dist_sq[kept] = nearest_neighbour(pu[kept], pv[kept], kp_dst)
    counts = [len(pu), int(kept.sum())]
    for th in thresholds:
        th = np.float64(th)
        with np.errstate(all='ignore'):
            counts.append(int((dist_sq[kept] < th * th).sum()))
    return dict(d=d, pu=pu, pv=pv, kept=kept, nearest=nearest, dist_sq=dist_sq, counts=np.array(counts, np.int32))


def score(depth1, depth2, P, kp1, kp2, thresholds=THRESHOLDS):
    """Both directions of one pair -> ``(dir12, dir21)``, each a :func:`direction` dict."""
    return (direction(depth1, depth2.shape, P, kp1, kp2, thresholds, False),
            direction(depth2, depth1.shape, P, kp2, kp1, thresholds, True))


def repeatability(counts):
    """``counts`` int ``[..., 2, 2 + T]`` -> float64 ``[..., T]``: ``(c12 / kept12 + c21 / kept21) / 2``, a direction
    that kept nothing contributing 0 (``utils.py:215-216``)."""
    c = np.asarray(counts, np.int64)
    kept = c[..., 1:2]
    share = np.where(kept > 0, c[..., 2:] / np.maximum(kept, 1), 0.0)
    return (share[..., 0, :] + share[..., 1, :]) / 2


def margins(res, kp_src, thresholds=THRESHOLDS):
    """-> (threshold margin, tie margin) of one direction: the smallest relative distance of a finite ``dist_sq`` of a
    kept row from a ``th * th``, and the smallest distance of a depth-look-up coordinate from a ``.5`` tie among the
    coordinates that are not exactly on one."""
    v = res['dist_sq'][res['kept']]
    v = v[np.isfinite(v)]
    thr = np.inf
    for th in thresholds:
        if v.size:
            thr = min(thr, float(np.abs(v - th * th).min() / (th * th)))
    c = np.asarray(kp_src, np.float64).reshape(-1)
    c = c[np.isfinite(c)]
    dist = np.abs((c - np.floor(c)) - 0.5)
    dist = dist[dist != 0.0]
    return thr, float(dist.min()) if dist.size else np.inf


# ------------------------------------------------------------------ synthetic keypoint sets
# The four views of match_score_oracle.make_scene; every ordered pair and the self pairs.
PAIRS = tuple((i, j) for i in range(4) for j in range(4))
# keypoints per view of the pinned sets: every count straddles a wave (64) or a query / target tile (256) somewhere
COUNTS = ((1, 63, 600, 257), (0, 64, 256, 65), (65, 255, 257, 600))
SOURCE_VIEW = 2                      # the true points are pixels of this view (40 x 64)
SPECIAL_FROM = 63                    # views with at least this many keypoints end in the 16 special rows


def _warp(views, k, c, r, z):
    """Pixels ``(c, r)`` with depth ``z`` of view SOURCE_VIEW seen in view ``k`` -> float64 ``[n,2]`` (clipped)."""
    P = mso.pair_block(views, SOURCE_VIEW, k)
    x, y = (c - P[2]) / P[0] * z, (r - P[3]) / P[1] * z
    R, t = P[8:17].reshape(3, 3), P[17:20]
    q = [(R[a][0] * x + R[a][1] * y) + R[a][2] * z + t[a] for a in range(3)]
    with np.errstate(all='ignore'):
        far = np.stack([P[4] * (q[0] / q[2]) + P[6], P[5] * (q[1] / q[2]) + P[7]], 1)
    far[~np.isfinite(far)] = 0.0
    return np.clip(far, -1e4, 1e4)


def make_keypoints(views, counts, seed, noise=0.4):
    """One float32 ``[n_k, 2]`` keypoint set per view.  Half of a set (rounded up) are TRUE points - 600 pixels of view
    SOURCE_VIEW, un-projected with its depth (holes take a stand-in depth) and seen in every view, with Gaussian noise of
    ``noise`` px: the same world points in every picture, so that keypoints repeat -, the rest uniformly random in (and a
    little outside of) the picture.  Sets of at least SPECIAL_FROM keypoints have three duplicated rows (10 = 3,
    40 = 41 = 7) and end in ``match_score_oracle.special_points`` (``.5`` ties, the picture's edges, +-inf, NaN)."""
    rng = np.random.default_rng(seed)
    hs, ws = views[SOURCE_VIEW]['depth'].shape
    n_true = 600
    c, r = rng.integers(0, ws, n_true), rng.integers(0, hs, n_true)
    z = views[SOURCE_VIEW]['depth'][r, c].astype(np.float64)
    z = np.where(z > 0, z, 9.0 + rng.random(n_true))
    sets = []
    for k, n in enumerate(counts):
        h, w = views[k]['depth'].shape
        true = _warp(views, k, c, r, z) + noise * rng.standard_normal((n_true, 2))
        pick = rng.permutation(n_true)[:(n + 1) // 2]
        anywhere = np.stack([rng.uniform(-2, w + 2, n), rng.uniform(-2, h + 2, n)], 1)
        kp = np.concatenate([true[pick], anywhere])[:n]
        kp = mso.off_tie(kp[rng.permutation(n)] if n else kp.reshape(0, 2))
        if n >= SPECIAL_FROM:
            kp[10], kp[40], kp[41] = kp[3], kp[7], kp[7]
            kp[n - 16:] = mso.special_points((h, w))
        sets.append(np.ascontiguousarray(kp, np.float32).reshape(-1, 2))
    return sets


def score_pairs(views, kps, pairs=PAIRS, thresholds=THRESHOLDS, blocks=None):
    """``score`` of every pair of one set; ``blocks``: the parameter blocks to use (default: ``pair_block``)."""
    return [score(views[i]['depth'], views[j]['depth'], mso.pair_block(views, i, j) if blocks is None else blocks[p],
                  kps[i], kps[j], thresholds) for p, (i, j) in enumerate(pairs)]


def set_margins(results, kps, pairs=PAIRS, thresholds=THRESHOLDS):
    thr = tie = np.inf
    for (i, j), (a, b) in zip(pairs, results):
        for res, kp in ((a, kps[i]), (b, kps[j])):
            x, y = margins(res, kp, thresholds)
            thr, tie = min(thr, x), min(tie, y)
    return thr, tie


def draw_set(views, counts, seed, thresholds=THRESHOLDS):
    """The keypoint sets of ``counts``, re-drawn (seed + 1000, + 2000, ...) until both margins hold -> (kps, the seed
    that was used, results, (threshold margin, tie margin)).  No row is excluded."""
    while True:
        kps = make_keypoints(views, counts, seed)
        results = score_pairs(views, kps, thresholds=thresholds)
        thr, tie = set_margins(results, kps, thresholds=thresholds)
        if thr >= MIN_THRESHOLD_MARGIN and tie >= MIN_TIE_MARGIN:
            return kps, seed, results, (thr, tie)
        seed += 1000


def pair_record(res):
    """One scored pair as JSON-able recorded values: the counters, and ``nearest`` / ``dist_sq`` by hash."""
    a, b = res
    return dict(counts=[[int(c) for c in a['counts']], [int(c) for c in b['counts']]],
                nearest_sha256=[cvo.sha(a['nearest']), cvo.sha(b['nearest'])],
                dist_sq_sha256=[cvo.sha(np.where(np.isnan(a['dist_sq']), np.nan, a['dist_sq'])),
                                cvo.sha(np.where(np.isnan(b['dist_sq']), np.nan, b['dist_sq']))])


def padded(results, max_kp):
    """The results of a pair list as the device lays them out -> (counts int32 [P,2,2+T], nearest int32 [P,2,max_kp],
    dist_sq float64 [P,2,max_kp]); rows past a picture's count hold -1 / NaN."""
    P = len(results)
    T = len(results[0][0]['counts']) - 2 if P else 0
    counts = np.zeros((P, 2, 2 + T), np.int32)
    nearest = np.full((P, 2, max_kp), -1, np.int32)
    dist_sq = np.full((P, 2, max_kp), np.nan)
    for p, pair in enumerate(results):
        for s, res in enumerate(pair):
            n = len(res['nearest'])
            counts[p, s], nearest[p, s, :n], dist_sq[p, s, :n] = res['counts'], res['nearest'], res['dist_sq']
    return counts, nearest, dist_sq


# ------------------------------------------------------------------ the reference's own functions
def reference_direction(ref, depth_src, shape_dst, P, kp_src, kp_dst, thresholds=THRESHOLDS, reverse=False):
    """``pose_evaluate``'s repeatability of one direction with the reference's own ``normalize_keypoints``,
    ``get_projected_kp``, ``unnormalize_keypoints`` and ``get_repeatability`` (``evaluation.py:135-177``) -> dict(kept
    bool [n], dist_sq float64 [kept rows] (its ``cdist`` + ``amin``), shares: what ``get_repeatability`` returns).  The
    target keypoints with a non-finite coordinate are REMOVED first (the specification's departure: the reference's
    ``amin`` would return NaN for every row); with no target left ``dist_sq`` and ``shares`` are None (it raises)."""
    utils, _ = ref
    P = np.asarray(P, np.float64)
    K1 = np.array([[P[0], 0, P[2]], [0, P[1], P[3]], [0, 0, 1]])
    K2 = np.array([[P[4], 0, P[6]], [0, P[5], P[7]], [0, 0, 1]])
    dR, dT = P[8:17].reshape(3, 3), P[17:20].reshape(3, 1)
    src = np.asarray(kp_src, np.float64).reshape(-1, 2)
    dst = np.asarray(kp_dst, np.float64).reshape(-1, 2)
    dst = dst[np.isfinite(dst).all(1)]
    n = len(src)
    with np.errstate(all='ignore'):
        at = np.round(src).astype(int)
        ok = (at[:, 0] >= 0) & (at[:, 0] < depth_src.shape[1]) & (at[:, 1] >= 0) & (at[:, 1] < depth_src.shape[0])
        d = np.zeros((n, 1))
        d[ok, 0] = depth_src[at[ok, 1], at[ok, 0]]
        one = np.zeros((1, 2))                                    # the other side of get_projected_kp: not used
        if not reverse:
            proj, _ = utils.get_projected_kp(utils.normalize_keypoints(src, K1), one, d, np.ones((1, 1)), dR, dT)
            proj = utils.unnormalize_keypoints(np.reshape(proj, (n, 2)), K2)
        else:
            _, proj = utils.get_projected_kp(one, utils.normalize_keypoints(src, K2), np.ones((1, 1)), d, dR, dT)
            proj = utils.unnormalize_keypoints(np.reshape(proj, (n, 2)), K1)
        nonzero = np.nonzero(d[:, 0])
        inside = np.where((proj[:, 0] < shape_dst[1]) & (proj[:, 1] < shape_dst[0]))
        rows = np.intersect1d(inside, nonzero)
        kept = np.zeros(n, bool)
        kept[rows] = True
        if len(dst) == 0 and len(rows):
            return dict(kept=kept, dist_sq=None, shares=None)
        shares = utils.get_repeatability(proj[rows], dst, list(thresholds))
        dist_sq = utils.distance.cdist(proj[rows], dst, metric='sqeuclidean').min(1) if len(rows) else np.zeros(0)
    return dict(kept=kept, dist_sq=dist_sq, shares=[float(s) for s in shares])


def compare_with_reference(mine, theirs):
    """One direction of the specification against :func:`reference_direction` -> (the largest relative difference of
    the minima, the largest absolute difference of their square roots, in pixels); zeros where the reference has no
    minima.  Asserts that the kept rows and every counter are identical."""
    assert np.array_equal(mine['kept'], theirs['kept']), 'kept rows'
    if theirs['shares'] is None:
        return 0.0, 0.0
    kept = int(mine['counts'][1])
    want = [int(c) / kept if kept else 0 for c in mine['counts'][2:]]
    assert theirs['shares'] == want, (theirs['shares'], want)
    a, b = theirs['dist_sq'], mine['dist_sq'][mine['kept']]
    both = np.isfinite(a) & np.isfinite(b)
    px = float(np.abs(np.sqrt(a[both]) - np.sqrt(b[both])).max()) if both.any() else 0.0
    return mso.rel_diff(a, b), px


def reference_diffs(ref, views, kps, results, pairs=PAIRS, thresholds=THRESHOLDS):
    """One set against the reference -> (the largest relative difference of the minima over the pairs ``i != j``, the
    largest absolute difference of the distances in pixels over the SELF pairs).  A self pair's minima are what
    rounding leaves of the distance between a keypoint and its own re-projection - 0, or some 1e-29 - so that a
    relative measure of them says nothing; their square roots are compared absolutely instead.  Kept rows and counters
    are asserted identical for every pair."""
    rel = px = 0.0
    for (i, j), (a, b) in zip(pairs, results):
        P = mso.pair_block(views, i, j)
        d1, d2 = views[i]['depth'], views[j]['depth']
        for mine, theirs in ((a, reference_direction(ref, d1, d2.shape, P, kps[i], kps[j], thresholds, False)),
                             (b, reference_direction(ref, d2, d1.shape, P, kps[j], kps[i], thresholds, True))):
            r, x = compare_with_reference(mine, theirs)
            if i == j:
                px = max(px, x)
            else:
                rel = max(rel, r)
    return rel, px
