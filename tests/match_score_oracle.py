"""Scoring matches against depth and pose, as a float64 numpy program: the SPECIFICATION of the
reference's ``compute_epipolar_error`` / ``get_episym`` / ``get_projected_kp`` + ``get_truesym`` for one pair's match
list, written with elementwise numpy operations only (no ``@``, no BLAS: every product and sum is one IEEE float64
operation, in the order written here), and the synthetic scenes and match lists its tests and the generator of the
pinned lists (``tools/gen_golden_match_score.py``) share.

``score`` is one pair's list; ``margins`` measures how far a list is from every decision that a last-bit difference
could flip (a threshold, a ``.5`` rounding tie); ``make_scene`` / ``make_matches`` draw depth maps of one tilted world
plane under cameras with real relative motion and matches made by warping true points, with controlled noise and
outliers; ``load_reference`` / ``reference_scores`` run the reference's own functions from the snapshot.
"""
import numpy as np

import covis_oracle as cvo

PARAM_DOUBLES = 20
FLAG_DEPTH1, FLAG_DEPTH2, FLAG_EPI, FLAG_EPISYM, FLAG_REPROJ = 1, 2, 4, 8, 16
VALUES = ('epi_ref', 'episym', 'reproj12_sq', 'reproj21_sq')
MIN_THRESHOLD_MARGIN = 1e-6      # relative distance of every thresholded quantity from its threshold
MIN_TIE_MARGIN = 1e-3            # distance of every depth-test coordinate from a .5 tie, unless it is exactly on one


def param_block(K1, K2, T):
    """The 20 doubles of one pair: fx fy cx cy of camera 1, of camera 2, R (row major), t of ``T_1to2``."""
    K1, K2, T = (np.asarray(a, np.float64) for a in (K1, K2, T))
    return np.concatenate([[K1[0, 0], K1[1, 1], K1[0, 2], K1[1, 2], K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2]],
                           T[:3, :3].reshape(9), T[:3, 3]])


def depth_at(depth, u, v):
    """Depth at ``(rint(v), rint(u))`` (half to even), 0 outside the map; the range test is made in float64."""
    H, W = depth.shape
    with np.errstate(all='ignore'):
        c, r = np.rint(u), np.rint(v)
        inside = (c >= 0.0) & (c < float(W)) & (r >= 0.0) & (r < float(H))
    d = np.zeros(u.shape, np.float64)
    d[inside] = depth[r[inside].astype(np.int64), c[inside].astype(np.int64)].astype(np.float64)
    return d


def score(depth1, depth2, P, k1, k2, epi_thr=5e-4, sym_thr=None, px_thr=None):
    """One pair's list.  ``k1`` / ``k2``: ``[m,2]`` original-picture coordinates (any float dtype; used as float64).
    -> dict(epi_ref, episym, reproj12_sq, reproj21_sq float64 [m], flags uint8 [m], counts int32 [5], d1, d2, z12)."""
    P = np.asarray(P, np.float64)
    k1, k2 = np.asarray(k1, np.float64).reshape(-1, 2), np.asarray(k2, np.float64).reshape(-1, 2)
    u1, v1, u2, v2 = k1[:, 0], k1[:, 1], k2[:, 0], k2[:, 1]
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = P[:8]
    (R00, R01, R02), (R10, R11, R12), (R20, R21, R22) = P[8:17].reshape(3, 3)
    t0, t1, t2 = P[17:20]
    nan = np.float64('nan')
    thr = [nan if t is None else np.float64(t) for t in (epi_thr, sym_thr, px_thr)]
    with np.errstate(all='ignore'):
        x1, y1 = (u1 - cx1) / fx1, (v1 - cy1) / fy1
        x2, y2 = (u2 - cx2) / fx2, (v2 - cy2) / fy2
        E00, E01, E02 = t1 * R20 - t2 * R10, t1 * R21 - t2 * R11, t1 * R22 - t2 * R12
        E10, E11, E12 = t2 * R00 - t0 * R20, t2 * R01 - t0 * R21, t2 * R02 - t0 * R22
        E20, E21, E22 = t0 * R10 - t1 * R00, t0 * R11 - t1 * R01, t0 * R12 - t1 * R02
        a0 = (E00 * x1 + E01 * y1) + E02
        a1 = (E10 * x1 + E11 * y1) + E12
        a2 = (E20 * x1 + E21 * y1) + E22
        b0 = (E00 * x2 + E10 * y2) + E20
        b1 = (E01 * x2 + E11 * y2) + E21
        s = (x2 * a0 + y2 * a1) + a2
        s2 = s * s
        epi = s2 * (1.0 / (a0 + a1) + 1.0 / (b0 + b1))
        sym = s2 * (1.0 / (a0 * a0 + a1 * a1) + 1.0 / (b0 * b0 + b1 * b1))
        d1, d2 = depth_at(depth1, u1, v1), depth_at(depth2, u2, v2)
        X1, Y1 = x1 * d1, y1 * d1
        p0 = ((R00 * X1 + R01 * Y1) + R02 * d1) + t0
        p1 = ((R10 * X1 + R11 * Y1) + R12 * d1) + t1
        p2 = ((R20 * X1 + R21 * Y1) + R22 * d1) + t2
        e0, e1 = (fx2 * (p0 / p2) + cx2) - u2, (fy2 * (p1 / p2) + cy2) - v2
        r12 = e0 * e0 + e1 * e1
        m0 = (R00 * t0 + R10 * t1) + R20 * t2
        m1 = (R01 * t0 + R11 * t1) + R21 * t2
        m2 = (R02 * t0 + R12 * t1) + R22 * t2
        X2, Y2 = x2 * d2, y2 * d2
        q0 = ((R00 * X2 + R10 * Y2) + R20 * d2) - m0
        q1 = ((R01 * X2 + R11 * Y2) + R21 * d2) - m1
        q2 = ((R02 * X2 + R12 * Y2) + R22 * d2) - m2
        g0, g1 = (fx1 * (q0 / q2) + cx1) - u1, (fy1 * (q1 / q2) + cy1) - v1
        r21 = g0 * g0 + g1 * g1
        has1, has2 = d1 != 0.0, d2 != 0.0
        both = has1 & has2
        ok_epi, ok_sym = epi < thr[0], sym < thr[1]
        ok_px = both & (r21 < thr[2] * thr[2])
    flags = (has1 * FLAG_DEPTH1 + has2 * FLAG_DEPTH2 + ok_epi * FLAG_EPI + ok_sym * FLAG_EPISYM
             + ok_px * FLAG_REPROJ).astype(np.uint8)
    off = lambda n, t: -1 if np.isnan(t) else int(n)
    counts = np.array([len(u1), off(ok_epi.sum(), thr[0]), off(ok_sym.sum(), thr[1]), int(both.sum()),
                       off(ok_px.sum(), thr[2])], np.int32)
    return dict(epi_ref=epi, episym=sym, reproj12_sq=r12, reproj21_sq=r21, flags=flags, counts=counts, d1=d1, d2=d2,
                z12=p2, z21=q2)


def margins(res, k1, k2, epi_thr=5e-4, sym_thr=None, px_thr=None):
    """-> (threshold margin, tie margin) of one scored list: the smallest relative distance of a thresholded quantity
    from its threshold (NaN and infinite values decide the same way whatever the last bit: skipped), and the smallest
    distance of a depth-test coordinate from a ``.5`` tie among the coordinates that are not exactly on one."""
    thr_margin = np.inf
    both = (res['flags'] & 3) == 3
    for v, t in ((res['epi_ref'], epi_thr), (res['episym'], sym_thr),
                 (res['reproj21_sq'][both], None if px_thr is None else px_thr * px_thr)):
        v = v[np.isfinite(v)]
        if t is not None and v.size:
            thr_margin = min(thr_margin, float(np.abs(v - t).min() / t))
    c = np.concatenate([np.asarray(k1, np.float64).reshape(-1), np.asarray(k2, np.float64).reshape(-1)])
    c = c[np.isfinite(c)]
    dist = np.abs((c - np.floor(c)) - 0.5)
    dist = dist[dist != 0.0]
    return thr_margin, float(dist.min()) if dist.size else np.inf


def equal_bits(a, b):
    """NaN-aware bit comparison of two arrays of one dtype: NaN equals NaN (whatever sign and payload the two
    machines give their NaNs), everything else is compared bit for bit (-0 is not +0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((np.isnan(a) & np.isnan(b)) | (a.view(bits) == b.view(bits))).all())


def rel_diff(a, b):
    """Largest relative difference of two float64 arrays; equal entries (inf, and NaN with NaN, too) count 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all='ignore'):
        d = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
    d[same] = 0.0
    assert not np.isnan(d).any(), 'one side is NaN or infinite where the other is not'
    return float(d.max()) if d.size else 0.0


# ------------------------------------------------------------------ synthetic scenes and match lists
# Drawn like covis_oracle's scenes: elementwise float64 arithmetic, libm's scalar functions and numpy's seeded
# generator only, so a recipe gives the same bytes on every machine.
SIZES = ((1, 1), (7, 5), (40, 64), (56, 56))       # (H, W)
BEHIND_VIEW = 3                                     # turned round: what the others see lies behind it (z <= 0)


def rigid_inverse(P):
    """inverse of a rigid ``[R | t]``: ``[R^T | -R^T t]``, elementwise."""
    R, t = P[:3, :3], P[:3, 3]
    Q = np.eye(4)
    Q[:3, :3] = R.T
    Q[:3, 3] = -cvo._matvec3(R.T, t)
    return Q


def relative_pose(pose1, pose2):
    """``T_1to2 = pose2 . inverse(pose1)`` in a fixed summation order."""
    A, B = np.asarray(pose2, np.float64), rigid_inverse(np.asarray(pose1, np.float64))
    return np.array([[((A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]) + A[i][3] * B[3][j]
                      for j in range(4)] for i in range(4)])


def make_scene(sizes=SIZES, seed=0, behind=BEHIND_VIEW):
    """One view per entry of ``sizes`` of one tilted world plane: float32 depth map (the plane's depth along the ray
    through each INTEGER pixel coordinate, the frame keypoints live in; 20 % holes), intrinsics and a world-to-camera
    pose with real relative motion.  View ``behind`` (where the scene has that many) is turned round by 2.9 rad."""
    rng = np.random.default_rng(seed)
    normal = np.array([0.1, 0.05, 1.0]) + 0.05 * rng.standard_normal(3)
    normal = normal / np.sqrt((normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2])
    d = 10.0 + rng.uniform(-1, 1)
    views = []
    for m, (h, w) in enumerate(sizes):
        f = (0.9 + 0.3 * rng.uniform()) * max(h, w, 8)
        K = np.array([[f, 0, (0.45 + 0.1 * rng.uniform()) * w], [0, f * 1.02, (0.45 + 0.1 * rng.uniform()) * h], [0, 0, 1]])
        R = cvo._matmul3(cvo._rot(1, 0.1 * rng.standard_normal() + (2.9 if m == behind else 0.0)),
                         cvo._rot(0, 0.06 * rng.standard_normal()))
        t = np.array([0.8, 0.5, 0.3]) * rng.standard_normal(3)
        P = cvo._pose(R, t)
        depth = cvo.render_plane(K, P, h, w, normal, d, (-0.5, -0.5), (1.0, 1.0))
        if m == behind:                                           # it faces away from the plane: a depth of its own
            depth = 8.0 + 4.0 * rng.random(depth.shape)
        depth[rng.random(depth.shape) < 0.2] = 0                  # holes
        views.append(dict(depth=depth.astype(np.float32), intrinsics=K, pose=P))
    return views


def pair_block(views, i, j):
    return param_block(views[i]['intrinsics'], views[j]['intrinsics'], relative_pose(views[i]['pose'], views[j]['pose']))


def off_tie(k):
    """float32 coordinates nearer than 2 * MIN_TIE_MARGIN to a ``.5`` tie, but not on it, moved by 0.01."""
    k = np.asarray(k, np.float32).copy()
    frac = np.abs((k.astype(np.float64) - np.floor(k.astype(np.float64))) - 0.5)
    near = (frac != 0.0) & (frac < 2 * MIN_TIE_MARGIN)
    k[near] += np.float32(0.01)
    return k


def make_matches(views, i, j, n, seed, noise=0.3, outliers=0.25):
    """``n`` matches of view ``i`` against view ``j`` -> float32 ``(k1 [n,2], k2 [n,2])``: pixels of map ``i`` (holes
    take a stand-in depth) un-projected, moved by ``T_1to2`` and projected into view ``j``; both ends get Gaussian
    noise of ``noise`` px (at least 0.02 px on every coordinate: no match is exact), a share ``outliers`` of the far
    ends lands anywhere in (and a little outside of) picture ``j``."""
    rng = np.random.default_rng(seed)
    h1, w1 = views[i]['depth'].shape
    h2, w2 = views[j]['depth'].shape
    P = pair_block(views, i, j)
    c, r = rng.integers(0, w1, n), rng.integers(0, h1, n)
    z = views[i]['depth'][r, c].astype(np.float64)
    z = np.where(z > 0, z, 9.0 + rng.random(n))
    x, y = (c - P[2]) / P[0] * z, (r - P[3]) / P[1] * z
    R, t = P[8:17].reshape(3, 3), P[17:20]
    q = [(R[k][0] * x + R[k][1] * y) + R[k][2] * z + t[k] for k in range(3)]
    with np.errstate(all='ignore'):
        far = np.stack([P[4] * (q[0] / q[2]) + P[6], P[5] * (q[1] / q[2]) + P[7]], 1)
    far[~np.isfinite(far)] = 0.0
    far = np.clip(far, -1e4, 1e4)

    def jitter(shape):
        e = noise * rng.standard_normal(shape)
        return np.where(np.abs(e) < 0.02, 0.02, e)
    k1 = np.stack([c, r], 1).astype(np.float64) + jitter((n, 2))
    k2 = far + jitter((n, 2))
    out = rng.random(n) < outliers
    anywhere = np.stack([rng.uniform(-2, w2 + 2, n), rng.uniform(-2, h2 + 2, n)], 1)
    k2[out] = anywhere[out]
    return off_tie(k1), off_tie(k2)


def special_points(shape):
    """The hand-made coordinates of one ``(H, W)`` map, float32 ``[16,2]``: exact ``.5`` ties (half to even goes both
    ways), -0.5 (rounds to -0: inside) and -0.51 (outside), ``W - 0.5`` / ``W - 0.49`` and ``H - 0.5`` / ``H - 0.49``,
    +-inf and NaN in either coordinate."""
    h, w = shape
    inf, nan = np.inf, np.nan
    xs = [0.5, 1.5, 2.5, -0.5, -0.51, w - 0.5, w - 0.49, inf, -inf, nan, 1.0, 1.0, 1.0, 2.0, 0.0, 3.5]
    ys = [1.5, 0.5, 2.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, inf, nan, -0.5, h - 0.5, h - 0.49, 4.5]
    return np.array([xs, ys], np.float32).T


def special_matches(shape1, shape2):
    """48 rows ``(k1, k2)``: the special points of map 1 against a plain point, a plain point against those of map 2,
    and both at once."""
    s1, s2 = special_points(shape1), special_points(shape2)
    plain = np.full_like(s1, 1.25)
    return np.concatenate([s1, plain, s1]), np.concatenate([plain, s2, s2])


# The pair list of the tests and of the pinned lists: both orders, self pairs, map 2 on nine pairs; the list lengths
# straddle a wave (64) and a workgroup (256).
PAIRS = ((2, 3), (3, 2), (2, 2), (3, 3), (0, 2), (2, 0), (1, 2), (2, 1), (1, 3), (3, 1), (0, 0), (2, 3), (3, 2), (1, 1))
LENGTHS = (600, 257, 256, 255, 65, 64, 63, 1, 0, 600, 64, 65, 257, 63)
THRESHOLDS = dict(epi_thr=5e-4, sym_thr=1e-4, px_thr=3.0)


def make_lists(views, pairs=PAIRS, lengths=LENGTHS, seed=0):
    """One finite match list per pair: ``[(k1, k2), ...]`` float32."""
    return [make_matches(views, i, j, n, seed=1000 * seed + 10 * p + 1) for p, ((i, j), n) in enumerate(zip(pairs, lengths))]


def score_lists(views, pairs, lists, blocks=None, **thr):
    """``score`` of every list; ``blocks``: the parameter blocks to use (default: ``pair_block`` of each pair)."""
    return [score(views[i]['depth'], views[j]['depth'], pair_block(views, i, j) if blocks is None else blocks[p], k1, k2, **thr)
            for p, ((i, j), (k1, k2)) in enumerate(zip(pairs, lists))]


def list_record(res):
    """One scored list as JSON-able recorded values: the counters, and flags and values by hash."""
    rec = dict(counts=[int(c) for c in res['counts']], flags_sha256=cvo.sha(res['flags']))
    rec.update({k + '_sha256': cvo.sha(res[k]) for k in VALUES})
    return rec


# ------------------------------------------------------------------ the reference's own functions
def load_reference(ref_dir):
    """The reference's ``dloc/evaluate/utils/utils.py`` and ``evaluation.py`` from the snapshot in ``ref_dir``
    (``oracle/_ref``) as two modules ``(utils, evaluation)``, loaded from their files alone: ``cv2`` and ``skimage``
    are empty stand-ins for the duration of the load only - ``sys.modules`` is put back as it was."""
    import importlib.util
    import sys
    import types
    from pathlib import Path
    base = Path(ref_dir) / 'dloc' / 'evaluate' / 'utils'
    pkg = 'ref_dloc_evaluate_utils'
    names = ('cv2', 'skimage', 'skimage.measure', 'skimage.transform', pkg, pkg + '.utils', pkg + '.evaluation')
    before = {n: sys.modules.get(n) for n in names}
    try:
        sys.modules.setdefault('cv2', types.ModuleType('cv2'))
        if 'skimage' not in sys.modules:
            sk = types.ModuleType('skimage')
            sk.measure, sk.transform = types.ModuleType('skimage.measure'), types.ModuleType('skimage.transform')
            sys.modules.update({'skimage': sk, 'skimage.measure': sk.measure, 'skimage.transform': sk.transform})
        holder = types.ModuleType(pkg)
        holder.__path__ = [str(base)]
        sys.modules[pkg] = holder
        mods = []
        for name in ('utils', 'evaluation'):                    # evaluation does `from .utils import ...`
            spec = importlib.util.spec_from_file_location(f'{pkg}.{name}', base / f'{name}.py')
            mod = importlib.util.module_from_spec(spec)
            sys.modules[f'{pkg}.{name}'] = mod
            spec.loader.exec_module(mod)
            mods.append(mod)
    finally:
        for n, m in before.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return tuple(mods)


def reference_scores(ref, depth1, depth2, P, k1, k2, epi_thr=5e-4, sym_thr=None, px_thr=None):
    """The reference's ``compute_epipolar_error``, ``get_episym`` and ``get_projected_kp`` + ``get_truesym`` (through
    ``normalize_keypoints`` / ``unnormalize_keypoints``) on one FINITE list, shaped like ``score``'s result; the
    distances squared for the comparison.  The depth look-up is ``pose_evaluate``'s (``np.round``, then the range
    test on integers), ``correct`` / ``precision`` are ``validation_error``'s."""
    utils, evaluation = ref
    P = np.asarray(P, np.float64)
    K1 = np.array([[P[0], 0, P[2]], [0, P[1], P[3]], [0, 0, 1]])
    K2 = np.array([[P[4], 0, P[6]], [0, P[5], P[7]], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = P[8:17].reshape(3, 3), P[17:20]
    k1, k2 = np.asarray(k1, np.float64).reshape(-1, 2), np.asarray(k2, np.float64).reshape(-1, 2)
    n = len(k1)
    res = dict(epi_ref=np.zeros(0), episym=np.zeros(0), reproj12_sq=np.zeros(0), reproj21_sq=np.zeros(0),
               flags=np.zeros(0, np.uint8), precision=0)
    if n:
        with np.errstate(all='ignore'):
            epi = evaluation.compute_epipolar_error(k1, k2, T, K1, K2)
            n1, n2 = utils.normalize_keypoints(k1, K1), utils.normalize_keypoints(k2, K2)
            sym = utils.get_episym(n1, n2, T[:3, :3], T[:3, 3])
            d = []
            for k, depth in ((k1, depth1), (k2, depth2)):
                at = np.round(k).astype(int)
                ok = (at[:, 0] >= 0) & (at[:, 0] < depth.shape[1]) & (at[:, 1] >= 0) & (at[:, 1] < depth.shape[0])
                col = np.zeros((n, 1))
                col[ok, 0] = depth[at[ok, 1], at[ok, 0]]
                d.append(col)
            p1, p2 = utils.get_projected_kp(n1, n2, d[0], d[1], T[:3, :3], T[:3, 3].reshape(3, 1))
            p1 = utils.unnormalize_keypoints(np.reshape(p1, (n, 2)), K2)
            p2 = utils.unnormalize_keypoints(np.reshape(p2, (n, 2)), K1)
            d21 = np.asarray(utils.get_truesym(k1, k2, p1, p2))         # its `ys = ys2`: |x2p - x1|
            d12 = np.asarray(utils.get_truesym(k2, k1, p2, p1))         # the other direction, by swapping the roles
            has1, has2 = d[0][:, 0] != 0, d[1][:, 0] != 0
            correct = epi < (np.nan if epi_thr is None else epi_thr)
            ok_sym = sym < (np.nan if sym_thr is None else sym_thr)
            ok_px = has1 & has2 & (d21 < (np.nan if px_thr is None else px_thr))
        flags = (has1 * FLAG_DEPTH1 + has2 * FLAG_DEPTH2 + correct * FLAG_EPI + ok_sym * FLAG_EPISYM
                 + ok_px * FLAG_REPROJ).astype(np.uint8)
        res = dict(epi_ref=epi, episym=sym, reproj12_sq=d12 * d12, reproj21_sq=d21 * d21, flags=flags,
                   precision=np.mean(correct))
    f = res['flags']
    off = lambda bit, t: -1 if t is None else int(((f & bit) != 0).sum())
    res['counts'] = np.array([n, off(FLAG_EPI, epi_thr), off(FLAG_EPISYM, sym_thr), int(((f & 3) == 3).sum()),
                              off(FLAG_REPROJ, px_thr)], np.int32)
    return res
