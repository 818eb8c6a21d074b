"""Scoring matches and overlap boxes against a HOMOGRAPHY, as a float64 numpy program: the SPECIFICATION (DESIGN
9.3i) of the planar evaluation protocol (``include/oetr_homography.h``), written with elementwise numpy operations
only (no ``@``, no BLAS: every product, sum and quotient is one IEEE float64 operation, in the order written here), and
the homographies and match lists its tests, the generator of the pinned results (``tools/gen_golden_homography.py``) and
the probe share.

``score`` restates the reference's ``h_evaluate`` (``dloc/evaluate/utils/evaluation.py``) and the counting of its
``benchmark_features`` (``dloc/evaluate/eval_hpatches.py``: ``mean(dist <= thr)`` for ``thr = 1 .. 15``); its one
departure is the project's standing one: the distance is delivered SQUARED and compared with ``thr * thr``.
``overlap_box`` is THIS PROJECT'S OWN statement - the reference has no overlap boxes under a homography: it is
``covis_oracle.overlap_box`` (``numpy_overlap_box``) with the depth-and-pose warp replaced by ``H`` and the landing
pixel rounded half to even, as ``depth_pose.h`` rounds.

Pixel centres sit at INTEGER coordinates (the convention of HPatches' ``H_1_k`` files and of ``h_evaluate``).  Sizes
are ``(H, W)`` pairs throughout.
"""
import math

import numpy as np

import covis_oracle as cvo
import match_score_oracle as mso

PARAM_DOUBLES = 16                 # OETR_HOMOGRAPHY_PARAM_DOUBLES
MAX_THRESHOLDS = 16                # OETR_HOMOGRAPHY_MAX_THRESHOLDS
THRESHOLDS = tuple(range(1, 16))   # the reference's rng = np.arange(1, 16)


def param_block(H, size1, size2):
    """The 16 doubles of one pair: ``H`` row major, ``W1, H1, W2, H2``, three reserved zeros."""
    p = np.zeros(PARAM_DOUBLES, np.float64)
    p[0:9] = np.asarray(H, np.float64).reshape(9)
    p[9:13] = size1[1], size1[0], size2[1], size2[0]
    return p


def apply(H, x, y):
    """-> ``(a0, a1, a2)``: the rows of ``H`` on ``(x, y, 1)``, ``(h_r0*x + h_r1*y) + h_r2``."""
    H = np.asarray(H, np.float64).reshape(3, 3)
    with np.errstate(all='ignore'):
        return tuple((H[r, 0] * x + H[r, 1] * y) + H[r, 2] for r in range(3))


def score(H, k1, k2, thresholds=THRESHOLDS):
    """One pair's list.  ``k1`` / ``k2``: float32 ``[m,2]``, widened to float64 (exact).
    -> dict(dist_sq float64 [m], counts int32 [1 + T], pu, pv float64 [m])."""
    k1 = np.asarray(k1, np.float32).astype(np.float64).reshape(-1, 2)
    k2 = np.asarray(k2, np.float32).astype(np.float64).reshape(-1, 2)
    x, y, x2, y2 = k1[:, 0], k1[:, 1], k2[:, 0], k2[:, 1]
    a0, a1, a2 = apply(H, x, y)
    with np.errstate(all='ignore'):
        pu, pv = a0 / a2, a1 / a2
        dist_sq = (x2 - pu) * (x2 - pu) + (y2 - pv) * (y2 - pv)
        counts = [len(x)] + [int((dist_sq <= np.float64(t) * np.float64(t)).sum()) for t in thresholds]
    return dict(dist_sq=dist_sq, counts=np.array(counts, np.int32), pu=pu, pv=pv)


def tie_distance(c):
    """Distance of every coordinate from the nearest ``.5`` tie of ``rint``."""
    return np.abs((c - np.floor(c)) - 0.5)


def overlap_box(H, W1, H1, W2, H2):
    """-> dict(box1, box2 int64 [4], valid bool, count int, margin float).  Every pixel ``(u, v)`` of picture 1 is
    kept when ``a2 > 0`` and its landing pixel ``(rint(a0 / a2), rint(a1 / a2))`` lies in picture 2 (tested in float64,
    false for NaN).  ``margin``: over every projection that lands within one pixel of picture 2's frame, inside or
    outside it and whatever the sign of ``a2``, the smallest distance of ``u2`` / ``v2`` to a ``.5`` tie and of ``a2``
    to 0."""
    W1, H1, W2, H2 = int(W1), int(H1), int(W2), int(H2)
    v, u = np.mgrid[0:H1, 0:W1]
    u, v = u.reshape(-1), v.reshape(-1)
    a0, a1, a2 = apply(H, u.astype(np.float64), v.astype(np.float64))
    with np.errstate(all='ignore'):
        u2, v2 = a0 / a2, a1 / a2
        i, j = np.rint(u2), np.rint(v2)
        inside = (i >= 0.0) & (i < float(W2)) & (j >= 0.0) & (j < float(H2))
        kept = (a2 > 0.0) & inside
        near = (np.isfinite(u2) & np.isfinite(v2) & (u2 > -1.5) & (u2 < W2 + 0.5) & (v2 > -1.5) & (v2 < H2 + 0.5))
    margin = np.inf
    if near.any():
        margin = float(min(tie_distance(u2[near]).min(), tie_distance(v2[near]).min(), np.abs(a2[near]).min()))
    count = int(kept.sum())
    box1 = box2 = np.zeros(4, np.int64)
    if count:
        uu, vv, ii, jj = u[kept], v[kept], i[kept].astype(np.int64), j[kept].astype(np.int64)
        box1 = np.array([uu.min(), vv.min(), uu.max(), vv.max()], np.int64)
        box2 = np.array([ii.min(), jj.min(), ii.max(), jj.max()], np.int64)
    return dict(box1=box1, box2=box2, valid=count > 0, count=count, margin=margin, a2=a2, inside=inside)


# ------------------------------------------------------------------ homographies
# Drawn like covis_oracle's scenes: elementwise float64 arithmetic, libm's scalar sin / cos and numpy's seeded
# generator only, so a (kind, sizes, seed) recipe gives the same bytes on every machine.
KINDS = ('identity', 'shift', 'similarity', 'zoom_in', 'zoom_out', 'perspective', 'horizon', 'disjoint')
# (picture 1, picture 2) as (H, W): one pixel, one row / one column, transposed, a wave's worth, off every tile, more
# than one workgroup with a short last one, a camera picture
BOX_SIZES = (((1, 1), (1, 1)), ((1, 7), (5, 1)), ((5, 7), (7, 5)), ((64, 64), (64, 64)), ((65, 63), (31, 130)),
             ((256, 257), (100, 75)), ((480, 640), (640, 480)))


def _about_centres(A, size1, size2, frac):
    """The 2x2 map ``A`` about picture 1's centre, onto picture 2's centre moved by ``frac``."""
    (h1, w1), (h2, w2) = size1, size2
    c1, c2 = ((w1 - 1) / 2.0, (h1 - 1) / 2.0), ((w2 - 1) / 2.0 + frac[0], (h2 - 1) / 2.0 + frac[1])
    t = [c2[r] - (A[r][0] * c1[0] + A[r][1] * c1[1]) for r in range(2)]
    return np.array([[A[0][0], A[0][1], t[0]], [A[1][0], A[1][1], t[1]], [0.0, 0.0, 1.0]])


def make_homography(kind, sizes, seed):
    """One ``H`` from picture 1 ``sizes[0]`` to picture 2 ``sizes[1]``.  ``kind``:
      'identity'     the identity;
      'shift'        a fractional translation of a few pixels;
      'similarity'   rotation and scale about the centres;
      'zoom_in'      x4 about the centres;  'zoom_out'  x0.25;
      'perspective'  a similarity with a projective row; ``a2 > 0`` on all of picture 1;
      'horizon'      ``a2`` changes sign inside picture 1, along its longer side, and pixels on BOTH sides of the line
                     land in picture 2 (a picture of one pixel has no room for the line and stays on the kept side);
      'disjoint'     a translation past picture 2: nothing lands in it."""
    rng = np.random.default_rng(seed)
    (h1, w1), (h2, w2) = sizes
    frac = rng.uniform(-0.45, 0.45, 2)
    jit = rng.uniform(-1.0, 1.0, 4)
    if kind == 'identity':
        return np.eye(3)
    if kind == 'shift':
        return np.array([[1.0, 0.0, 3.0 * jit[0]], [0.0, 1.0, 3.0 * jit[1]], [0.0, 0.0, 1.0]])
    if kind == 'disjoint':
        return np.array([[1.0, 0.0, w2 + 7.25 + jit[0]], [0.0, 1.0, 0.25 * jit[1]], [0.0, 0.0, 1.0]])
    if kind in ('zoom_in', 'zoom_out'):
        s = 4.0 if kind == 'zoom_in' else 0.25
        return _about_centres([[s, 0.0], [0.0, s]], sizes[0], sizes[1], frac)
    if kind in ('similarity', 'perspective'):
        s = 0.8 * min(w2 / w1, h2 / h1) * (1.0 + 0.2 * jit[0])
        ang = 0.3 + 0.1 * jit[1]
        c, sn = s * math.cos(ang), s * math.sin(ang)
        Hm = _about_centres([[c, -sn], [sn, c]], sizes[0], sizes[1], frac)
        if kind == 'perspective':
            Hm[2, 0], Hm[2, 1] = 0.2 * jit[2] / w1, 0.2 * jit[3] / h1          # a2 in (0.6, 1.4)
        return Hm
    if kind == 'horizon':
        along_x = w1 >= h1
        L, S = (w1, h1) if along_x else (h1, w1)                              # t runs along the longer side
        L2, S2 = (w2, h2) if along_x else (h2, w2)
        c = 0.6 * L + 0.13 + 0.05 * jit[0]                                    # the line t = c; a2 = 1 - t / c
        # along t: (L2 / 2 - 0.3) + 0.25 * L2 / (c - t); across: (S2 / 2 - 0.2) + 0.3 * S2 * (s / S) / (c - t)
        p, q = (L2 / 2.0 - 0.3 + frac[0]) / c, 0.25 * L2 / c
        r, w = (S2 / 2.0 - 0.2 + frac[1]) / c, 0.3 * S2 / (S * c)
        rows = [[-p, 0.0, p * c + q], [-r, w, r * c], [-1.0 / c, 0.0, 1.0]]
        if not along_x:                                                       # swap the roles of x and y on both sides
            rows = [[rows[1][1], rows[1][0], rows[1][2]], [rows[0][1], rows[0][0], rows[0][2]],
                    [rows[2][1], rows[2][0], rows[2][2]]]
        return np.array(rows)
    raise ValueError(kind)


def checked_homography(kind, sizes, seed):
    """``make_homography`` re-drawn (``seed + 1000 * attempt``) until the decision margin of its boxes is at least
    ``covis_oracle.MIN_MARGIN``.  -> (H, result of ``overlap_box``).  No pair is ever left out of a comparison."""
    (h1, w1), (h2, w2) = sizes
    for attempt in range(20):
        Hm = make_homography(kind, sizes, seed + 1000 * attempt)
        res = overlap_box(Hm, w1, h1, w2, h2)
        if res['margin'] >= cvo.MIN_MARGIN:
            return Hm, res
    raise AssertionError(f'no {kind} homography of {sizes} with margin >= {cvo.MIN_MARGIN} in 20 draws from seed {seed}')


def make_boxes(seed=0, kinds=KINDS, sizes=BOX_SIZES):
    """Every kind x every size pair -> ``[dict(kind, sizes, H, res), ...]`` with checked homographies, kinds outermost."""
    out = []
    for a, kind in enumerate(kinds):
        for b, pair in enumerate(sizes):
            Hm, res = checked_homography(kind, pair, 100 * seed + 31 * a + 7 * b + 5)
            out.append(dict(kind=kind, sizes=pair, H=Hm, res=res))
    return out


def box_record(res):
    return dict(box1=[int(x) for x in res['box1']], box2=[int(x) for x in res['box2']], valid=bool(res['valid']),
                count=int(res['count']))


# ------------------------------------------------------------------ match lists
def make_matches(H, sizes, n, seed, outliers=0.15, exact=4):
    """``n`` matches under ``H`` -> float32 ``(k1 [n,2], k2 [n,2])``: points of picture 1 (the first ``exact`` on
    integer pixels) against their projections moved by 0 .. 20 px in a random direction, so that every threshold from
    1 to 15 decides something; the first ``exact`` far ends are the projection itself (rounded to float32), a share
    ``outliers`` lands anywhere in (and a little outside of) picture 2.  A projection that is not finite, or beyond
    1e4, is replaced by the origin."""
    rng = np.random.default_rng(seed)
    (h1, w1), (h2, w2) = sizes
    k1 = np.stack([rng.uniform(-0.5, w1 - 0.5, n), rng.uniform(-0.5, h1 - 0.5, n)], 1)
    k1[:exact] = np.floor(k1[:exact] + 0.5)
    k1 = k1.astype(np.float32)
    a0, a1, a2 = apply(H, k1[:, 0].astype(np.float64), k1[:, 1].astype(np.float64))
    with np.errstate(all='ignore'):
        far = np.stack([a0 / a2, a1 / a2], 1)
    far[~(np.isfinite(far).all(1) & (np.abs(far) < 1e4).all(1))] = 0.0
    g = rng.standard_normal((n, 2))
    g = g / np.sqrt(g[:, 0:1] * g[:, 0:1] + g[:, 1:2] * g[:, 1:2])
    radius = rng.uniform(0.0, 20.0, (n, 1))
    radius[:exact] = 0.0
    k2 = far + radius * g
    out = rng.random(n) < outliers
    out[:exact] = False
    anywhere = np.stack([rng.uniform(-2, w2 + 2, n), rng.uniform(-2, h2 + 2, n)], 1)
    k2[out] = anywhere[out]
    return k1, k2.astype(np.float32)


# The pinned lists (tests/homography_expected.json): ten lists whose lengths straddle a wave (64) and a workgroup
# (256), empty lists first and last, every kind; then the two deliberately degenerate ones.
LIST_SIZES = ((40, 64), (56, 56))
LIST_KINDS = ('identity', 'shift', 'similarity', 'zoom_in', 'zoom_out', 'perspective', 'horizon', 'disjoint',
              'similarity', 'perspective')
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 0)
DEGENERATE = ('a2_zero', 'nan_H')
A2_ZERO_H = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-0.5, 0.0, 1.0]])


def make_lists(seed=0, kinds=LIST_KINDS, lengths=LENGTHS, sizes=LIST_SIZES):
    """-> ``[dict(kind, H, k1, k2), ...]``: one list per entry of ``kinds`` / ``lengths`` under a checked homography,
    then ``DEGENERATE``: 'a2_zero' (rows 0-3 have ``x = 2`` under ``a2 = 1 - x / 2``: ``a2 == 0`` exactly, ``a0 / a2``
    infinite and, where ``y = 0``, ``a1 / a2 = 0 / 0``; rows 4-7 are finite) and 'nan_H' (a similarity's list of 64
    with ``h01 = NaN``)."""
    lists = []
    for p, (kind, n) in enumerate(zip(kinds, lengths)):
        Hm, _ = checked_homography(kind, sizes, 100 * seed + 7 * p)
        k1, k2 = make_matches(Hm, sizes, n, seed=1000 * seed + 10 * p + 1)
        lists.append(dict(kind=kind, H=Hm, k1=k1, k2=k2))
    k1 = np.array([[2, 0], [2, 1], [2, 5.5], [2, -3], [1, 1], [0, 0], [3, 2], [5, 4]], np.float32)
    k2 = np.array([[2, 0], [0, 0], [1, 1], [7, 7], [2, 2], [0, 0.5], [-6, -4], [-3, -3]], np.float32)
    lists.append(dict(kind='a2_zero', H=A2_ZERO_H.copy(), k1=k1, k2=k2))
    Hm, _ = checked_homography('similarity', sizes, 100 * seed + 77)
    k1, k2 = make_matches(Hm, sizes, 64, seed=1000 * seed + 771)
    Hm = Hm.copy()
    Hm[0, 1] = np.nan
    lists.append(dict(kind='nan_H', H=Hm, k1=k1, k2=k2))
    return lists


def threshold_margin(dist_sq, thresholds=THRESHOLDS):
    """The smallest relative distance of a finite ``dist_sq`` from a ``thr * thr``."""
    d = np.asarray(dist_sq, np.float64)
    d = d[np.isfinite(d)]
    m = np.inf
    for t in thresholds:
        tt = float(t) * float(t)
        if d.size and tt > 0:
            m = min(m, float(np.abs(d - tt).min() / tt))
    return m


def list_record(res):
    return dict(counts=[int(c) for c in res['counts']], dist_sq_sha256=cvo.sha(res['dist_sq']))


def concatenate(lists):
    """-> (params float64 [P,16], k1, k2 float32 [M,2], lengths) of lists drawn for ``LIST_SIZES``."""
    params = np.stack([param_block(e['H'], *LIST_SIZES) for e in lists])
    k1 = np.concatenate([e['k1'] for e in lists]).astype(np.float32).reshape(-1, 2)
    k2 = np.concatenate([e['k2'] for e in lists]).astype(np.float32).reshape(-1, 2)
    return params, k1, k2, [len(e['k1']) for e in lists]


# ------------------------------------------------------------------ the reference's own function
def reference_distances(ref, H, k1, k2):
    """The reference's ``h_evaluate`` on one non-empty list, called as its loader calls it: ``kpts0`` / ``kpts1``
    float32 torch tensors, ``H`` float64, ``matches`` the identity pairing.  -> float64 distances (NOT squared)."""
    import torch
    _, evaluation = ref
    n = len(k1)
    idx = np.stack([np.arange(n), np.arange(n)], 1)
    with np.errstate(all='ignore'):
        dist = evaluation.h_evaluate(np.asarray(H, np.float64), torch.from_numpy(np.asarray(k1, np.float32)),
                                     torch.from_numpy(np.asarray(k2, np.float32)), idx)
    dist = np.asarray(dist)
    assert dist.dtype == np.float64 and dist.shape == (n,), (dist.dtype, dist.shape)
    return dist


def reference_accumulation(counts, seq_names, thresholds=THRESHOLDS):
    """``benchmark_features``' accumulation, transcribed on recorded counters: per pair ``mean(dist <= thr)`` - 0 for
    an empty list, its ``dist = [inf]`` substitute - added to ``i_err[thr]`` or ``v_err[thr]`` by the first letter of
    the sequence's name."""
    i_err = {thr: 0 for thr in thresholds}
    v_err = {thr: 0 for thr in thresholds}
    for row, name in zip(counts, seq_names):
        n = int(row[0])
        for t, thr in enumerate(thresholds):
            share = (int(row[1 + t]) / n) if n else 0.0
            if name[0] == 'i':
                i_err[thr] += share
            else:
                v_err[thr] += share
    return i_err, v_err
