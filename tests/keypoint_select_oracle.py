"""The specification of keypoint selection (``select_keypoints``, ``include/oetr_keypoint_select.h``):
numpy, float32, a fixed operation order, no torch, no GPU.

It is this project's own statement, modelled on SuperPoint's published post-processing - ``simple_nms`` with its two
suppression rounds, ``remove_borders``, ``top_k_keypoints``, ``sample_descriptors`` - with everything that code leaves
to torch decided:

* a NaN score is loaded as ``-inf`` (:func:`load_scores`);
* ``pool`` counts only positions inside the map (:func:`pool`);
* with more candidates than ``max_keypoints`` the best are kept in descending score order and a tie goes to the LOWER
  raster index (``torch.topk`` leaves it open); otherwise all are kept in raster order (:func:`select`);
* the descriptor arithmetic rounds every product and sum on its own, sums the four taps as ``((nw + ne) + sw) + se``
  and the squares in 64 partial sums joined by a fixed tree (:func:`sample_descriptors`).
"""
import numpy as np

COUNTERS = 2                 # candidates, kept
F32 = np.float32
NEG_INF = F32(-np.inf)
EPS = F32(1e-12)
MAX_RADIUS, MAX_KEYPOINTS = 8, 4096


def load_scores(S):
    S = np.asarray(S, F32)
    return np.where(np.isnan(S), NEG_INF, S)


def pool(X, r, fill):
    """The maximum over the ``(2r+1)^2`` window, positions outside the map not counted (``fill``: a value below every
    entry).  The maximum is exact, so the order - rows, then columns - does not matter."""
    H, W = X.shape
    P = np.full((H, W + 2 * r), fill, X.dtype)
    P[:, r:r + W] = X
    R = P[:, 0:W].copy()
    for dx in range(1, 2 * r + 1):
        R = np.maximum(R, P[:, dx:dx + W])
    P = np.full((H + 2 * r, W), fill, X.dtype)
    P[r:r + H] = R
    R = P[0:H].copy()
    for dy in range(1, 2 * r + 1):
        R = np.maximum(R, P[dy:dy + H])
    return R


def nms_mask(S, r):
    """``simple_nms``'s final mask ``M`` on loaded scores ``S`` ``[H,W]``."""
    M = S == pool(S, r, NEG_INF)
    for _ in range(2):
        supp = pool(M.astype(np.uint8), r, 0) > 0
        S2 = np.where(supp, F32(0), S)
        M = M | ((S2 == pool(S2, r, NEG_INF)) & ~supp)
    return M


def simple_nms(S, r):
    """``N = where(M, S, 0)`` of a raw score map."""
    S = load_scores(S)
    return np.where(nms_mask(S, r), S, F32(0))


def select(S, nms_radius, threshold, remove_borders, max_keypoints):
    """``(raster indices of the kept keypoints in output order, number of candidates)`` of a raw score map."""
    S = load_scores(S)
    H, W = S.shape
    N = np.where(nms_mask(S, nms_radius), S, F32(0))
    b = int(remove_borders)
    ys, xs = np.mgrid[0:H, 0:W]
    cand = (N > F32(threshold)) & (ys >= b) & (ys < H - b) & (xs >= b) & (xs < W - b)
    idx = np.flatnonzero(cand.reshape(-1))                           # raster order
    if len(idx) > max_keypoints:
        bits = S.reshape(-1)[idx].view(np.uint32).astype(np.int64)   # positive floats order as their bit patterns
        idx = idx[np.lexsort((idx, -bits))[:max_keypoints]]
    return idx.astype(np.int64), int(cand.sum())


def sample_coordinate(kp, n, cell):
    """SuperPoint's ``sample_descriptors`` normalisation followed by ``grid_sample``'s ``align_corners=True``
    un-normalisation, float32, one rounding per operation.  ``kp`` float32 array, ``n``: the map's ``w`` (or ``h``)."""
    kp = np.asarray(kp, F32)
    half = F32(cell / 2)
    den = F32(float(n) * cell - cell / 2 - 0.5)
    with np.errstate(all='ignore'):
        t = (kp - half) + F32(0.5)
        g = (t / den) * F32(2) - F32(1)
        return ((g + F32(1)) / F32(2)) * F32(n - 1)


def sample_descriptors(F, xs, ys, cell):
    """``[K,D]`` float32: the descriptors of the keypoints ``(xs[i], ys[i])`` from the map ``F`` ``[D,h,w]``."""
    F = np.asarray(F, F32)
    D, h, w = F.shape
    K = len(xs)
    if K == 0:
        return np.zeros((0, D), F32)
    with np.errstate(all='ignore'):
        ix, iy = sample_coordinate(np.asarray(xs, F32), w, cell), sample_coordinate(np.asarray(ys, F32), h, cell)
        x0, y0 = np.floor(ix), np.floor(iy)
        x1, y1 = x0 + F32(1), y0 + F32(1)
        wx1, wx0, wy1, wy0 = ix - x0, x1 - ix, iy - y0, y1 - iy

        def term(xf, yf, wx, wy):
            inside = (xf >= 0) & (xf <= F32(w - 1)) & (yf >= 0) & (yf <= F32(h - 1))    # NaN: no tap
            xi = np.where(inside, xf, 0).astype(np.int64)
            yi = np.where(inside, yf, 0).astype(np.int64)
            val = F[:, yi, xi].T                                     # [K,D]
            weight = (wx * wy).astype(F32)
            return np.where(inside[:, None], val * weight[:, None], F32(0)).astype(F32)

        v = ((term(x0, y0, wx0, wy0) + term(x1, y0, wx1, wy0)) + term(x0, y1, wx0, wy1)) + term(x1, y1, wx1, wy1)
        p = np.zeros((K, 64), F32)
        for d in range(D):
            p[:, d % 64] = p[:, d % 64] + v[:, d] * v[:, d]
        for stride in (32, 16, 8, 4, 2, 1):
            p[:, :stride] = p[:, :stride] + p[:, stride:2 * stride]
        n = np.sqrt(p[:, 0])
        n = np.where(n < EPS, EPS, n)
        return (v / n[:, None]).astype(F32)


def select_image(S, F, nms_radius=4, threshold=0.005, remove_borders=4, max_keypoints=MAX_KEYPOINTS, cell=8):
    """One image: ``keypoints`` float32 ``[K,2]`` (x, y), ``scores`` ``[K]``, ``descriptors`` ``[K,D]``, ``counts``
    (candidates, kept)."""
    assert 0 <= nms_radius <= MAX_RADIUS and 1 <= max_keypoints <= MAX_KEYPOINTS and threshold >= 0
    S = np.asarray(S, F32)
    W = S.shape[1]
    idx, n_cand = select(S, nms_radius, threshold, remove_borders, max_keypoints)
    ys, xs = idx // W, idx % W
    return dict(keypoints=np.stack([xs, ys], -1).astype(F32).reshape(-1, 2),
                scores=load_scores(S).reshape(-1)[idx].astype(F32),
                descriptors=sample_descriptors(F, xs, ys, cell),
                counts=np.array([n_cand, len(idx)], np.int32))


def join(images, max_keypoints, D):
    """What one device call returns for the per-image results ``images``: ``n * max_keypoints`` rows of capacity, the
    rows from ``offsets[n]`` on -1 / NaN / 0."""
    n = len(images)
    rows = n * max_keypoints
    out = dict(keypoints=np.full((rows, 2), -1, F32), scores=np.full(rows, np.nan, F32),
               descriptors=np.zeros((rows, D), F32), offsets=np.zeros(n + 1, np.int32),
               counts=np.zeros((n, COUNTERS), np.int32))
    at = 0
    for b, im in enumerate(images):
        K = len(im['scores'])
        out['offsets'][b] = at
        out['keypoints'][at:at + K] = im['keypoints']
        out['scores'][at:at + K] = im['scores']
        out['descriptors'][at:at + K] = im['descriptors']
        out['counts'][b] = im['counts']
        at += K
    out['offsets'][n] = at
    return out


def select_call(scores, descriptors, nms_radius=4, threshold=0.005, remove_borders=4, max_keypoints=MAX_KEYPOINTS,
                cell=8):
    images = [select_image(S, F, nms_radius, threshold, remove_borders, max_keypoints, cell)
              for S, F in zip(scores, descriptors)]
    return join(images, max_keypoints, np.asarray(descriptors[0]).shape[0])
