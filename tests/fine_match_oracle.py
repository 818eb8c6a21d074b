"""The specification of the fine-level refinement (``fine_windows`` / ``refine_matches``, ``include/oetr_fine_match.h``,
DESIGN 9.3p): numpy, no torch, no GPU, float32 with every operation rounded on its own, in a fixed order.

This is THE PROJECT'S OWN STATEMENT, modelled on LoFTR's published fine matching (per coarse match a ``W x W`` window
of fine features around both cells, the correlation of window 0's centre with window 1, a softmax over the ``W * W``
positions, its spatial expectation and standard deviation).  That code lives in a ``third_party/`` tree outside the
reference checkout, so no parity with it is claimed.

* the match list is every side-0 token ``a`` of a vouched pair with ``0 <= matches0[a] < S_p``, pair after pair in
  ascending ``a``, cut at the capacity (:func:`match_list`);
* window element ``ky * W + kx`` of a token at coarse ``(row, col)`` is fine token ``(row * stride + ky - W // 2,
  col * stride + kx - W // 2)``, ``+0`` outside the map (:func:`gather`);
* the dot product (:func:`dot16`) is :data:`PARTIALS` ``fmaf`` chains - channel ``c`` belongs to partial
  ``(c // 4) % 16`` - and one fixed tree of adjacent pairs; ``t = s * float32(1 / sqrt(C))``; a non-finite ``t`` is no
  candidate; ``e`` is ``dual_softmax_oracle.e32``; ``Z`` and the four moments are serial sums in ascending ``r``
  (:func:`head`).
"""
import numpy as np

from dual_softmax_oracle import e32
from nn_match_oracle import fma32

WINDOW_COUNTERS = 2          # matched, kept
COUNTERS = 3                 # matched, kept, kept matches without a candidate
PARTIALS = 16
WINDOWS = (3, 5, 7)
F32 = np.float32
NEG_INF = F32(-np.inf)
VAR_MIN = F32(1e-10)


def grid(W):
    """``G[k] = float32((2 k - (W - 1)) / (W - 1))``, formed in double."""
    return ((2.0 * np.arange(W) - (W - 1)) / (W - 1)).astype(F32)


def grid2(W):
    """The rounded squares of ``G``."""
    g = grid(W)
    return (g * g).astype(F32)


def scale_of(C):
    return F32(1.0 / np.sqrt(float(C)))


def radius_of(W, fine_cell):
    return F32(F32(W // 2) * F32(fine_cell))


def partial_of(c):
    return (np.asarray(c) >> 2) % PARTIALS


def tree(partials):
    """The fixed tree of adjacent pairs along the last axis, float32."""
    p = np.asarray(partials, F32)
    assert p.shape[-1] == PARTIALS
    while p.shape[-1] > 1:
        p = (p[..., 0::2] + p[..., 1::2]).astype(F32)
    return p[..., 0]


def dot16(a, B):
    """``a`` ``[..., C]`` against every row of ``B`` ``[..., R, C]`` -> ``[..., R]``: 16 partial ``fmaf`` chains over
    ascending ``c`` from +0, then the tree."""
    a, B = np.asarray(a, F32), np.asarray(B, F32)
    C = a.shape[-1]
    assert C % 4 == 0 and B.shape[-1] == C
    part = np.zeros(B.shape[:-1] + (PARTIALS,), F32)
    with np.errstate(all='ignore'):
        for c in range(C):
            s = int(partial_of(c))
            part[..., s] = fma32(a[..., None, c], B[..., c], part[..., s])
        return tree(part)


def head_of_s(s, W, C):
    """The softmax and the expectation on the dot products ``s`` ``[M, W*W]`` -> ``(expec [M,3], has [M], heat)``."""
    s = np.asarray(s, F32)
    M, WW = s.shape
    assert WW == W * W
    with np.errstate(all='ignore'):
        t = (s * scale_of(C)).astype(F32)
        cand = np.isfinite(t)
        has = cand.any(-1)
        m = np.where(cand, t, NEG_INF).max(-1) if WW else np.full(M, NEG_INF)
        q = np.where(cand, e32(np.where(cand, t - m[:, None], NEG_INF)), F32(0)).astype(F32)
        Z = np.zeros(M, F32)
        for r in range(WW):
            Z = (Z + q[:, r]).astype(F32)
        heat = np.where(has[:, None], (q / Z[:, None]).astype(F32), F32(0)).astype(F32)
        G, G2 = grid(W), grid2(W)
        mom = np.zeros((4, M), F32)
        for r in range(WW):
            ky, kx = divmod(r, W)
            for which, g in enumerate((G[kx], G[ky], G2[kx], G2[ky])):
                mom[which] = fma32(heat[:, r], g, mom[which])
        x, y, xx, yy = mom
        vx = (xx - (x * x).astype(F32)).astype(F32)
        vy = (yy - (y * y).astype(F32)).astype(F32)
        vx, vy = np.where(vx > VAR_MIN, vx, VAR_MIN), np.where(vy > VAR_MIN, vy, VAR_MIN)
        sd = (np.sqrt(vx).astype(F32) + np.sqrt(vy).astype(F32)).astype(F32)
    expec = np.stack([np.where(has, x, F32(0)), np.where(has, y, F32(0)), np.where(has, sd, F32(np.nan))], -1)
    return expec.astype(F32), has, heat


def head(win0, win1, W):
    """``win0``, ``win1`` ``[M, W*W, C]`` -> ``(expec [M,3], has [M])``."""
    win0, win1 = np.asarray(win0, F32), np.asarray(win1, F32)
    M, WW, C = win1.shape
    if M == 0:
        return np.zeros((0, 3), F32), np.zeros(0, bool)
    expec, has, _ = head_of_s(dot16(win0[:, WW // 2], win1), W, C)
    return expec, has


def _range(off, p, n):
    s = min(max(int(off[p]), 0), n)
    e = min(max(int(off[p + 1]), s), n)
    return s, e


def _multiplies(g, r):
    return g[0] >= 0 and g[1] >= 0 and int(g[0]) * int(g[1]) == r[1] - r[0]


def vouched(p, off0, off1, grids0, grids1, foff0, foff1, fgrids0, fgrids1, n_tok0, n_tok1, n_fine0, n_fine1, max_k0):
    """The clamped ranges ``(r0, r1, f0, f1)`` of pair ``p`` when it is vouched for, else ``None``."""
    r0, r1 = _range(off0, p, n_tok0), _range(off1, p, n_tok1)
    f0, f1 = _range(foff0, p, n_fine0), _range(foff1, p, n_fine1)
    ok = (r0[1] - r0[0] <= max_k0 and _multiplies(grids0[p], r0) and _multiplies(grids1[p], r1)
          and _multiplies(fgrids0[p], f0) and _multiplies(fgrids1[p], f1))
    return (r0, r1, f0, f1) if ok else None


def gather(fine, frange, fgrid, cgrid, token, W, stride):
    """The window ``[W*W, C]`` of coarse ``token`` of a ``cgrid`` grid from the fine rows ``frange`` of ``fine``."""
    C = fine.shape[1]
    win = np.zeros((W * W, C), F32)
    row, col = divmod(int(token), int(cgrid[1]))
    for ky in range(W):
        for kx in range(W):
            fy, fx = row * stride + ky - W // 2, col * stride + kx - W // 2
            if 0 <= fy < fgrid[0] and 0 <= fx < fgrid[1]:
                win[ky * W + kx] = fine[frange[0] + fy * int(fgrid[1]) + fx]
    return win


def windows_call(matches0, off0, off1, grids0, grids1, n_tok1, fine0, foff0, fgrids0, fine1, foff1, fgrids1, W=5,
                 stride=4, max_matches=0, max_k0=None):
    """What ``oetr_fine_windows`` returns: ``rows``, ``moffsets``, ``counts``, ``win0``, ``win1``."""
    matches0 = np.asarray(matches0)
    fine0, fine1 = np.asarray(fine0, F32), np.asarray(fine1, F32)
    P, cap, C = len(off0) - 1, int(max_matches), fine0.shape[1]
    n_tok0 = len(matches0)
    max_k0 = n_tok0 if max_k0 is None else max_k0
    rows = np.full((cap, 3), -1, np.int32)
    win0, win1 = np.zeros((cap, W * W, C), F32), np.zeros((cap, W * W, C), F32)
    moffsets, counts = np.zeros(P + 1, np.int32), np.full((P, WINDOW_COUNTERS), -1, np.int32)
    at = 0
    for p in range(P):
        moffsets[p] = min(at, cap)
        v = vouched(p, off0, off1, grids0, grids1, foff0, foff1, fgrids0, fgrids1, n_tok0, n_tok1, len(fine0), len(fine1),
                    max_k0)
        if v is None:
            continue
        r0, r1, f0, f1 = v
        K1 = r1[1] - r1[0]
        m = matches0[r0[0]:r0[1]].astype(np.int64)
        mine = np.nonzero((m >= 0) & (m < K1))[0]
        for a in mine:
            if at < cap:
                rows[at] = (p, a, m[a])
                win0[at] = gather(fine0, f0, fgrids0[p], grids0[p], a, W, stride)
                win1[at] = gather(fine1, f1, fgrids1[p], grids1[p], m[a], W, stride)
            at += 1
        counts[p] = (len(mine), min(at, cap) - moffsets[p])
    moffsets[P] = min(at, cap)
    return dict(rows=rows, moffsets=moffsets, counts=counts, win0=win0, win1=win1)


def refine_call(win0, win1, rows, moffsets, wcounts, keypoints0, off0, keypoints1, off1, W=5, fine_cell=2.0):
    """What ``oetr_fine_refine`` returns: ``expec``, ``mkpts0``, ``mkpts1``, ``keypoints1`` (the refined copy),
    ``counts``."""
    win0, win1 = np.asarray(win0, F32), np.asarray(win1, F32)
    kp0, kp1 = np.asarray(keypoints0, F32).reshape(-1, 2), np.asarray(keypoints1, F32).reshape(-1, 2)
    cap, P = len(rows), len(moffsets) - 1
    total = min(max(int(moffsets[P]), 0), cap)
    expec = np.full((cap, 3), np.nan, F32)
    mkpts0, mkpts1 = np.full((cap, 2), np.nan, F32), np.full((cap, 2), np.nan, F32)
    kp1f = kp1.copy()
    live = np.zeros(cap, bool)
    where0, where1 = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    for m in range(total):
        p, a, j = (int(v) for v in rows[m])
        if not 0 <= p < P:
            continue
        r0, r1 = _range(off0, p, len(kp0)), _range(off1, p, len(kp1))
        if 0 <= a < r0[1] - r0[0] and 0 <= j < r1[1] - r1[0]:
            live[m], where0[m], where1[m] = True, r0[0] + a, r1[0] + j
    idx = np.nonzero(live)[0]
    e, has = head(win0[idx], win1[idx], W)
    radius = radius_of(W, fine_cell)
    with np.errstate(all='ignore'):
        expec[idx] = e
        mkpts0[idx] = kp0[where0[idx]]
        mkpts1[idx] = (kp1[where1[idx]] + (e[:, :2] * radius).astype(F32)).astype(F32)
    kp1f[where1[idx]] = mkpts1[idx]
    counts = np.full((P, COUNTERS), -1, np.int32)
    for p in range(P):
        if wcounts[p][0] < 0:
            continue
        s = min(max(int(moffsets[p]), 0), cap)
        e_ = min(max(int(moffsets[p + 1]), s), cap)
        counts[p] = (wcounts[p][0], wcounts[p][1], int(np.isnan(expec[s:e_, 2]).sum()))
    return dict(expec=expec, mkpts0=mkpts0, mkpts1=mkpts1, keypoints1=kp1f, counts=counts)


def published_fine(fine0_map, fine1_map, tokens0, tokens1, cgrid0, cgrid1, W, stride):
    """A plain float64 restatement of the published head for ONE pair, for the CPU test's comparison: ``unfold``-style
    windows of the whole zero-padded fine maps ``[hf, wf, C]``, indexed by the matches, ``einsum`` of the centre with
    window 1, ``softmax(sim / sqrt(C))``, the expectation over a ``linspace(-1, 1, W)`` grid and its standard
    deviation.  Returns ``(win0, win1, expec [M,3])`` in float64."""
    def unfold(fmap, cgrid):
        hf, wf, C = fmap.shape
        pad = W // 2
        big = np.zeros(((cgrid[0] - 1) * stride + W + hf, (cgrid[1] - 1) * stride + W + wf, C))
        big[pad:pad + hf, pad:pad + wf] = fmap
        out = np.zeros((cgrid[0] * cgrid[1], W * W, C))
        for row in range(cgrid[0]):
            for col in range(cgrid[1]):
                out[row * cgrid[1] + col] = big[row * stride:row * stride + W, col * stride:col * stride + W].reshape(W * W, C)
        return out
    u0 = unfold(np.asarray(fine0_map, np.float64), cgrid0)[np.asarray(tokens0, np.int64)]
    u1 = unfold(np.asarray(fine1_map, np.float64), cgrid1)[np.asarray(tokens1, np.int64)]
    C = u0.shape[-1]
    sim = np.einsum('mc,mrc->mr', u0[:, W * W // 2], u1) / np.sqrt(C)
    heat = np.exp(sim - sim.max(1, keepdims=True))
    heat = heat / heat.sum(1, keepdims=True)
    lin = np.linspace(-1, 1, W)
    gx, gy = np.tile(lin, W), np.repeat(lin, W)
    x, y = heat @ gx, heat @ gy
    var_x, var_y = heat @ gx ** 2 - x ** 2, heat @ gy ** 2 - y ** 2
    sd = np.sqrt(np.maximum(var_x, 1e-10)) + np.sqrt(np.maximum(var_y, 1e-10))
    return u0, u1, np.stack([x, y, sd], -1)
