"""The specification of the dual-softmax coarse matcher (``match_dense``, ``include/oetr_dual_softmax.h``):
numpy, no torch, no GPU, float32 with every operation rounded on its own, in a fixed order.

This is THE PROJECT'S OWN STATEMENT, modelled on LoFTR's published coarse matching (similarity, a softmax along both
axes, threshold, border removal, the mutual-maximum test).  That code lives in a ``third_party/`` tree outside the
reference checkout, so no parity with it is claimed.

* the similarity is ``nn_match_oracle.similarity`` - ONE float32 ``fmaf`` chain per ``(i, j)`` over ascending ``d``, what
  gfx950's f32-input MFMA computes - and ``t = s * scale`` with ONE float32 ``scale`` (:func:`scale_of`).  A non-finite
  ``t`` is no candidate: it enters no maximum and no sum, and is nobody's match;
* ``e(x)`` (:func:`e32`) is a stated float32 exponential for ``x <= 0``, exactly 0 below :data:`E_CUT` and never
  subnormal;
* a row's sum (:func:`ordered_sum`) is :data:`PARTIALS` partial sums by position (:func:`slot`), each taking its
  columns in ascending ``j``, then one fixed tree;
* ``conf = (e(t - m_i) / Z_i) * (e(t - c_j) / Y_j)``: two divisions and one product, each rounded; an element with a
  factor below :data:`Q_MIN` ``= 2^-62`` is no candidate, so no product is ever subnormal (and a subnormal quotient is
  below ``2^-62`` whether or not the hardware flushes it);
* the decision takes the LOWEST index that attains a maximum.

Every function takes leading batch dimensions, so many pairs of one shape are one call.
"""
import numpy as np

from nn_match_oracle import fma32, similarity

COUNTERS = 4                 # L, S, rows over the threshold and off the border, rows matched
PARTIALS = 8
F32 = np.float32
NEG_INF = F32(-np.inf)

E_CUT = F32(-87.0)
E_LOG2E = F32(1.44269502162933349609375)
E_LN2_HI = F32(0.693359375)
E_LN2_LO = F32(-2.12194440e-4)
# from the highest power down; then 1, 1
E_POLY = tuple(F32(c) for c in (1.9875691500e-4, 1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 0.5))
Q_MIN = F32(2.0 ** -62)


def scale_of(D, temperature):
    """The ONE float32 the wrapper computes: ``float32(1 / (D * temperature))``, formed in double."""
    return F32(1.0 / (float(D) * float(temperature)))


def e32(x):
    """``e(x)`` for ``x <= 0`` (finite or -inf): 0 below the cut-off; else ``n = rint(x * log2e)``, ``r = x - n ln 2``
    in two ``fmaf``, the polynomial by Horner in seven ``fmaf``, ``n`` added to the exponent field."""
    x = np.asarray(x, F32)
    with np.errstate(all='ignore'):
        live = x >= E_CUT
        xs = np.where(live, x, F32(0))
        n = np.rint(xs * E_LOG2E).astype(F32)
        r = fma32(n, -E_LN2_HI, xs)
        r = fma32(n, -E_LN2_LO, r)
        p = np.broadcast_to(E_POLY[0], r.shape)
        for c in E_POLY[1:] + (F32(1), F32(1)):
            p = fma32(p, r, c)
        bits = p.view(np.int32) + n.astype(np.int32) * np.int32(1 << 23)
        return np.where(live, bits.view(F32), F32(0)).astype(F32)


def is_candidate(t):
    return np.isfinite(t)


def slot(j):
    """The partial sum column ``j`` belongs to: within a tile of 128 columns, the 64-column half, the lane half
    ``(j / 4) % 2`` and the 32-column accumulator."""
    j = np.asarray(j)
    return ((j >> 6) & 1) * 4 + ((j >> 2) & 1) * 2 + ((j >> 5) & 1)


def tree(partials):
    """``((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))`` along the last axis, float32."""
    p = np.asarray(partials, F32)
    assert p.shape[-1] == PARTIALS
    while p.shape[-1] > 1:
        p = (p[..., 0::2] + p[..., 1::2]).astype(F32)
    return p[..., 0]


def ordered_sum(terms):
    """The stated sum along the last axis: every partial starts at +0 and adds its columns in ascending ``j``."""
    terms = np.asarray(terms, F32)
    K = terms.shape[-1]
    part = np.zeros(terms.shape[:-1] + (PARTIALS,), F32)
    slots = slot(np.arange(K))
    for s in range(PARTIALS):
        for j in np.nonzero(slots == s)[0]:
            part[..., s] = part[..., s] + terms[..., j]
    return tree(part)


def statistics(t):
    """``(m, Z)`` of every row of ``t`` ``[..., L, S]``: the maximum of the row's candidates (-inf without one) and the
    stated sum of ``e(t - m)`` over them (a non-candidate adds +0, which changes no bit)."""
    t = np.asarray(t, F32)
    lead = t.shape[:-1]
    if t.shape[-1] == 0:
        return np.full(lead, NEG_INF), np.zeros(lead, F32)
    cand = is_candidate(t)
    m = np.where(cand, t, NEG_INF).max(-1).astype(F32)
    with np.errstate(all='ignore'):
        terms = np.where(cand, e32(np.where(cand, t - m[..., None], NEG_INF)), F32(0))
    return m, ordered_sum(terms)


def confidence(t):
    """``(conf, cand)``: the confidence of every element of ``t`` ``[..., L, S]`` and which elements are candidates."""
    t = np.asarray(t, F32)
    m, Z = statistics(t)
    c, Y = statistics(np.swapaxes(t, -1, -2))
    with np.errstate(all='ignore'):
        fin = is_candidate(t)
        q0 = (e32(np.where(fin, t - m[..., :, None], NEG_INF)) / Z[..., :, None]).astype(F32)
        q1 = (e32(np.where(fin, t - c[..., None, :], NEG_INF)) / Y[..., None, :]).astype(F32)
        cand = fin & (q0 >= Q_MIN) & (q1 >= Q_MIN)
        conf = np.where(cand, (q0 * q1).astype(F32), F32(-1))
    return conf, cand


def best(conf, cand):
    """``(value, index)`` along the last axis: the maximum confidence over the candidates and the LOWEST index that
    attains it; ``(0, -1)`` without a candidate."""
    lead = conf.shape[:-1]
    if conf.shape[-1] == 0:
        return np.zeros(lead, F32), np.full(lead, -1, np.int32)
    v = np.where(cand, conf, F32(-1))
    top = v.max(-1)
    first = np.argmax(cand & (v == top[..., None]), -1)
    has = cand.any(-1)
    return np.where(has, top, F32(0)).astype(F32), np.where(has, first, -1).astype(np.int32)


def inside(i, h, w, border):
    row, col = i // max(w, 1), i % max(w, 1)
    return (row >= border) & (row < h - border) & (col >= border) & (col < w - border)


def keypoints(h, w, cell):
    """``(col * cell, row * cell)`` of every token of an ``h x w`` grid in raster order, float32 ``[h * w, 2]``."""
    i = np.arange(h * w)
    return np.stack([(i % max(w, 1)) * cell, (i // max(w, 1)) * cell], -1).astype(F32).reshape(-1, 2)


def match_t(t, grid0, grid1, threshold=0.2, border_rm=2):
    """The matcher on ``t = s * scale`` ``[..., L, S]`` with ``grid_i = (h, w)``: ``matches0`` after the tests,
    ``matching_scores0`` (the row's maximum confidence BEFORE them), ``matches1`` (direction 1's argmax before them)
    and the counters."""
    t = np.asarray(t, F32)
    L, S = t.shape[-2:]
    assert grid0[0] * grid0[1] == L and grid1[0] * grid1[1] == S and threshold >= 0
    conf, cand = confidence(t)
    s0, j_star = best(conf, cand)
    _, i_star = best(np.swapaxes(conf, -1, -2), np.swapaxes(cand, -1, -2))
    i = np.arange(L)
    safe = np.where(j_star > -1, j_star, 0).astype(np.int64)
    over = (j_star > -1) & (s0 > F32(threshold)) & inside(i, *grid0, border_rm) & inside(safe, *grid1, border_rm)
    if S:
        mutual = np.take_along_axis(i_star, safe, -1) == i
    else:
        mutual = np.zeros(j_star.shape, bool)
    keep = over & mutual
    lead = t.shape[:-2]
    counts = np.stack([np.full(lead, L), np.full(lead, S), over.sum(-1), keep.sum(-1)], -1).astype(np.int32)
    return dict(matches0=np.where(keep, j_star, -1).astype(np.int32), matching_scores0=s0, matches1=i_star,
                counts=counts)


def match_pair(A, B, grid0, grid1, temperature=0.1, threshold=0.2, border_rm=2):
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    t = (similarity(A, B) * scale_of(A.shape[-1], temperature)).astype(F32)
    return match_t(t, grid0, grid1, threshold, border_rm)


def match_call(ts, grids0, grids1, n_tok0, n_tok1, off0, off1, threshold=0.2, border_rm=2, cell=8, max_k0=None,
               max_k1=None):
    """What one device call returns, in its joined form.  ``ts[p]``: ``t`` of pair ``p`` (or ``None`` for a pair whose
    grids do not multiply to its rows), whose sides own rows ``off_i[p] .. off_i[p+1]-1``.  Rows no pair owns read
    -1 / 0 / NaN; a pair beyond ``max_k*`` or with wrong grids is not matched: four -1 and its rows -1 / 0 / NaN."""
    out = dict(matches0=np.full(n_tok0, -1, np.int32), matching_scores0=np.zeros(n_tok0, F32),
               matches1=np.full(n_tok1, -1, np.int32), keypoints0=np.full((n_tok0, 2), np.nan, F32),
               keypoints1=np.full((n_tok1, 2), np.nan, F32), counts=np.full((len(ts), COUNTERS), -1, np.int32))
    for p, t in enumerate(ts):
        K0, K1 = int(off0[p + 1] - off0[p]), int(off1[p + 1] - off1[p])
        g0, g1 = tuple(int(v) for v in grids0[p]), tuple(int(v) for v in grids1[p])
        if min(g0 + g1) < 0 or g0[0] * g0[1] != K0 or g1[0] * g1[1] != K1:
            continue
        if (max_k0 is not None and K0 > max_k0) or (max_k1 is not None and K1 > max_k1):
            continue
        res = match_t(t, g0, g1, threshold, border_rm)
        out['matches0'][off0[p]:off0[p + 1]] = res['matches0']
        out['matching_scores0'][off0[p]:off0[p + 1]] = res['matching_scores0']
        out['matches1'][off1[p]:off1[p + 1]] = res['matches1']
        out['keypoints0'][off0[p]:off0[p + 1]] = keypoints(*g0, cell)
        out['keypoints1'][off1[p]:off1[p + 1]] = keypoints(*g1, cell)
        out['counts'][p] = res['counts']
    return out


def published_head(A, B, grid0, grid1, temperature=0.1, threshold=0.2, border_rm=2):
    """A plain float64 restatement of the published head, for the CPU test's comparison: ``softmax(dim=1) *
    softmax(dim=2)``, ``> thr``, the border, the two ``== max`` tests.  Returns ``matches0`` (-1: none), the counters'
    last two entries, the confidence matrix and the smallest relative margins it met (best against second confidence
    per row and column, confidence against threshold)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    L, S = len(A), len(B)
    sim = A @ B.T / (A.shape[1] * temperature)
    conf = np.exp(sim - sim.max(1, keepdims=True))
    conf = conf / conf.sum(1, keepdims=True)
    col = np.exp(sim - sim.max(0, keepdims=True))
    conf = conf * (col / col.sum(0, keepdims=True))
    mask = conf > threshold
    mask &= inside(np.arange(L), *grid0, border_rm)[:, None] & inside(np.arange(S), *grid1, border_rm)[None, :]
    over = (mask & (conf == conf.max(1, keepdims=True))).any(1)
    mask &= (conf == conf.max(1, keepdims=True)) & (conf == conf.max(0, keepdims=True))
    matches = np.where(mask.any(1), mask.argmax(1), -1).astype(np.int32)
    margins = []
    for c in (conf, conf.T):
        if c.shape[1] >= 2:
            two = np.sort(c, 1)[:, -2:]
            margins.append(((two[:, 1] - two[:, 0]) / two[:, 1]).min())
    if threshold > 0:
        margins.append((np.abs(conf.max(1) - threshold) / threshold).min())
    return dict(matches0=matches, over=int(over.sum()), kept=int((matches > -1).sum()), conf=conf,
                margin=float(min(margins)) if margins else np.inf)
