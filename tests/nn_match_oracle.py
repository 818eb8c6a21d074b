"""The specification of the nearest-neighbour matcher (``match_descriptors``, ``include/oetr_nn_match.h``):
numpy, no torch, no GPU.  It restates ``find_nn`` / ``mutual_check`` / ``NearestNeighbor`` of the reference's
``dloc/core/matchers/nearest_neighbor.py`` with everything the reference leaves to torch decided:

* the similarity is ONE float32 ``fmaf`` chain per ``(i, j)`` over ascending ``d`` (:func:`similarity`) - what gfx950's
  f32-input MFMA computes - so direction 1's similarity is the transpose, bit for bit;
* the top two of a row are order-free (:func:`top2`): NaN and -inf are no candidates, the LOWEST index attains the
  maximum (torch's ``topk`` leaves a tied index open: a stated departure), the second value counts multiplicity and is
  -inf with fewer than two candidates (so ``K1 = 1`` passes a ratio test where the reference's ``topk(2)`` raises: the
  second departure);
* ``find_nn`` runs in float32 with one rounding per operation (:func:`find_nn`).

Every function takes leading batch dimensions, so many pairs of one shape are one call.
"""
import numpy as np

COUNTERS = 4                 # K0, K1, rows of side 0 that pass find_nn, rows matched after the mutual check
F32 = np.float32
NEG_INF = F32(-np.inf)


def fma32(a, b, c):
    """``fmaf(a, b, c)`` on float32 arrays, exactly: the product is exact in float64; the sum is taken by TwoSum and,
    where it is inexact and the float64 sum's last mantissa bit is even, moved one ulp towards the true value (round to
    odd), so the final rounding to float32 sees on which side of a float32 midpoint the true value lies."""
    a, b, c = np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32)
    with np.errstate(all='ignore'):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = np.broadcast_to(c.astype(np.float64), p.shape)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) == 1
        move = np.isfinite(s) & (err != 0) & ~odd
        s = np.where(move, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def similarity(A, B):
    """``sim[..., i, j]``: ``acc = 0; for d ascending: acc = fmaf(A[..., i, d], B[..., j, d], acc)``.
    ``A`` ``[..., K0, D]``, ``B`` ``[..., K1, D]`` float32."""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    acc = np.zeros(A.shape[:-1] + (B.shape[-2],), F32)
    if acc.size:
        for d in range(A.shape[-1]):
            acc = fma32(A[..., :, None, d], B[..., None, :, d], acc)
    return acc


def top2(sim):
    """``(b1, i1, b2)`` along the last axis, whatever order the row is walked in."""
    sim = np.asarray(sim, F32)
    lead = sim.shape[:-1]
    if sim.shape[-1] == 0:
        return np.full(lead, NEG_INF), np.full(lead, -1, np.int32), np.full(lead, NEG_INF)
    cand = ~(np.isnan(sim) | (sim == NEG_INF))
    v = np.where(cand, sim, NEG_INF)
    b1 = v.max(-1)
    first = np.argmax(cand & (v == b1[..., None]), -1)               # the lowest index that attains b1
    i1 = np.where(cand.any(-1), first, -1).astype(np.int32)
    rest = v.copy()
    np.put_along_axis(rest, first[..., None], NEG_INF, -1)
    return b1, i1, rest.max(-1)


def squared_threshold(t):
    """``t * t`` formed in double and rounded once; ``None`` or 0: the test is off (the reference's ``if thresh:``)."""
    return F32(float(t) * float(t)) if t else None


def find_nn(sim, ratio_threshold=None, distance_threshold=None):
    """``(matches int32, scores float32)`` of every row of ``sim``: the reference's ``find_nn`` in float32."""
    b1, i1, b2 = top2(sim)
    r2, t2 = squared_threshold(ratio_threshold), squared_threshold(distance_threshold)
    with np.errstate(all='ignore'):
        d0 = F32(2) * (F32(1) - b1)
        d1 = F32(2) * (F32(1) - b2)
        mask = i1 >= 0
        if r2 is not None:
            mask = mask & (d0 <= r2 * d1)
        if t2 is not None:
            mask = mask & (d0 <= t2)
        score = (b1 + F32(1)) / F32(2)
    return np.where(mask, i1, -1).astype(np.int32), np.where(mask, score, F32(0)).astype(F32)


def mutual_check(m0, m1):
    """``m0[i]`` where ``m0[i] > -1`` and ``m1[m0[i]] == i``, else -1."""
    if m1.shape[-1] == 0 or m0.shape[-1] == 0:
        return np.full(m0.shape, -1, np.int32)
    loop = np.take_along_axis(m1, np.where(m0 > -1, m0, 0).astype(np.int64), -1)
    ok = (m0 > -1) & (loop == np.arange(m0.shape[-1]))
    return np.where(ok, m0, -1).astype(np.int32)


def match_similarity(sim, ratio_threshold=None, distance_threshold=None, do_mutual_check=True):
    """The matcher on a similarity ``[..., K0, K1]``: ``matches0``, ``matching_scores0`` (direction 0's scores BEFORE
    the mutual check, as the reference returns them), ``matches1`` (direction 1 after ``find_nn``) and the counters."""
    sim = np.asarray(sim, F32)
    m0, s0 = find_nn(sim, ratio_threshold, distance_threshold)
    m1, _ = find_nn(np.swapaxes(sim, -1, -2), ratio_threshold, distance_threshold)
    passed = (m0 > -1).sum(-1)
    if do_mutual_check:
        m0 = mutual_check(m0, m1)
    K0, K1 = sim.shape[-2:]
    counts = np.stack([np.full(passed.shape, K0), np.full(passed.shape, K1), passed, (m0 > -1).sum(-1)], -1)
    return dict(matches0=m0, matching_scores0=s0, matches1=m1, counts=counts.astype(np.int32))


def match_pair(A, B, ratio_threshold=None, distance_threshold=None, do_mutual_check=True):
    return match_similarity(similarity(A, B), ratio_threshold, distance_threshold, do_mutual_check)


def match_call(sims, n_kp0, n_kp1, off0, off1, ratio_threshold=None, distance_threshold=None, do_mutual_check=True,
               max_k0=None, max_k1=None):
    """What one device call returns, in its joined form.  ``sims[p]``: the similarity of pair ``p``, whose sides own
    rows ``off_i[p] .. off_i[p+1]-1``.  Rows no pair owns read -1 / 0; a pair beyond ``max_k0`` / ``max_k1`` (when
    given) is not matched: four -1 and its rows -1 / 0."""
    out = dict(matches0=np.full(n_kp0, -1, np.int32), matching_scores0=np.zeros(n_kp0, F32),
               matches1=np.full(n_kp1, -1, np.int32), counts=np.full((len(sims), COUNTERS), -1, np.int32))
    for p, sim in enumerate(sims):
        K0, K1 = sim.shape
        assert off0[p + 1] - off0[p] == K0 and off1[p + 1] - off1[p] == K1
        if (max_k0 is not None and K0 > max_k0) or (max_k1 is not None and K1 > max_k1):
            continue
        res = match_similarity(sim, ratio_threshold, distance_threshold, do_mutual_check)
        out['matches0'][off0[p]:off0[p + 1]] = res['matches0']
        out['matching_scores0'][off0[p]:off0[p + 1]] = res['matching_scores0']
        out['matches1'][off1[p]:off1[p + 1]] = res['matches1']
        out['counts'][p] = res['counts']
    return out
