"""The refit of a RANSAC pose on its inliers, as a float64 numpy program: the SPECIFICATION of
``oetr_pose_refit``.  It takes a model - the one ``oetr_pose_ransac`` selected, or any other - and the pair's match
list, and runs a FIXED number of least-squares rounds on the model's inliers; then it delivers exactly what
``pose_ransac_oracle.estimate`` delivers for a selected model.

Everything ``pose_ransac_oracle`` (``pro``) and ``homography_ransac_oracle`` (``hro``) state is taken from there:
the normalisation, Sampson's test, the decomposition, the cheirality votes and the cosines from ``pro``; the summation
order (``hro.tree_sum``: 256 partial sums by list position, one fixed tree) from ``hro``.  Stated here: the 44 sums of
the moment matrix, the held entry, the 8 x 9 system, its elimination on a general matrix (``pro.solve``'s and
``hro.solve8``'s pivot rule), the candidate's scaling, the acceptance rule.

It is THE PROJECT'S OWN STATEMENT: float64, elementwise ``+ - * /``, ``sqrt`` and comparisons only, a fixed operation
order, no BLAS or LAPACK.  No parity with ``cv2`` is claimed.  Not done, on purpose: Hartley normalisation, a
projection onto the essential manifold before scoring (``pro.decompose`` ignores the singular values), a second
threshold, non-linear minimisation, adaptive termination.

One round, from the current model ``F`` with ``count`` inliers over ALL rows of the list:
  1. the inlier rows of ``F``; fewer than 8: stop;
  2. per row ``w = (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1)``, the six products rounded on their own;
  3. the upper triangle of ``M = sum w w^T``: 36 sums of products (each product rounded on its own), 8 sums of a
     ``w_i``, and ``M[8][8]`` the count as an exact integer converted once - 44 floating-point sums;
  4. every sum in ``hro``'s order: partial ``c`` adds the terms of the inlier rows at list positions ``c`` modulo 256,
     ascending, from 0.0; then ``hro.tree_sum``;
  5. the held entry ``k``: the entry of ``F`` of largest ``abs``, the lowest index on a tie;
  6. the 8 x 9 system: rows and columns of ``M`` without ``k``, right-hand side ``-M[:, k]``;
  7. Gauss-Jordan with partial pivoting by comparisons of ``abs``, the lowest row on a tie; a zero or NaN pivot: no
     candidate, stop;
  8. the candidate: the eight solutions with 1 at ``k``, times ``1 / sqrt(sum of squares, added in entry order)``;
     no sign rule (``pro.candidates`` covers both signs);
  9. the candidate's count over ALL rows;
  10. accepted iff every entry is finite and its count ``>= count``; otherwise the current model stays and the rounds
      stop.  The delivered model never has fewer inliers than ``model_in``.
"""
import numpy as np

import homography_ransac_oracle as hro
import pose_ransac_oracle as pro

TERMS = 44                       # floating-point sums of one round
PRODUCTS = 36                    # of them, sums of products: the upper triangle of the leading 8 x 8
MIN_ROWS = 8                     # a round needs that many inlier rows
MAX_REFIT, DEFAULT_REFIT = 8, 4
COUNTERS = 5                     # list length, inliers of model_in, rounds accepted or -1, inliers delivered, votes
CLASSES = hro.CLASSES


# ------------------------------------------------------------------ the sums
def row_terms(x1, y1, x2, y2):
    """The 44 terms one row adds: ``w_i * w_j`` for ``i <= j < 8`` in row-major order of the upper triangle, then
    ``w_0 .. w_7``."""
    w = [x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1]
    return [w[i] * w[j] for i in range(8) for j in range(i, 8)] + w


def moment_index(i, j):
    """Where ``M[i][j]`` lives among the sums; ``TERMS`` for ``M[8][8]``, the count."""
    i, j = min(i, j), max(i, j)
    if j == 8:
        return TERMS if i == 8 else PRODUCTS + i
    return (8 * i - (i * (i - 1)) // 2) + (j - i)


def moment_sums(x1, y1, x2, y2, inl):
    """The 44 sums over the inlier rows ``inl`` (bool ``[m]``) of one list, in ``hro``'s order."""
    m = len(x1)
    rounds = (m + CLASSES - 1) // CLASSES
    with np.errstate(all='ignore'):
        terms = np.zeros((TERMS, rounds * CLASSES))
        terms[:, :m] = np.stack(row_terms(x1, y1, x2, y2))
        terms = terms.reshape(TERMS, rounds, CLASSES)
        use = np.zeros(rounds * CLASSES, bool)
        use[:m] = inl
        use = use.reshape(rounds, CLASSES)
        partial = np.zeros((TERMS, CLASSES))
        for r in range(rounds):                                   # a row that is no inlier is SKIPPED, not added as 0.0
            partial = np.where(use[r][None, :], partial + terms[:, r, :], partial)
    return [hro.tree_sum(partial[k]) for k in range(TERMS)]


# ------------------------------------------------------------------ the system
def held_entry(F):
    """The entry of largest ``abs``, the lowest index on a tie."""
    best, k = np.abs(F[0]), 0
    for i in range(1, 9):
        if np.abs(F[i]) > best:
            best, k = np.abs(F[i]), i
    return k


def system(S, n, k):
    """The augmented 8 x 9 system: rows and columns of ``M`` without ``k``, right-hand side ``-M[:, k]``."""
    val = lambda i, j: np.float64(n) if moment_index(i, j) == TERMS else np.float64(S[moment_index(i, j)])
    keep = [i for i in range(9) if i != k]
    return [[val(i, j) for j in keep] + [-val(i, k)] for i in keep]


def eliminate(A):
    """Gauss-Jordan with partial pivoting on an 8 x 9 system (``pro.solve``'s rule) -> the 8 unknowns, or None for a
    zero or NaN pivot."""
    A = [[np.float64(v) for v in row] for row in A]
    with np.errstate(all='ignore'):
        for c in range(8):
            best, piv = np.abs(A[c][c]), c
            for r in range(c + 1, 8):
                if np.abs(A[r][c]) > best:
                    best, piv = np.abs(A[r][c]), r
            if not best > 0.0:
                return None
            A[c], A[piv] = A[piv], A[c]
            d = A[c][c]
            for j in range(c + 1, 9):
                A[c][j] = A[c][j] / d
            for r in range(8):
                if r == c:
                    continue
                f = A[r][c]
                for j in range(c + 1, 9):
                    A[r][j] = A[r][j] - f * A[c][j]
    return [A[r][8] for r in range(8)]


def scaled(sol, k):
    """The eight solutions with 1 at ``k``, of unit norm: the squares added in entry order."""
    cand = [np.float64(v) for v in sol[:k]] + [np.float64(1.0)] + [np.float64(v) for v in sol[k:]]
    with np.errstate(all='ignore'):
        ss = cand[0] * cand[0]
        for i in range(1, 9):
            ss = ss + cand[i] * cand[i]
        scale = 1.0 / np.sqrt(ss)
        return np.array([v * scale for v in cand])


def refit_candidate(F, x1, y1, x2, y2, inl):
    """One round's candidate from the inlier rows ``inl`` of ``F``: float64 [9] (possibly non-finite), or None (fewer
    than 8 rows, or a zero pivot)."""
    n = int(inl.sum())
    if n < MIN_ROWS:
        return None
    k = held_entry(F)
    sol = eliminate(system(moment_sums(x1, y1, x2, y2, inl), n, k))
    return None if sol is None else scaled(sol, k)


# ------------------------------------------------------------------ one pair
def _threshold_margin(lhs, rhs):
    with np.errstate(all='ignore'):
        dec = np.isfinite(lhs) & np.isfinite(rhs) & (rhs > 0)
        return float((np.abs(lhs - rhs)[dec] / rhs[dec]).min()) if dec.any() else np.inf


def refit(P, k1, k2, model_in, px_thr=1.0, refit_iters=DEFAULT_REFIT):
    """One pair -> dict(model [9], pose [12], cosines [2], counts int32 [5], inliers uint8 [m], candidates (every
    round's candidate, in order), candidate_counts, margins)."""
    if not 0 <= int(refit_iters) <= MAX_REFIT:
        raise ValueError(f'refit_iters must be in 0..{MAX_REFIT}')
    k1, k2 = np.asarray(k1, np.float32).reshape(-1, 2), np.asarray(k2, np.float32).reshape(-1, 2)
    m = len(k1)
    F = np.asarray(model_in, np.float64).reshape(9).copy()
    res = dict(model=np.full(9, np.nan), pose=np.full(12, np.nan), cosines=np.full(2, np.nan),
               inliers=np.zeros(m, np.uint8), counts=np.array([m, 0, -1, 0, 0], np.int32), candidates=[],
               candidate_counts=[], margins={})
    if m == 0 or not np.isfinite(F).all():
        return res
    x1, y1, x2, y2, thr_sq = pro.normalise(P, k1, k2, px_thr)
    table, lhs, rhs = pro.inlier_table(F, x1, y1, x2, y2, thr_sq)
    inl, thr_margin = table[0], _threshold_margin(lhs[0], rhs[0])
    count_in = count = int(inl.sum())
    accepted = 0
    for _ in range(int(refit_iters)):                             # fixed: nothing iterates on data
        cand = refit_candidate(F, x1, y1, x2, y2, inl)
        if cand is None:
            break
        res['candidates'].append(cand)
        if not np.isfinite(cand).all():
            res['candidate_counts'].append(-1)
            break
        t, l, r = pro.inlier_table(cand, x1, y1, x2, y2, thr_sq)
        thr_margin = min(thr_margin, _threshold_margin(l[0], r[0]))
        c = int(t[0].sum())
        res['candidate_counts'].append(c)
        if c < count:
            break
        F, inl, count, accepted = cand, t[0], c, accepted + 1
    # what pro.estimate does after select
    R1, R2, t = pro.decompose(F)
    votes, depth_margin = pro.cheirality(R1, R2, t, *(a[inl] for a in (x1, y1, x2, y2)))
    chosen = int(np.argmax(votes))                                # the lowest number on a tie
    R, tc = pro.candidates(R1, R2, t)[chosen]
    res.update(model=F.copy(), pose=np.concatenate([R, tc]), cosines=pro.cosines(P, R, tc),
               inliers=inl.astype(np.uint8), counts=np.array([m, count_in, accepted, count, votes[chosen]], np.int32),
               margins=dict(threshold=thr_margin, depth=depth_margin, votes=[int(v) for v in votes]))
    return res


margins_hold = pro.margins_hold


def refit_lists(blocks, lists, models, px_thr=1.0, refit_iters=DEFAULT_REFIT):
    return [refit(blocks[p], k1, k2, models[p], px_thr, refit_iters) for p, (k1, k2) in enumerate(lists)]


def error_of(res):
    return float(pro.pose_errors(res['cosines'][None], res['counts'][None])[2][0])


def list_record(res):
    """One refitted pair as JSON-able recorded values: counters, values by hash (16 hex digits), margins."""
    sha, z = (lambda a: pro.mso.cvo.sha(a)[:16]), (lambda a: np.nan_to_num(np.asarray(a, np.float64), nan=-7.0))
    return dict(counts=[int(c) for c in res['counts']], model=sha(z(res['model'])), pose=sha(z(res['pose'])),
                cosines=sha(z(res['cosines'])), inliers=sha(res['inliers']),
                candidates=sha(z(np.array(res['candidates']).reshape(-1, 9))),
                candidate_counts=[int(c) for c in res['candidate_counts']],
                margins={k: v for k, v in res['margins'].items()})


# ------------------------------------------------------------------ the pinned call
# 16 lists in ONE call: the lengths straddle the 8-row minimum, a wave (64) and the 256 partial sums; the last five
# carry up to 1 px noise, 60 % outliers and duplicated rows.  (length, noise px, outlier share, duplicates)
PINNED = ((0, 0.3, 0.2, 0), (7, 0.0, 0.0, 0), (8, 0.0, 0.0, 0), (9, 0.3, 0.0, 0), (63, 0.3, 0.2, 0), (64, 0.0, 0.0, 0),
          (65, 0.3, 0.2, 0), (255, 0.3, 0.2, 0), (256, 0.3, 0.2, 0), (257, 0.3, 0.2, 0), (600, 0.3, 0.2, 0),
          (300, 0.5, 0.3, 0), (120, 0.5, 0.6, 4), (1000, 0.5, 0.6, 0), (40, 1.0, 0.3, 10), (513, 0.5, 0.5, 0))
PINNED_HYPOTHESES = 85
PINNED_SEED = pro.PINNED_SEED
PINNED_REFITS = (0, 1, 2, 4)
PINNED_SOURCES = ('estimate', 'true')
MAX_DRAWS = pro.MAX_DRAWS


def pinned_list(p, draw=0):
    """List p of the pinned call in its ``draw``-th drawing -> ``(P, k1, k2)``."""
    n, noise, outliers, dup = PINNED[p]
    P, k1, k2, _ = pro.make_scene(max(n, 1), seed=7000 + 100 * p + draw, noise=noise, outliers=outliers, duplicates=dup)
    return P, k1[:n], k2[:n]


def pinned_models(P, k1, k2, p):
    """``model_in`` of list p from the two sources: ``pro.estimate``'s selected model, the true essential matrix."""
    est = pro.estimate(P, k1, k2, PINNED_HYPOTHESES, PINNED_SEED, 1.0, p)
    return dict(estimate=est['model'], true=pro.true_essential(P)), est


def pinned_call(draws=None):
    """-> ``(blocks [16,20], lists, models {source: [16,9]}, draws)``.  ``draws`` None: every list is re-drawn until
    the margins of the estimate and of every refit hold (at most MAX_DRAWS times); otherwise the recorded draws are
    used as they are."""
    blocks, lists, used = [], [], []
    models = {s: [] for s in PINNED_SOURCES}
    for p in range(len(PINNED)):
        tries = range(MAX_DRAWS) if draws is None else [draws[p]]
        for d in tries:
            P, k1, k2 = pinned_list(p, d)
            M, est = pinned_models(P, k1, k2, p)
            if draws is not None or (pro.margins_hold(est) and all(
                    margins_hold(refit(P, k1, k2, M[s], 1.0, r)) for s in PINNED_SOURCES for r in PINNED_REFITS)):
                break
        else:
            raise AssertionError(f'list {p}: no drawing with margins in {MAX_DRAWS}')
        blocks.append(P), lists.append((k1, k2)), used.append(d)
        for s in PINNED_SOURCES:
            models[s].append(M[s])
    return np.stack(blocks), lists, {s: np.stack(v) for s, v in models.items()}, used


# ------------------------------------------------------------------ the scenes of the CPU tests
NOISE_FREE = dict(scenes=pro.NOISE_FREE_SCENES, n=200, outliers=0.5, px_thr=0.01, n_hyp=1024, seed=1)
NOISY = dict(n=pro.NOISY['n'], noise=pro.NOISY['noise'], n_hyp=1024, px_thr=1.0, seed=pro.NOISY['seed'])
NOISY_REFITS = (0, 1, 2, 4)


def noise_free_result(i, refit_iters=DEFAULT_REFIT):
    """Scene i (200 rows, 50 % outliers, px_thr 0.01) -> (``pro.estimate``'s result, its refit)."""
    c = NOISE_FREE
    P, k1, k2, _ = pro.make_scene(c['n'], seed=1000 + 20 * i, outliers=c['outliers'])
    est = pro.estimate(P, k1, k2, c['n_hyp'], c['seed'], c['px_thr'], i)
    return est, refit(P, k1, k2, est['model'], c['px_thr'], refit_iters)


def noisy_results(i, share):
    """A noisy scene of ``pro`` at px_thr 1 -> (``pro.estimate``'s result, {refit_iters: refit}, the inliers of the
    true essential matrix under the same test)."""
    c = NOISY
    P, k1, k2 = pro.noisy_scene(i, share)
    est = pro.estimate(P, k1, k2, c['n_hyp'], c['seed'], c['px_thr'], i)
    x1, y1, x2, y2, thr_sq = pro.normalise(P, k1, k2, c['px_thr'])
    true_inliers = int(pro.score_models(pro.true_essential(P), x1, y1, x2, y2, thr_sq)[0])
    return est, {r: refit(P, k1, k2, est['model'], c['px_thr'], r) for r in NOISY_REFITS}, true_inliers


# ------------------------------------------------------------------ refusals and edges
REJECTED_SEED, REJECTED_THR = 2, 1.0


def exact_essential():
    """The true essential matrix of ``pro.EXACT_BLOCK`` (R = I, t = (1, 0, 0)): ``y2 = y1``.  Entries 5 and 7 tie in
    ``abs``."""
    return np.array([0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0])


def exact_scene(n=40, seed=3):
    """``n`` matches under ``pro.EXACT_BLOCK``: a horizontal disparity of ``512 / z`` px, 0.2 px noise on ``v2``."""
    rng = np.random.default_rng(seed)
    u, v, z = rng.uniform(0, 500, n), rng.uniform(0, 479, n), rng.uniform(4.0, 12.0, n)
    k1 = np.stack([u, v], 1).astype(np.float32)
    k2 = np.stack([u + 512.0 / z, v + 0.2 * rng.standard_normal(n)], 1).astype(np.float32)
    return pro.EXACT_BLOCK.copy(), k1, k2


def rejected_list(seed=REJECTED_SEED):
    return pro.make_scene(40, seed=9000 + seed, noise=0.5, outliers=0.2)[:3]


def edge_cases():
    """name -> ``(P, k1, k2, model_in, px_thr)``, every ``px_thr`` 1: the cases fit one call.
    ``few``: a model with fewer than 8 inliers: no round, the model is delivered as it is.
    ``zero_pivot``: every ``x1 == 0`` exactly (``pro.EXACT_BLOCK``): whole columns of ``M`` are zero and the held entry
    is none of them - an EXACT zero pivot, no candidate.
    ``rejected``: a finite candidate with fewer inliers than the current model: the model stays, the rounds stop.
    ``nan``: a NaN ``model_in``.  ``empty``: a list of 0 rows.
    ``tie``: ``abs`` of entries 5 and 7 equal and largest: entry 5 is held."""
    P, k1, k2 = pro.noise_free_scene(0)
    E = pro.unit(pro.true_essential(P))
    Pe, on_axis, _ = pro.degenerate_lists()['collinear_exact']
    Pr, r1, r2 = rejected_list()
    return dict(few=(P, k1[:7], k2[:7], E, 1.0),
                zero_pivot=(Pe, on_axis, on_axis.copy(), exact_essential(), 1.0),     # every row: s == 0 exactly
                rejected=(Pr, r1, r2, pro.unit(pro.true_essential(Pr)), REJECTED_THR),
                nan=(P, k1[:20], k2[:20], np.where(np.arange(9) == 4, np.nan, E), 1.0),
                empty=(P, k1[:0], k2[:0], E, 1.0),
                tie=exact_scene() + (exact_essential(), 1.0))
