"""The pinned inputs of the nearest-neighbour matcher's tests (CPU and GPU), seeded, with the specification's
similarities computed once per call and shared.

Two kinds of descriptors:

* ``unit``: the rows of a Gaussian, normalised; half of side 0's rows get a planted partner - a side-1 row plus Gaussian
  noise of relative size 0.01 - 0.08, normalised again - so every threshold branch is taken decisively;
* ``grid``: entries ``k / 64`` with integer ``|k| <= 8``: every partial sum is exact in float32 for ``D <= 512``, so
  ANY summation order gives the same similarity; planted partners (a side-1 row with six entries redrawn) and
  deliberate duplicates (at most 8 rows per call and side, in the pairs with ``K0 >= 128``) pin ties and the mutual
  check under ties.

The shapes are the smallest that cross every tile edge of the kernel (64 query rows, 128 key rows, 64 columns of D).
"""
import functools
import hashlib

import numpy as np

import nn_match_oracle as nmo

F32 = np.float32
K_EDGES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 300)
# name -> (D, the pairs' (K0, K1)); every K of K_EDGES stands on both sides of 'ragged128', with K0 = 0, K1 = 0 and K1 = 1
SHAPES = {
    'ragged128': (128, ((0, 33), (31, 0), (65, 1), (1, 64), (2, 2), (32, 31), (33, 63), (63, 32), (64, 65), (127, 129),
                        (129, 127), (300, 300))),
    'wide256': (256, ((300, 257), (128, 200), (65, 300), (200, 129))),
    'd4': (4, ((65, 33), (3, 64), (64, 65))),
    'd512': (512, ((65, 64), (33, 65), (17, 5))),
}
KINDS = ('unit', 'grid')
CALLS = tuple((name, kind) for name in SHAPES for kind in KINDS)
# (ratio_threshold, distance_threshold), each with the mutual check on and off
THRESHOLDS = ((None, None), (0.8, None), (None, 0.7), (0.8, 0.7))
SETTINGS = tuple((r, t, mutual) for r, t in THRESHOLDS for mutual in (True, False))
MAX_DUPLICATES = 8
DUPLICATE_MIN_K0 = 128


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _normalised(x):
    return (x / np.linalg.norm(x.astype(np.float64), axis=-1, keepdims=True)).astype(F32)


def unit_pair(rng, K0, K1, D):
    B = _normalised(rng.standard_normal((K1, D)))
    A = _normalised(rng.standard_normal((K0, D)))
    if K0 and K1:
        rows = rng.permutation(K0)[:K0 // 2]
        partners = rng.integers(0, K1, len(rows))
        noise = rng.standard_normal((len(rows), D)) / np.sqrt(D) * rng.uniform(0.01, 0.08, (len(rows), 1))
        A[rows] = _normalised(B[partners] + noise)
    return A, B


def grid_pair(rng, K0, K1, D, budget):
    """``budget``: [duplicates left for side 0, for side 1] of the call, used up by the pairs with ``K0 >= 128``."""
    A = (rng.integers(-8, 9, (K0, D)) / 64).astype(F32)
    B = (rng.integers(-8, 9, (K1, D)) / 64).astype(F32)
    if K0 and K1:
        rows = rng.permutation(K0)[:K0 // 2]
        partners = rng.integers(0, K1, len(rows))
        A[rows] = B[partners]
        for r in rows:
            cols = rng.permutation(D)[:6]
            A[r, cols] = (rng.integers(-8, 9, len(cols)) / 64).astype(F32)
    if K0 >= DUPLICATE_MIN_K0 and K1 >= 2:
        for side, X in enumerate((A, B)):
            n = min(budget[side], 4, len(X) // 2)
            picks = rng.permutation(len(X))[:2 * n]
            X[picks[:n]] = X[picks[n:]]
            budget[side] -= n
    return A, B


@functools.lru_cache(maxsize=None)
def make_call(name, kind):
    """One call: descriptors joined per side, their offsets, and the specification's similarity of every pair."""
    D, pairs = SHAPES[name]
    rng = np.random.default_rng([sorted(SHAPES).index(name), KINDS.index(kind), 20250])
    budget = [MAX_DUPLICATES, MAX_DUPLICATES]
    sides = [unit_pair(rng, K0, K1, D) if kind == 'unit' else grid_pair(rng, K0, K1, D, budget) for K0, K1 in pairs]
    desc0 = np.concatenate([a for a, _ in sides]).astype(F32).reshape(-1, D)
    desc1 = np.concatenate([b for _, b in sides]).astype(F32).reshape(-1, D)
    off0 = np.concatenate([[0], np.cumsum([K0 for K0, _ in pairs])]).astype(np.int32)
    off1 = np.concatenate([[0], np.cumsum([K1 for _, K1 in pairs])]).astype(np.int32)
    sims = [nmo.similarity(a, b) for a, b in sides]
    for x in (desc0, desc1, off0, off1, *sims):
        x.setflags(write=False)
    return dict(name=name, kind=kind, D=D, pairs=pairs, desc0=desc0, desc1=desc1, off0=off0, off1=off1, sims=sims,
                max_k0=max(K0 for K0, _ in pairs), max_k1=max(K1 for _, K1 in pairs))


def expected(call, ratio_threshold, distance_threshold, do_mutual_check, **kw):
    return nmo.match_call(call['sims'], len(call['desc0']), len(call['desc1']), call['off0'], call['off1'],
                          ratio_threshold, distance_threshold, do_mutual_check, **kw)


def setting_key(ratio_threshold, distance_threshold, do_mutual_check):
    return f'ratio={ratio_threshold} distance={distance_threshold} mutual={int(do_mutual_check)}'


def result_record(res):
    """What the fixture keeps of one result: the counters and a hash of every output."""
    return dict(counts=res['counts'].tolist(), matches0=sha(res['matches0']),
                matching_scores0=sha(res['matching_scores0'].view(np.uint32)), matches1=sha(res['matches1']))


def many_small_pairs(n_pairs=65538, seed=7):
    """More pairs than one grid dimension holds (65 535): ``K0, K1`` in {2, 3}, ``D = 4``, unit-norm descriptors, and
    the specification's result, computed shape by shape in batches."""
    rng = np.random.default_rng(seed)
    K0 = rng.integers(2, 4, n_pairs)
    K1 = rng.integers(2, 4, n_pairs)
    off0 = np.concatenate([[0], np.cumsum(K0)]).astype(np.int32)
    off1 = np.concatenate([[0], np.cumsum(K1)]).astype(np.int32)
    desc0 = _normalised(rng.standard_normal((off0[-1], 4)))
    desc1 = _normalised(rng.standard_normal((off1[-1], 4)))
    settings = dict(ratio_threshold=0.8, distance_threshold=None, do_mutual_check=True)
    out = dict(matches0=np.full(off0[-1], -1, np.int32), matching_scores0=np.zeros(off0[-1], F32),
               matches1=np.full(off1[-1], -1, np.int32), counts=np.zeros((n_pairs, nmo.COUNTERS), np.int32))
    for k0 in (2, 3):
        for k1 in (2, 3):
            sel = np.nonzero((K0 == k0) & (K1 == k1))[0]
            r0 = off0[sel, None] + np.arange(k0)
            r1 = off1[sel, None] + np.arange(k1)
            res = nmo.match_similarity(nmo.similarity(desc0[r0], desc1[r1]), **settings)
            out['matches0'][r0], out['matching_scores0'][r0] = res['matches0'], res['matching_scores0']
            out['matches1'][r1], out['counts'][sel] = res['matches1'], res['counts']
    return dict(desc0=desc0, desc1=desc1, off0=off0, off1=off1, D=4, max_k0=3, max_k1=3, settings=settings,
                expected=out)
