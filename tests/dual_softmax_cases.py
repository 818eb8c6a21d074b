"""The pinned inputs of the dual-softmax matcher's tests (CPU and GPU), seeded, with the specification's ``t`` computed
once per call and setting and shared.

Two kinds of features, the idea of ``nn_match_cases``:

* ``gauss``: unit-variance Gaussian rows; half of side 0's tokens get a planted partner - a side-1 row plus Gaussian noise
  of relative size 0.05 - 0.3 - so at temperature 0.1 the planted confidences clear the threshold decisively and at
  temperature 1 none does;
* ``grid``: entries ``k / 4`` with integer ``|k| <= 8``: every partial sum of a similarity is exact in float32 for
  ``D <= 512``, so equal rows give EQUAL similarities; planted partners (a side-1 row with six entries redrawn) and
  deliberate duplicates on both sides pin maxima that tie in both directions.

The token counts are the smallest that cross every tile edge of the kernel (64 query rows, 128 key rows, 64 columns of
D), each with a grid that multiplies to it.
"""
import functools
import hashlib

import numpy as np

import dual_softmax_oracle as dso
import nn_match_oracle as nmo

F32 = np.float32
# a grid for every token count of the tests
GRID_OF = {0: (0, 3), 1: (1, 1), 9: (3, 3), 20: (4, 5), 25: (5, 5), 33: (3, 11), 63: (7, 9), 64: (8, 8), 65: (5, 13),
           127: (1, 127), 128: (8, 16), 129: (3, 43), 300: (15, 20)}
# name -> (D, the pairs' (L, S))
SHAPES = {
    'ragged64': (64, ((0, 65), (63, 0), (1, 64), (64, 1), (65, 63), (127, 129), (128, 127), (129, 128), (300, 300),
                      (63, 300))),
    'borders': (64, ((1, 1), (9, 9), (9, 20), (20, 25), (25, 25), (25, 1), (300, 25))),
    'd4': (4, ((65, 33), (9, 64))),
    'd68': (68, ((65, 129), (128, 33))),
    'd256': (256, ((300, 129), (128, 65))),
    'd512': (512, ((65, 64), (9, 25))),
}
KINDS = ('gauss', 'grid')
CALLS = tuple((name, kind) for name in SHAPES for kind in KINDS)
# (temperature, threshold, border_rm): both temperatures, both thresholds, every border
SETTINGS = ((0.1, 0.2, 2), (0.1, 0.0, 0), (1.0, 0.0, 1), (1.0, 0.2, 0))
CELL = 8
DUPLICATE_MIN = 20


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def gauss_pair(rng, L, S, D):
    B = rng.standard_normal((S, D)).astype(F32)
    A = rng.standard_normal((L, D)).astype(F32)
    if L and S:
        rows = rng.permutation(L)[:(L + 1) // 2]
        partners = rng.permutation(S)[:len(rows)]
        rows = rows[:len(partners)]
        noise = rng.standard_normal((len(rows), D)) * rng.uniform(0.05, 0.3, (len(rows), 1))
        A[rows] = (B[partners] + noise).astype(F32)
    return A, B


def grid_pair(rng, L, S, D):
    A = (rng.integers(-8, 9, (L, D)) / 4).astype(F32)
    B = (rng.integers(-8, 9, (S, D)) / 4).astype(F32)
    if L and S:
        rows = rng.permutation(L)[:(L + 1) // 2]
        partners = rng.integers(0, S, len(rows))
        A[rows] = B[partners]
        for r in rows[::2]:
            cols = rng.permutation(D)[:min(6, D)]
            A[r, cols] = (rng.integers(-8, 9, len(cols)) / 4).astype(F32)
    if L >= DUPLICATE_MIN and S >= DUPLICATE_MIN:                      # equal tokens: maxima tie in both directions
        for X in (A, B):
            picks = rng.permutation(len(X))[:8]
            X[picks[:4]] = X[picks[4:]]
    return A, B


def join(sides, D):
    feat0 = np.concatenate([a for a, _ in sides]).astype(F32).reshape(-1, D)
    feat1 = np.concatenate([b for _, b in sides]).astype(F32).reshape(-1, D)
    off0 = np.concatenate([[0], np.cumsum([len(a) for a, _ in sides])]).astype(np.int32)
    off1 = np.concatenate([[0], np.cumsum([len(b) for _, b in sides])]).astype(np.int32)
    return feat0, feat1, off0, off1


@functools.lru_cache(maxsize=None)
def make_call(name, kind):
    """One call: features joined per side, offsets, grids and the specification's similarity of every pair."""
    D, pairs = SHAPES[name]
    rng = np.random.default_rng([sorted(SHAPES).index(name), KINDS.index(kind), 20260])
    sides = [gauss_pair(rng, L, S, D) if kind == 'gauss' else grid_pair(rng, L, S, D) for L, S in pairs]
    feat0, feat1, off0, off1 = join(sides, D)
    grids0 = np.array([GRID_OF[L] for L, _ in pairs], np.int32)
    grids1 = np.array([GRID_OF[S] for _, S in pairs], np.int32)
    sims = [nmo.similarity(a, b) for a, b in sides]
    for x in (feat0, feat1, off0, off1, grids0, grids1, *sims):
        x.setflags(write=False)
    return dict(name=name, kind=kind, D=D, pairs=pairs, feat0=feat0, feat1=feat1, off0=off0, off1=off1, grids0=grids0,
                grids1=grids1, sims=sims, max_k0=max(L for L, _ in pairs), max_k1=max(S for _, S in pairs))


def ts_of(call, temperature):
    scale = dso.scale_of(call['D'], temperature)
    return [(s * scale).astype(F32) for s in call['sims']]


@functools.lru_cache(maxsize=None)
def _expected(name, kind, temperature, threshold, border_rm):
    call = make_call(name, kind)
    return dso.match_call(ts_of(call, temperature), call['grids0'], call['grids1'], len(call['feat0']),
                          len(call['feat1']), call['off0'], call['off1'], threshold, border_rm, CELL)


def expected(call, temperature, threshold, border_rm):
    """The specification's result of a pinned call (cached: shared, never modified)."""
    return _expected(call['name'], call['kind'], temperature, threshold, border_rm)


def setting_key(temperature, threshold, border_rm):
    return f'temperature={temperature} threshold={threshold} border_rm={border_rm}'


def result_record(res):
    """What the fixture keeps of one result: the counters and a hash of every output."""
    return dict(counts=res['counts'].tolist(), matches0=sha(res['matches0']),
                matching_scores0=sha(res['matching_scores0'].view(np.uint32)), matches1=sha(res['matches1']),
                keypoints0=sha(res['keypoints0'].view(np.uint32)), keypoints1=sha(res['keypoints1'].view(np.uint32)))


# ------------------------------------------------------------------ the calls held against the float64 head
# (L, S, D, temperature, threshold, border_rm); the generator draws seeds until the float64 program's own margins hold
HEAD_SHAPES = ((300, 300, 64, 0.1, 0.2, 2), (129, 65, 256, 0.1, 0.2, 1), (65, 128, 68, 0.1, 0.0, 0),
               (64, 63, 512, 1.0, 0.0, 1), (25, 20, 4, 1.0, 0.2, 0), (128, 300, 128, 0.1, 0.2, 2))
HEAD_MARGIN = 1e-3


def head_pair(k, seed):
    L, S, D = HEAD_SHAPES[k][:3]
    return gauss_pair(np.random.default_rng([k, seed, 977]), L, S, D)


def head_compare(k, seed):
    """The specification against the float64 head on one drawn call: the float64 program's smallest margin, whether
    ``matches0`` and the last two counters are EQUAL on every row, and the error of the confidences - relative where the
    float64 confidence is at least :data:`HEAD_REL_FLOOR`, absolute everywhere (no candidate counts as 0)."""
    L, S, D, temperature, threshold, border_rm = HEAD_SHAPES[k]
    A, B = head_pair(k, seed)
    g0, g1 = GRID_OF[L], GRID_OF[S]
    ref = dso.published_head(A, B, g0, g1, temperature, threshold, border_rm)
    t = (nmo.similarity(A, B) * dso.scale_of(D, temperature)).astype(F32)
    spec = dso.match_t(t, g0, g1, threshold, border_rm)
    conf, cand = dso.confidence(t)
    conf = np.where(cand, conf, 0).astype(np.float64)
    err = np.abs(conf - ref['conf'])
    big = ref['conf'] >= HEAD_REL_FLOOR
    return dict(margin=ref['margin'], matched=ref['kept'],
                equal=bool(np.array_equal(spec['matches0'], ref['matches0'])
                           and spec['counts'][2:].tolist() == [ref['over'], ref['kept']]),
                conf_rel_err=float((err[big] / ref['conf'][big]).max()), conf_abs_err=float(err.max()))


HEAD_REL_FLOOR = 1e-6


def e_sweep():
    """The arguments ``e`` is measured on: a dense sweep of ``[cut-off, 0]``, the neighbours of the cut-off and of 0,
    and a sweep beyond the cut-off with -inf."""
    inside = np.concatenate([np.linspace(-87.0, 0.0, 2_000_001), -np.logspace(-45, 1.9, 20_001)]).astype(F32)
    edge = np.array([-87.0, np.nextafter(F32(-87), F32(0)), -0.0, 0.0, -np.finfo(F32).tiny], F32)
    inside = np.concatenate([inside[inside >= F32(-87)], edge])
    beyond = np.concatenate([np.linspace(-1000.0, -87.0, 20_001)[:-1], [np.nextafter(F32(-87), F32(-np.inf)), -3e38,
                                                                         -np.inf]]).astype(F32)
    return inside, beyond[beyond < F32(-87)]


def e_error(inside):
    """The largest relative error of ``e`` against float64 ``np.exp`` on ``inside``."""
    ref = np.exp(inside.astype(np.float64))
    return float((np.abs(dso.e32(inside).astype(np.float64) - ref) / ref).max())


# ------------------------------------------------------------------ special calls of the GPU tests
def all_equal_call(L=63, S=20, D=64):
    """Every token equal: every confidence is ``1 / (L * S)`` up to the specification's roundings."""
    A, B = np.full((L, D), 0.5, F32), np.full((S, D), 0.5, F32)
    return A, B, GRID_OF[L], GRID_OF[S]


def cutoff_pair(seed=5, L=65, S=129, D=64):
    """Features scaled so that ``t - m`` runs from 0 far past the cut-off of ``e`` (-87) within the rows: planted
    partners at ``t`` of a few hundred, the rest spread over hundreds on either side of 0."""
    rng = np.random.default_rng(seed)
    A, B = gauss_pair(rng, L, S, D)
    return (A * F32(6)).astype(F32), (B * F32(6)).astype(F32), GRID_OF[L], GRID_OF[S]


def many_small_pairs(n_pairs=65538, seed=7):
    """More pairs than one grid dimension holds (65 535): 2 x 2 grids on both sides, ``D = 4``, and the specification's
    result, computed in one batch."""
    rng = np.random.default_rng(seed)
    feat0 = rng.standard_normal((n_pairs, 4, 4)).astype(F32)
    feat1 = rng.standard_normal((n_pairs, 4, 4)).astype(F32)
    feat0[::3, :2] = feat1[::3, 2:]                                   # partners that clear the threshold
    settings = dict(temperature=0.1, threshold=0.2, border_rm=0)
    t = (nmo.similarity(feat0, feat1) * dso.scale_of(4, 0.1)).astype(F32)
    res = dso.match_t(t, (2, 2), (2, 2), 0.2, 0)
    kp = np.tile(dso.keypoints(2, 2, CELL), (n_pairs, 1))
    off = (np.arange(n_pairs + 1) * 4).astype(np.int32)
    out = dict(matches0=res['matches0'].reshape(-1), matching_scores0=res['matching_scores0'].reshape(-1),
               matches1=res['matches1'].reshape(-1), keypoints0=kp, keypoints1=kp.copy(), counts=res['counts'])
    return dict(feat0=feat0.reshape(-1, 4), feat1=feat1.reshape(-1, 4), off0=off, off1=off.copy(),
                grids=np.tile(np.array([[2, 2]], np.int32), (n_pairs, 1)), D=4, max_k0=4, max_k1=4, settings=settings,
                expected=out)
