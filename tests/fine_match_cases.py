"""The drawn calls the fine-match tests share (``tests/test_fine_match_cpu.py``, ``tests/test_gpu_fine_match.py``,
``tools/gen_golden_fine_match.py``): coarse match results in the joined form ``match_dense`` leaves, fine maps as joined
token rows, and what the specification ``tests/fine_match_oracle.py`` makes of them.  numpy only.

A pair is ``(g0, g1, kind, cut0, cut1)``: the coarse grids of the two sides, how its ``matches0`` is drawn, and how
many fine rows / columns each side's fine grid is SHORT of ``stride`` times the coarse one (``None``: an empty fine
map).  Kinds: ``rand`` (about half of the tokens, the four corners always, injective, plus out-of-range values),
``none``, ``all`` (every token), ``coarse`` / ``fine`` (a coarse / fine grid that does not multiply to its rows: not
vouched for), ``long`` (more side-0 rows than ``max_k0``)."""
import hashlib

import numpy as np

import dual_softmax_oracle as dso
import fine_match_oracle as fmo

F32 = np.float32
CELL = 8
OUT_OF_RANGE = (-1, -5, 2 ** 31 - 1, -2 ** 31)       # and S_p itself

# name -> (C, W, stride, pairs)
SHAPES = {
    'c4w3s1': (4, 3, 1, [((1, 1), (1, 1), 'all', 0, 0), ((3, 4), (2, 5), 'rand', 0, 0), ((7, 9), (7, 9), 'rand', 0, 0)]),
    'c8w5s2': (8, 5, 2, [((2, 3), (3, 3), 'rand', 0, 1), ((5, 5), (4, 6), 'rand', 3, 0), ((1, 1), (2, 2), 'rand', 0, 0)]),
    'c60w7s4': (60, 7, 4, [((3, 3), (4, 3), 'rand', 0, 0), ((1, 2), (2, 1), 'all', 5, 2)]),
    'c64w5s4': (64, 5, 4, [((4, 5), (5, 4), 'rand', 0, 0), ((2, 2), (2, 2), 'all', 0, 0)]),
    'c68w3s2': (68, 3, 2, [((3, 5), (5, 3), 'rand', 1, 1), ((1, 1), (1, 1), 'none', 0, 0)]),
    'c128w5s4': (128, 5, 4, [((7, 9), (6, 8), 'rand', 0, 0), ((2, 3), (3, 2), 'rand', 2, 7)]),
    'c512w7s1': (512, 7, 1, [((2, 3), (3, 3), 'rand', 0, 0), ((1, 1), (1, 1), 'all', 0, 0)]),
    # every kind of pair in one call; pair 5 has 63 rows and max_k0 is 35
    'mixed': (64, 5, 4, [((3, 4), (4, 4), 'rand', 0, 0), ((2, 5), (5, 2), 'none', 0, 0), ((3, 3), (3, 4), 'all', 0, 0),
                         ((2, 2), (2, 3), 'coarse', 0, 0), ((2, 3), (2, 2), 'fine', 0, 0), ((7, 9), (7, 9), 'long', 0, 0),
                         ((2, 2), (2, 2), 'all', None, 0), ((1, 3), (2, 2), 'all', 0, None), ((5, 7), (7, 5), 'rand', 9, 13)]),
}
MAX_K0 = {'mixed': 35}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def draw_matches(rng, K0, K1, kind, g0, g1):
    m = np.full(K0, -1, np.int64)
    if kind == 'none':
        m[rng.random(K0) < 0.5] = K1                                 # out of range by one
        return m
    if kind in ('all', 'coarse', 'fine', 'long'):
        assert K1 >= K0 or kind != 'all'
        m[:] = rng.permutation(max(K1, K0))[:K0] % max(K1, 1)
        return m
    corners0 = sorted({0, g0[1] - 1, (g0[0] - 1) * g0[1], K0 - 1})
    corners1 = sorted({0, g1[1] - 1, (g1[0] - 1) * g1[1], K1 - 1})
    n = min(len(corners0), len(corners1))
    m[corners0[:n]] = rng.permutation(corners1)[:n]
    rest0 = np.setdiff1d(np.arange(K0), corners0[:n])
    rest1 = rng.permutation(np.setdiff1d(np.arange(K1), m[corners0[:n]]))
    take = rest0[rng.random(len(rest0)) < 0.5][:len(rest1)]
    m[take] = rest1[:len(take)]
    free = np.nonzero(m == -1)[0]
    for k, a in enumerate(free[:len(OUT_OF_RANGE) + 1]):
        m[a] = (OUT_OF_RANGE + (K1,))[k]
    return m


def make_call(name, seed=0):
    """The inputs of one call: what ``match_dense`` leaves (``matches0``, offsets, grids, keypoints) and the fine side."""
    C, W, stride, pairs = SHAPES[name]
    rng = np.random.default_rng([sum(name.encode()), seed])
    off0, off1, foff0, foff1 = [0], [0], [0], [0]
    grids0, grids1, fgrids0, fgrids1, matches, kp0, kp1 = [], [], [], [], [], [], []
    for g0, g1, kind, cut0, cut1 in pairs:
        K0, K1 = g0[0] * g0[1], g1[0] * g1[1]
        fg = [(0, 0) if cut is None else (max(g[0] * stride - cut, 0), max(g[1] * stride - cut // 2, 0))
              for g, cut in ((g0, cut0), (g1, cut1))]
        matches.append(draw_matches(rng, K0, K1, kind, g0, g1))
        kp0.append(dso.keypoints(*g0, CELL))
        kp1.append(dso.keypoints(*g1, CELL))
        off0.append(off0[-1] + K0)
        off1.append(off1[-1] + K1)
        foff0.append(foff0[-1] + fg[0][0] * fg[0][1])
        foff1.append(foff1[-1] + fg[1][0] * fg[1][1])
        grids0.append((g0[0] + 1, g0[1]) if kind == 'coarse' else g0)
        grids1.append(g1)
        fgrids0.append(fg[0])
        fgrids1.append((fg[1][0], fg[1][1] + 1) if kind == 'fine' else fg[1])
    i32 = lambda v, shape=(-1,): np.asarray(v, np.int64).astype(np.int32).reshape(shape)   # noqa: E731
    return dict(name=name, C=C, W=W, stride=stride, pairs=pairs, matches0=i32(np.concatenate(matches)),
                off0=i32(off0), off1=i32(off1), grids0=i32(grids0, (-1, 2)), grids1=i32(grids1, (-1, 2)),
                foff0=i32(foff0), foff1=i32(foff1), fgrids0=i32(fgrids0, (-1, 2)), fgrids1=i32(fgrids1, (-1, 2)),
                kp0=np.concatenate(kp0).astype(F32), kp1=np.concatenate(kp1).astype(F32),
                fine0=rng.standard_normal((foff0[-1], C)).astype(F32), fine1=rng.standard_normal((foff1[-1], C)).astype(F32),
                max_k0=MAX_K0.get(name))


def matched_total(call):
    """The matches a call has in its vouched pairs, whatever the capacity."""
    return int(np.clip(windows(call, 0)['counts'][:, 0], 0, None).sum())


def windows(call, max_matches):
    return fmo.windows_call(call['matches0'], call['off0'], call['off1'], call['grids0'], call['grids1'], len(call['kp1']),
                            call['fine0'], call['foff0'], call['fgrids0'], call['fine1'], call['foff1'], call['fgrids1'],
                            W=call['W'], stride=call['stride'], max_matches=max_matches, max_k0=call['max_k0'])


def refine(call, win, win0=None, win1=None, fine_cell=2.0):
    return fmo.refine_call(win['win0'] if win0 is None else win0, win['win1'] if win1 is None else win1, win['rows'],
                           win['moffsets'], win['counts'], call['kp0'], call['off0'], call['kp1'], call['off1'],
                           W=call['W'], fine_cell=fine_cell)


def expected(call, max_matches, fine_cell=2.0):
    win = windows(call, max_matches)
    return win, refine(call, win, fine_cell=fine_cell)


def result_record(win, fine):
    """What the fixture keeps of one call's results."""
    return dict(counts=fine['counts'].tolist(), moffsets=win['moffsets'].tolist(), rows=sha(win['rows']),
                win0=sha(win['win0']), win1=sha(win['win1']), expec=sha(fine['expec']), mkpts1=sha(fine['mkpts1']),
                keypoints1=sha(fine['keypoints1']))


# ---------------------------------------------------------------------------------------- the float64 restatement
HEAD_SHAPES = [(8, 3, 1, (3, 4), (4, 3)), (64, 5, 4, (5, 6), (6, 5)), (128, 5, 4, (4, 4), (4, 4)), (32, 7, 2, (3, 3), (3, 5)),
               (256, 5, 4, (2, 3), (3, 2))]                           # C, W, stride, g0, g1


def head_compare(k, seed):
    """Specification against the float64 restatement on one drawn pair whose fine grids are one row short: the list
    and the windows EQUAL, and the largest difference of the expectation, the std and the refined keypoint."""
    C, W, stride, g0, g1 = HEAD_SHAPES[k]
    rng = np.random.default_rng(seed)
    K0, K1 = g0[0] * g0[1], g1[0] * g1[1]
    fg0, fg1 = (g0[0] * stride - 1, g0[1] * stride), (g1[0] * stride, max(g1[1] * stride - 1, 1))
    m = np.full(K0, -1, np.int64)
    take = rng.permutation(K0)[:min(K0, K1) * 3 // 4]
    m[take] = rng.permutation(K1)[:len(take)]
    # a feature scale at which the softmax is neither flat nor one-hot
    fine0 = (rng.standard_normal((fg0[0] * fg0[1], C)) * 1.5).astype(F32)
    fine1 = (rng.standard_normal((fg1[0] * fg1[1], C)) * 1.5).astype(F32)
    kp0, kp1 = dso.keypoints(*g0, CELL), dso.keypoints(*g1, CELL)
    i32 = lambda v: np.asarray(v, np.int32)                            # noqa: E731
    win = fmo.windows_call(m.astype(np.int32), i32([0, K0]), i32([0, K1]), i32([g0]), i32([g1]), K1, fine0,
                           i32([0, len(fine0)]), i32([fg0]), fine1, i32([0, len(fine1)]), i32([fg1]), W=W, stride=stride,
                           max_matches=K0)
    fine = fmo.refine_call(win['win0'], win['win1'], win['rows'], win['moffsets'], win['counts'], kp0, i32([0, K0]), kp1,
                           i32([0, K1]), W=W, fine_cell=CELL / stride)
    tokens0 = np.nonzero(m > -1)[0]
    u0, u1, expec = fmo.published_fine(fine0.reshape(*fg0, C), fine1.reshape(*fg1, C), tokens0, m[tokens0], g0, g1, W, stride)
    n = len(tokens0)
    equal = (int(win['moffsets'][1]) == n and np.array_equal(win['rows'][:n, 1], tokens0)
             and np.array_equal(win['rows'][:n, 2], m[tokens0]) and np.array_equal(win['win0'][:n], u0)
             and np.array_equal(win['win1'][:n], u1) and win['counts'].tolist() == [[n, n]])
    want1 = kp1[m[tokens0]] + expec[:, :2] * (W // 2) * (CELL / stride)
    return dict(equal=bool(equal), matches=n,
                expec_err=float(np.abs(fine['expec'][:n].astype(np.float64) - expec).max()),
                mkpts1_err=float(np.abs(fine['mkpts1'][:n].astype(np.float64) - want1).max()),
                spread=float(np.abs(expec[:, :2]).mean()))


# ---------------------------------------------------------------------------------------- exact cases
def one_hot_windows(W, C, at, rng):
    """``win0`` / ``win1`` ``[1, W*W, C]`` whose heat is one-hot at position ``at``: window 1's rows are orthogonal to
    window 0's centre except row ``at``, whose product is large."""
    WW = W * W
    win0 = rng.standard_normal((1, WW, C)).astype(F32)
    win1 = np.zeros((1, WW, C), F32)
    centre = np.zeros(C, F32)
    centre[0] = 32
    win0[0, WW // 2] = centre
    win1[0, :, 1:] = rng.standard_normal((WW, C - 1)).astype(F32)     # channel 0 is 0: orthogonal to the centre
    win1[0, at, 0] = F32(4 * np.sqrt(C))                              # t = 128 against 0: e(-128) = 0 exactly
    return win0, win1


def planted_scene(W, stride, C, shift, rng, g=(4, 5)):
    """One pair whose fine features' best match is displaced by ``shift`` = (dy, dx) whole fine cells inside the window:
    fine map 1 is fine map 0 rolled by ``shift`` (one-hot-like features), every token matched to itself.  Returns the
    call pieces and the true pixel positions of side 1 ``[K, 2]``."""
    K = g[0] * g[1]
    fg = (g[0] * stride, g[1] * stride)
    base = (rng.standard_normal((fg[0], fg[1], C)) * 3).astype(F32)
    moved = np.roll(base, shift, axis=(0, 1))
    kp = dso.keypoints(*g, CELL)
    fine_cell = CELL / stride
    truth = kp + np.array([shift[1], shift[0]], F32) * F32(fine_cell)
    return dict(matches0=np.arange(K, dtype=np.int32), off=np.array([0, K], np.int32), grid=np.array([g], np.int32),
                foff=np.array([0, fg[0] * fg[1]], np.int32), fgrid=np.array([fg], np.int32), kp=kp,
                fine0=base.reshape(-1, C), fine1=moved.reshape(-1, C), truth=truth, fine_cell=fine_cell, K=K)
