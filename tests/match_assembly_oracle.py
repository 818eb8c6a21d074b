"""The specification of the match-assembly extension (``include/oetr_match_assembly.h``): numpy, fixed
operation order, no tolerance anywhere.

It restates the tail of the reference's ``process()`` (``dloc/core/overlap_features.py:118-155``) for a whole pair list:

* ``origin``: ``(keypoints / ratio + bbox[:2]) * scales`` with the reference's dtypes - float32 keypoints over the
  float32 ratio (the correctly rounded float32 quotient), plus the float32 box origin (float32), times a pair of Python
  floats (float64);
* ``assemble``: per pair ``valid = matches > -1``, ``index0 = nonzero(valid)``, ``index1 = matches[valid]``,
  ``mconf = conf[valid]`` - where a match ``>= K1`` (numpy would raise on it) is dropped and counted - the lists
  concatenated in pair order, ``k1`` / ``k2`` the float32 roundings of the origin keypoints, the ``-1`` / NaN tail, the
  four counters per pair and the selection of the pairs with too few matches.

``make_call`` builds the ONE pinned call of the tests (``tests/match_assembly_expected.json`` holds its hashes, counters
and offsets; ``tools/gen_golden_match_assembly.py`` writes it).
"""
import numpy as np

from covis_oracle import sha  # noqa: F401  (sha256 of an array's bytes)
from match_score_oracle import equal_bits  # noqa: F401  (NaN-aware comparison by bits)

COUNTERS = 4          # K0, K1, kept, rejected
MIN_MATCHES = 30      # overlap_features.py:215

# oetr_crop_info (include/oetr_hip.h), 152 bytes
INFO_DTYPE = np.dtype([('valid', '<i4'), ('box', '<i4', (2, 4)), ('crop_w', '<i4', (2,)), ('crop_h', '<i4', (2,)),
                       ('new_w', '<i4', (2,)), ('new_h', '<i4', (2,)), ('out_w', '<i4', (2,)), ('out_h', '<i4', (2,)),
                       ('ratio', '<f8', (2, 2)), ('sbox', '<f4', (2, 4))], align=True)


def origin(kp, ratio, sbox_xy, scale):
    """float32 ``[K,2]`` crop keypoints -> float64 ``[K,2]`` in the original picture.  ``ratio``: two doubles (rounded
    to float32 first, as the reference's ``torch.tensor(ratio)`` does), ``sbox_xy``: two float32, ``scale``: two
    doubles."""
    k = np.asarray(kp, np.float32).reshape(-1, 2)
    r = np.asarray(ratio, np.float64).astype(np.float32).reshape(1, 2)
    b = np.asarray(sbox_xy, np.float32).reshape(1, 2)
    q = (k / r).astype(np.float32)                    # float32 / float32: the correctly rounded quotient
    t = (q + b).astype(np.float32)
    return t.astype(np.float64) * np.asarray(scale, np.float64).reshape(1, 2)


def assemble(info, scales, kp0, kp1, off0, off1, matches, conf=None, min_matches=MIN_MATCHES):
    """The whole call.  ``info``: ``INFO_DTYPE [P]``; ``scales``: float64 ``[P,2,2]``; ``kp0`` / ``kp1``: float32
    ``[N0,2]`` / ``[N1,2]``; ``off0`` / ``off1``: ``[P+1]``; ``matches``: integer ``[N0]``; ``conf``: float32 ``[N0]``
    or None.  Returns every output array as the device call leaves it."""
    P, N0, N1 = len(info), len(kp0), len(kp1)
    out = dict(origin0=np.full((N0, 2), np.nan), origin1=np.full((N1, 2), np.nan),
               index0=np.full(N0, -1, np.int32), index1=np.full(N0, -1, np.int32),
               k1=np.full((N0, 2), np.nan, np.float32), k2=np.full((N0, 2), np.nan, np.float32),
               offsets=np.zeros(P + 1, np.int32), counts=np.zeros((P, COUNTERS), np.int32))
    if conf is not None:
        out['mconf'] = np.full(N0, np.nan, np.float32)
    few, at = [], 0
    for p in range(P):
        out['offsets'][p] = at
        s0, e0, s1, e1 = int(off0[p]), int(off0[p + 1]), int(off1[p]), int(off1[p + 1])
        K0, K1 = e0 - s0, e1 - s1
        if info['valid'][p] < 0:                      # no crops were made: nothing to assemble
            out['counts'][p] = -1
            few.append(p)
            continue
        for i, (s, e, kp, name) in enumerate(((s0, e0, kp0, 'origin0'), (s1, e1, kp1, 'origin1'))):
            out[name][s:e] = origin(kp[s:e], info['ratio'][p, i], info['sbox'][p, i, :2], scales[p, i])
        m = np.asarray(matches[s0:e0]).astype(np.int64)
        valid = m > -1
        keep = valid & (m < K1)
        index0 = np.nonzero(keep)[0]
        index1 = m[keep]
        n = len(index0)
        out['index0'][at:at + n] = index0
        out['index1'][at:at + n] = index1
        out['k1'][at:at + n] = out['origin0'][s0:e0][index0].astype(np.float32)       # round to nearest even
        out['k2'][at:at + n] = out['origin1'][s1:e1][index1].astype(np.float32)
        if conf is not None:
            out['mconf'][at:at + n] = conf[s0:e0][keep]
        out['counts'][p] = (K0, K1, n, int((valid & ~keep).sum()))
        if min_matches is not None and n < min_matches:
            few.append(p)
        at += n
    out['offsets'][P] = at
    if min_matches is not None:
        out['few'] = np.full(P, -1, np.int32)
        out['few'][:len(few)] = few
        out['n_few'] = np.array([len(few)], np.int32)
    return out


# ------------------------------------------------------------------ the pinned call
# (K0, K1, kind of matches0, oetr_crop_info.valid).  K0 on the wave edges (64, and 256: a quarter of a workgroup), on
# the edges of a workgroup's chunk (1024 rows: 1023, 1024, 1025) and beyond two chunks (2049: three chunks, so the
# running base is carried twice and both LDS buffers of the emit launch are used again); K1 with 0 and 1.
#   none: no row matched; all: every row matched, no b twice; dup: every row matched, b drawn with replacement;
#   random: about half matched; over: as random, a tenth of the matched rows with b in [K1, K1 + 60) - addresses that,
#   unguarded, would still lie in the NEXT pairs' rows of kp1, never outside the tensor.
PAIRS = ((0, 5, 'none', 1), (1, 1, 'all', 1), (63, 40, 'random', 1), (64, 64, 'all', 1), (65, 0, 'over', 1),
         (255, 300, 'none', 1), (256, 256, 'random', 0), (257, 100, 'dup', 1), (513, 700, 'random', -1),
         (1000, 900, 'over', 1), (1023, 1024, 'random', 1), (1024, 1024, 'all', 1), (1025, 600, 'dup', 1),
         (2049, 2100, 'random', 1), (300, 128, 'random', 1), (40, 1, 'random', 1), (20, 20, 'all', 1))
SCALES = ((1.6, 1.6), (0.75, 0.75), (1.0, 1.0), (1.25, 0.8))
OVER = 60


def make_matches(rng, K0, K1, kind):
    none = rng.choice(np.array([-1, -1, -1, -2, -7]), size=K0)
    if kind == 'none':
        return none
    if kind == 'all':
        return rng.permutation(K1)[:K0]
    if kind == 'dup':
        return rng.integers(0, K1, size=K0)
    matched = rng.random(K0) < 0.5
    b = rng.integers(0, max(K1, 1), size=K0) if K1 else rng.integers(0, 3, size=K0)
    if kind == 'over':
        b = np.where(rng.random(K0) < 0.1, rng.integers(K1, K1 + OVER, size=K0), b)
    return np.where(matched, b, none)


def make_call(seed=0, pairs=PAIRS):
    """The pinned call: ``dict(info, scales, kp0, kp1, off0, off1, matches (int32), conf)``."""
    rng = np.random.default_rng(seed)
    P = len(pairs)
    info = np.zeros(P, INFO_DTYPE)
    scales = np.zeros((P, 2, 2))
    kp0, kp1, matches = [], [], []
    for p, (K0, K1, kind, valid) in enumerate(pairs):
        info['valid'][p] = valid
        if valid == 1:                                # doubles that are no float32 values; box origins off zero
            info['ratio'][p] = rng.uniform(0.35, 2.8, size=(2, 2))
            info['sbox'][p, :, :2] = rng.uniform(1.0, 200.0, size=(2, 2)).astype(np.float32)
            info['sbox'][p, :, 2:] = info['sbox'][p, :, :2] + np.float32(320.0)
        elif valid == 0:                              # the gate failed: ratio 1 and the full-image box
            info['ratio'][p] = 1.0
            info['sbox'][p] = ((0, 0, 640, 480), (0, 0, 512, 384))
        # valid == -1: a zeroed record; nothing of it may reach the outputs
        scales[p, 0] = SCALES[p % len(SCALES)]
        scales[p, 1] = SCALES[(p + 1) % len(SCALES)] if p % 3 else rng.uniform(0.5, 2.5, size=2)
        kp0.append(rng.uniform(0.0, 640.0, size=(K0, 2)).astype(np.float32))
        kp1.append(rng.uniform(0.0, 640.0, size=(K1, 2)).astype(np.float32))
        matches.append(make_matches(rng, K0, K1, kind).astype(np.int32))
    off0 = np.concatenate([[0], np.cumsum([q[0] for q in pairs])]).astype(np.int32)
    off1 = np.concatenate([[0], np.cumsum([q[1] for q in pairs])]).astype(np.int32)
    N0 = int(off0[-1])
    return dict(info=info, scales=scales, kp0=np.concatenate(kp0).reshape(-1, 2), kp1=np.concatenate(kp1).reshape(-1, 2),
                off0=off0, off1=off1, matches=np.concatenate(matches), conf=rng.random(N0).astype(np.float32))


def input_hashes(call):
    return {k: sha(call[k]) for k in ('info', 'scales', 'kp0', 'kp1', 'off0', 'off1', 'matches', 'conf')}


def record(seed, call, res):
    """What ``tests/match_assembly_expected.json`` holds: no arrays."""
    return dict(seed=seed, pairs=[list(q) for q in PAIRS], min_matches=MIN_MATCHES, inputs_sha256=input_hashes(call),
                counts=res['counts'].tolist(), offsets=res['offsets'].tolist(), few=res['few'].tolist(),
                n_few=int(res['n_few'][0]),
                outputs_sha256={k: sha(res[k]) for k in ('index0', 'index1', 'offsets', 'counts', 'few')})
