"""The calls of ``tests/test_gpu_pair_counts.py`` and their expected arrays: pair lists past one grid of pairs (the
y extent of a launch, read from the kernels' sources), past one block of the one-thread-per-pair kernels, and many
short match lists in one wave.  Every expected array is the float64 specification of ``tests/*_oracle.py`` computed for
a short cycle of distinct pairs and TILED over the call with numpy; ``tests/test_pair_counts_cpu.py`` checks the tiling
against the specifications run directly on the tiled call's own inputs.  numpy only: no GPU, no torch.
"""
import functools
import json
import re
from pathlib import Path

import numpy as np

import covis_oracle as cvo
import covis_set_oracle as cso
import homography_oracle as hmo
import keypoint_score_oracle as kso
import match_score_oracle as mso
import pose_ransac_oracle as pro

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / 'imagematching_oetr_amd' / 'csrc'


def grid_limit(source, name):
    """``constexpr int <name> = <value>;`` of a kernel source: a renamed or removed constant fails here, at import."""
    return int(re.search(r'constexpr int %s = (\d+);' % name, (CSRC / source).read_text()).group(1))


COVIS_MAX_GRID_Y = grid_limit('covis.hip', 'COVIS_MAX_GRID_Y')
HOM_MAX_GRID_Y = grid_limit('homography.hip', 'HOM_MAX_GRID_Y')


def expected_json(name):
    return json.loads((REPO / 'tests' / name).read_text())


def cycle(n, k, phase=0):
    """Pair p of a call of ``n`` pairs is pair ``(p + phase) % k`` of the cycle."""
    return (np.arange(n) + phase) % k


def launches(n, limit):
    """The launches a call of ``n`` pairs makes under the grid limit ``limit``."""
    return -(-n // limit)


# ------------------------------------------------------------------ covis_boxes (stacked)
COVIS_KINDS = cvo.KINDS + ('plane', 'trunc', 'no_overlap')        # K = 7: valid and invalid pairs alternate
COVIS_SIZES = ((9, 13), (5, 7))


def covis_from_block(depth1, depth2, block):
    """``covis_oracle.overlap_box`` run directly on one pair of a device call: its two maps and its parameter block."""
    b = np.asarray(block, np.float64)
    K1 = np.array([[b[16], 0, b[18]], [0, b[17], b[19]], [0, 0, 1]])
    return cvo.overlap_box(K1, depth1, None, b[29:31], b[31:33], b[20:29].reshape(3, 3), depth2, None, b[33:35],
                           b[35:37], T=b[0:16].reshape(4, 4))


@functools.lru_cache(maxsize=None)
def covis_cycle(h, w, seed=900):
    """The K = 7 checked scenes of one size -> dict of stacked inputs (depth1, depth2 float32 [K,h,w], params float64
    [K,40] with numpy's ``T``) and restated results (box1, box2 float32 [K,4], valid bool, count int32, mask1, mask2
    uint8 [K,h,w], margin)."""
    drawn = [cvo.checked_scene(kind, h, w, seed + 17 * n) for n, kind in enumerate(COVIS_KINDS)]
    assert all(res['margin'] >= cvo.MIN_MARGIN for _, res in drawn)
    stack = lambda key, dtype: np.stack([res[key] for _, res in drawn]).astype(dtype)
    return dict(depth1=np.stack([sc['depth1'] for sc, _ in drawn]), depth2=np.stack([sc['depth2'] for sc, _ in drawn]),
                params=np.stack([cvo.param_block(sc) for sc, _ in drawn]), box1=stack('box1', np.float32),
                box2=stack('box2', np.float32), valid=stack('valid', bool), count=stack('count', np.int32),
                mask1=stack('mask1', np.uint8), mask2=stack('mask2', np.uint8), margin=stack('margin', np.float64))


def covis_call(h, w, n_pairs):
    """-> (cycle dict, src int [n_pairs], expected dict of tiled arrays)."""
    cyc = covis_cycle(h, w)
    src = cycle(n_pairs, len(COVIS_KINDS))
    return cyc, src, {k: cyc[k][src] for k in ('box1', 'box2', 'valid', 'count', 'mask1', 'mask2')}


# ------------------------------------------------------------------ overlap_boxes_indexed / mine_pairs
SET_SIZES = cso.SIZES + ((1, 1), (41, 50), (64, 64))               # the nine-map set of tests/test_gpu_covis_set.py


@functools.lru_cache(maxsize=None)
def the_set():
    views, results = cso.checked_set(SET_SIZES, 0)
    assert min(r['margin'] for r in results.values()) >= cso.MIN_MARGIN
    return views, results


def indexed_call(limit):
    """The 72 ordered pairs cycled to ``limit + 3`` with three index pairs outside the set at ``limit - 1``, ``limit``
    and ``limit + 1`` -> (views, index int32 [P,2], bad bool [P], expected dict: box1, box2 int64 [P,4] (the select
    restatement takes integers), valid bool, count int32)."""
    views, results = the_set()
    pairs, n = sorted(results), len(views)
    P = limit + 3
    src = cycle(P, len(pairs))
    index = np.array(pairs, np.int32)[src]
    bad = np.zeros(P, bool)
    for at, pair in ((limit - 1, (-1, 2)), (limit, (2, n)), (limit + 1, (n, -1))):
        index[at], bad[at] = pair, True
    base = {k: np.stack([results[p][k] for p in pairs]) for k in ('box1', 'box2', 'valid', 'count')}
    want = dict(box1=base['box1'][src].astype(np.int64), box2=base['box2'][src].astype(np.int64),
                valid=base['valid'][src].astype(bool), count=base['count'][src].astype(np.int32))
    want['box1'][bad], want['box2'][bad], want['valid'][bad], want['count'][bad] = 0, 0, False, -1
    return views, index, bad, want


def tiled_select(box1, box2, valid, min_scale_diff=2.0, limit=None):
    """``covis_set_oracle.select`` of a list with few DISTINCT rows: the criterion is evaluated once per distinct
    ``(box1, box2, valid)`` and tiled -> (kept int32 [P], n_kept, scale_diff float64 [P])."""
    rows = np.concatenate([np.asarray(box1, np.int64), np.asarray(box2, np.int64),
                           np.asarray(valid, np.int64).reshape(-1, 1)], axis=1)
    uniq, inverse = np.unique(rows, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    sd = np.array([cso.scale_diff(r[0:4], r[4:8]) for r in uniq], np.float64)
    keep = np.array([cso.keep(r[0:4], r[4:8], bool(r[8]), min_scale_diff) for r in uniq], bool)
    chosen = np.flatnonzero(keep[inverse])
    if limit is not None and limit > 0:
        chosen = chosen[:limit]
    kept = np.full(len(rows), -1, np.int32)
    kept[:len(chosen)] = chosen
    return kept, len(chosen), sd[inverse]


# ------------------------------------------------------------------ overlap_boxes_from_homography
@functools.lru_cache(maxsize=None)
def homography_boxes():
    boxes = hmo.make_boxes(expected_json('homography_expected.json')['seed'])
    assert min(b['res']['margin'] for b in boxes) >= cvo.MIN_MARGIN
    return boxes


def homography_call(n_pairs):
    """``homography_oracle.make_boxes`` (every kind x every size pair) cycled -> (params float64 [P,16], (max_h1,
    max_w1), src, expected dict)."""
    boxes = homography_boxes()
    src = cycle(n_pairs, len(boxes))
    params = np.stack([hmo.param_block(b['H'], *b['sizes']) for b in boxes])
    stack = lambda key, dtype: np.stack([b['res'][key] for b in boxes]).astype(dtype)
    want = dict(box1=stack('box1', np.float32)[src], box2=stack('box2', np.float32)[src],
                valid=stack('valid', bool)[src], count=stack('count', np.int32)[src])
    top = (max(b['sizes'][0][0] for b in boxes), max(b['sizes'][0][1] for b in boxes))
    return params[src], top, src, want


# ------------------------------------------------------------------ pinned match lists, tiled
def _tile_lists(lists, copies):
    """``[(k1, k2), ...]`` repeated ``copies`` times -> (k1, k2 float32 [M,2], lengths)."""
    k1 = np.concatenate([a for a, _ in lists]).astype(np.float32).reshape(-1, 2)
    k2 = np.concatenate([b for _, b in lists]).astype(np.float32).reshape(-1, 2)
    return np.tile(k1, (copies, 1)), np.tile(k2, (copies, 1)), [len(a) for a, _ in lists] * copies


@functools.lru_cache(maxsize=None)
def match_score_call(copies=20):
    """The 14 pinned lists of ``tests/match_score_expected.json`` x ``copies`` -> dict(views, pairs, k1, k2, lengths,
    blocks float64 [P,20], thr, want: flags uint8 [M], the four value arrays float64 [M], counts int32 [P,5])."""
    rec = expected_json('match_score_expected.json')
    thr = rec['thresholds']
    views = mso.make_scene(tuple(tuple(s) for s in rec['sizes']), rec['seed'])
    lists = mso.make_lists(views, seed=rec['seed'])
    assert [cvo.sha(np.concatenate([a, b])) for a, b in lists] == rec['kpts_sha256']
    wants = mso.score_lists(views, mso.PAIRS, lists, **thr)
    for res, (a, b) in zip(wants, lists):
        t, tie = mso.margins(res, a, b, **thr)
        assert t >= mso.MIN_THRESHOLD_MARGIN and tie >= mso.MIN_TIE_MARGIN
    k1, k2, lengths = _tile_lists(lists, copies)
    want = {k: np.tile(np.concatenate([w[k] for w in wants]), copies) for k in mso.VALUES + ('flags',)}
    want['counts'] = np.tile(np.stack([w['counts'] for w in wants]), (copies, 1))
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in mso.PAIRS])
    return dict(views=views, pairs=list(mso.PAIRS) * copies, k1=k1, k2=k2, lengths=lengths,
                blocks=np.tile(blocks, (copies, 1)), thr=thr, want=want)


@functools.lru_cache(maxsize=None)
def homography_score_call(copies=22):
    """The 12 pinned lists of ``tests/homography_expected.json`` x ``copies`` (264 pairs) -> dict(params float64
    [P,16], k1, k2, lengths, want: dist_sq float64 [M], counts int32 [P,16])."""
    rec = expected_json('homography_expected.json')
    lists = hmo.make_lists(rec['seed'])
    assert [cvo.sha(np.concatenate([e['k1'], e['k2']])) for e in lists] == rec['kpts_sha256']
    wants = [hmo.score(e['H'], e['k1'], e['k2']) for e in lists]
    margin = min(hmo.threshold_margin(w['dist_sq']) for w in wants)
    assert margin >= mso.MIN_THRESHOLD_MARGIN
    params, k1, k2, lengths = hmo.concatenate(lists)
    return dict(params=np.tile(params, (copies, 1)), k1=np.tile(k1, (copies, 1)), k2=np.tile(k2, (copies, 1)),
                lengths=lengths * copies,
                want=dict(dist_sq=np.tile(np.concatenate([w['dist_sq'] for w in wants]), copies),
                          counts=np.tile(np.stack([w['counts'] for w in wants]), (copies, 1))))


@functools.lru_cache(maxsize=None)
def keypoint_call(copies=3):
    """The 48 pinned pairs of ``tests/keypoint_score_expected.json`` x ``copies`` over the SAME 12 pictures -> dict(
    views, kps, pairs, blocks, thr, max_kp, want: counts, nearest, dist_sq in the device's layout)."""
    rec = expected_json('keypoint_score_expected.json')
    thr = tuple(rec['thresholds'])
    scene = mso.make_scene(tuple(tuple(s) for s in rec['sizes']), rec['seed'])
    views, kps, pairs = [], [], []
    for s, one in enumerate(rec['sets']):
        sets = kso.make_keypoints(scene, one['counts'], one['seed'])
        assert [cvo.sha(k) for k in sets] == one['kpts_sha256']
        results = kso.score_pairs(scene, sets, thresholds=thr)
        t, tie = kso.set_margins(results, sets, thresholds=thr)
        assert t >= kso.MIN_THRESHOLD_MARGIN and tie >= kso.MIN_TIE_MARGIN
        views += scene
        kps += sets
        pairs += [(4 * s + i, 4 * s + j) for i, j in kso.PAIRS]
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in pairs])
    max_kp = max(len(k) for k in kps)
    results = [kso.score(views[i]['depth'], views[j]['depth'], blocks[p], kps[i], kps[j], thr)
               for p, (i, j) in enumerate(pairs)]
    want = dict(zip(('counts', 'nearest', 'dist_sq'), kso.padded(results, max_kp)))
    return dict(views=views, kps=kps, pairs=pairs * copies, blocks=np.tile(blocks, (copies, 1)), thr=thr,
                max_kp=max_kp, want={k: np.tile(v, (copies, 1, 1)) for k, v in want.items()})


@functools.lru_cache(maxsize=None)
def pose_call(copies=17):
    """The 16 pinned lists of ``tests/pose_ransac_expected.json`` x ``copies`` (272 pairs), ``pair_ids = p % 16``, the
    smallest pinned ``n_hyp`` -> dict(blocks, k1, k2, lengths, pair_ids, n_hyp, seed, want: models, model_counts,
    model, pose, cosines, counts per pair and inliers per row)."""
    rec = expected_json('pose_ransac_expected.json')
    blocks, lists, _ = pro.pinned_call(rec['pinned']['draws'])
    assert [cvo.sha(np.concatenate([a, b])) for a, b in lists] == rec['pinned']['kpts_sha256']
    n_hyp = min(pro.PINNED_HYPOTHESES)
    wants = pro.estimate_lists(blocks, lists, n_hyp, pro.PINNED_SEED)
    assert all(pro.margins_hold(w) for w in wants)
    k1, k2, lengths = _tile_lists(lists, copies)
    n = len(lists)
    want = {k: np.tile(np.stack([w[k] for w in wants]), (copies,) + (1,) * wants[0][k].ndim)
            for k in ('models', 'model_counts', 'model', 'pose', 'cosines', 'counts')}
    want['inliers'] = np.tile(np.concatenate([w['inliers'] for w in wants]), copies)
    return dict(blocks=np.tile(blocks, (copies, 1)), k1=k1, k2=k2, lengths=lengths,
                pair_ids=(np.arange(n * copies) % n).astype(np.int32), n_hyp=n_hyp, seed=pro.PINNED_SEED, want=want)


# ------------------------------------------------------------------ many short lists in one wave
SHORT_LENGTHS = (0, 1, 2, 3, 0, 5, 64, 1)
SHORT_LISTS = 70000
SHORT_BEFORE, SHORT_AFTER = 50, 53
SHORT_SIZES = ((40, 64), (56, 56))
SHORT_COMBOS = ((0, 1), (1, 0))                                    # the (i, j) of even and of odd pairs
SHORT_HOM_THRESHOLDS = (1, 3)


def short_offsets(n_lists=SHORT_LISTS):
    """-> (offsets int32 [n_lists + 1], M, owner int [M]: the list of every row, -1 outside every list)."""
    lengths = np.resize(np.array(SHORT_LENGTHS), n_lists)
    offsets = (SHORT_BEFORE + np.concatenate([[0], np.cumsum(lengths)])).astype(np.int32)
    M = int(offsets[-1]) + SHORT_AFTER
    owner = np.searchsorted(offsets, np.arange(M), 'right') - 1
    owner[(owner < 0) | (owner >= n_lists)] = -1
    return offsets, M, owner


def _by_combo(owner, parts):
    """Row m from ``parts[owner[m] % 2]`` (a row outside every list from ``parts[0]``)."""
    odd = (owner >= 0) & (owner % 2 == 1)
    return np.where(odd.reshape((-1,) + (1,) * (parts[0].ndim - 1)), parts[1], parts[0])


def _bincount(owner, hit, n_lists):
    inside = owner >= 0
    return np.bincount(owner[inside & hit], minlength=n_lists).astype(np.int32)


@functools.lru_cache(maxsize=None)
def short_match_call(n_lists=SHORT_LISTS, seed=0):
    """``score_matches`` over ``n_lists`` short lists whose pairs alternate between ``SHORT_COMBOS``: the rows are
    scored by the specification in TWO calls, one per combination, and every row takes the result of its own list's
    combination; the counters are ``np.bincount`` over the rows' owners.  Re-drawn (seed + 1000, ...) until the
    margins of ``match_score_oracle`` hold over every row; none is left out.  -> dict(views, pairs int32 [P,2], blocks,
    offsets, k1, k2, owner, thr, seed, want: flags, the four value arrays (NaN / 0 outside every list), counts)."""
    thr = dict(mso.THRESHOLDS)
    offsets, M, owner = short_offsets(n_lists)
    inside = owner >= 0
    for attempt in range(20):
        s = seed + 1000 * attempt
        views = mso.make_scene(SHORT_SIZES, s, behind=None)
        drawn = [mso.make_matches(views, i, j, M, seed=s + 31 + c) for c, (i, j) in enumerate(SHORT_COMBOS)]
        k1, k2 = (_by_combo(owner, [d[side] for d in drawn]) for side in (0, 1))
        blocks = [mso.pair_block(views, i, j) for i, j in SHORT_COMBOS]
        scored = [mso.score(views[i]['depth'], views[j]['depth'], blocks[c], k1, k2, **thr)
                  for c, (i, j) in enumerate(SHORT_COMBOS)]
        res = {k: _by_combo(owner, [sc[k] for sc in scored]) for k in mso.VALUES + ('flags',)}
        t, tie = mso.margins({k: v[inside] for k, v in res.items()}, k1[inside], k2[inside], **thr)
        if t >= mso.MIN_THRESHOLD_MARGIN and tie >= mso.MIN_TIE_MARGIN:
            break
    else:
        raise AssertionError('no draw of the short lists keeps the margins')
    assert np.isfinite(res['episym'][inside]).all()                   # a NaN of the device then means "no list"
    want = {k: np.where(inside, res[k], np.nan) for k in mso.VALUES}
    want['flags'] = np.where(inside, res['flags'], 0).astype(np.uint8)
    f = want['flags']
    both = (f & 3) == 3
    want['counts'] = np.stack([np.diff(offsets).astype(np.int32), _bincount(owner, (f & mso.FLAG_EPI) != 0, n_lists),
                               _bincount(owner, (f & mso.FLAG_EPISYM) != 0, n_lists), _bincount(owner, both, n_lists),
                               _bincount(owner, (f & mso.FLAG_REPROJ) != 0, n_lists)], axis=1)
    pairs = np.array(SHORT_COMBOS, np.int32)[np.arange(n_lists) % 2]
    return dict(views=views, pairs=pairs, blocks=np.stack(blocks)[np.arange(n_lists) % 2], offsets=offsets, k1=k1,
                k2=k2, owner=owner, thr=thr, seed=s, want=want)


@functools.lru_cache(maxsize=None)
def short_homography_call(n_lists=SHORT_LISTS, seed=0):
    """``score_matches_homography`` over the same offsets, the pairs alternating between two checked homographies
    (a similarity and a perspective one), thresholds ``SHORT_HOM_THRESHOLDS`` -> dict(params float64 [P,16], offsets,
    k1, k2, owner, seed, want: dist_sq (NaN outside every list), counts int32 [P,3])."""
    offsets, M, owner = short_offsets(n_lists)
    inside = owner >= 0
    for attempt in range(20):
        s = seed + 1000 * attempt
        Hs = [hmo.checked_homography(kind, hmo.LIST_SIZES, s + 7 * c)[0] for c, kind in enumerate(('similarity', 'perspective'))]
        drawn = [hmo.make_matches(H, hmo.LIST_SIZES, M, seed=s + 31 + c) for c, H in enumerate(Hs)]
        k1, k2 = (_by_combo(owner, [d[side] for d in drawn]) for side in (0, 1))
        scored = [hmo.score(H, k1, k2, SHORT_HOM_THRESHOLDS)['dist_sq'] for H in Hs]
        dist_sq = _by_combo(owner, scored)
        if hmo.threshold_margin(dist_sq[inside], SHORT_HOM_THRESHOLDS) >= mso.MIN_THRESHOLD_MARGIN:
            break
    else:
        raise AssertionError('no draw of the short lists keeps the threshold margin')
    assert np.isfinite(dist_sq[inside]).all()
    counts = [np.diff(offsets).astype(np.int32)]
    counts += [_bincount(owner, dist_sq <= np.float64(t) * np.float64(t), n_lists) for t in SHORT_HOM_THRESHOLDS]
    params = np.stack([hmo.param_block(H, *hmo.LIST_SIZES) for H in Hs])[np.arange(n_lists) % 2]
    return dict(params=params, offsets=offsets, k1=k1, k2=k2, owner=owner, seed=s,
                want=dict(dist_sq=np.where(inside, dist_sq, np.nan), counts=np.stack(counts, axis=1)))
