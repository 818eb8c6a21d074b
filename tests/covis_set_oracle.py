"""float64 numpy restatement of the depth-map-set extension (``include/oetr_covis_set.h``), written from the
specification, and the synthetic image sets its tests, the generator of the pinned sets
(``tools/gen_golden_covis_set.py``) and the probe (``tools/covis_set_probe.py``) share.  Builds on
``covis_oracle`` (its plane renderer, its margin rule, its hashes) and changes nothing there.

``overlap_box_hw`` is ``covis_oracle.overlap_box`` for a map 1 of ``H1 x W1`` against a map 2 of ``H2 x W2`` (landing
test ``0 <= i < W2, 0 <= j < H2``) and reports the same DECISION MARGIN.  ``scale_diff`` and ``keep`` are the
reference's mining criterion (``src/utils/megadepth_preprocess.py:71-92, 199-200``) with Python's ``max``.
``make_set`` draws M cameras on one tilted plane; ``checked_set`` re-draws a whole set until EVERY ordered pair
``(i, j)``, ``i != j``, has margin >= ``MIN_MARGIN`` - no pair is ever left out.  A self pair ``(i, i)`` projects every
pixel onto itself, an integer: its margin is zero by construction, so a comparison of self pairs must hand the
restatement the very ``T`` the device used (``overlap_box_hw(..., T=...)``); then every operation is the same IEEE
float64 operation on both sides and the results are equal whatever the margin.
"""
import numpy as np

import covis_oracle as cvo

MIN_MARGIN = cvo.MIN_MARGIN
SIDES = ('depth', 'intrinsics', 'pose', 'bbox', 'ratio')


def overlap_box_hw(K1, depth1, pose1, bbox1, ratio1, K2, depth2, pose2, bbox2, ratio2, T=None):
    """-> dict(box1, box2 int64 [4], valid bool, count int, margin float).  ``depth1`` [H1,W1] / ``depth2`` [H2,W2]
    are used as float64.  ``T``: ``pose2 @ inv(pose1)`` when the caller has it."""
    d1, d2 = np.asarray(depth1, np.float64), np.asarray(depth2, np.float64)
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    b1, r1, b2, r2 = (np.asarray(a, np.float64) for a in (bbox1, ratio1, bbox2, ratio2))
    H2, W2 = d2.shape
    if T is None:
        T = np.asarray(pose2, np.float64) @ np.linalg.inv(np.asarray(pose1, np.float64))
    v1, u1 = np.nonzero(d1 > 0)
    Z = d1[v1, u1]
    with np.errstate(all='ignore'):
        x = (u1 + b1[1] + 0.5) / r1[1]
        y = (v1 + b1[0] + 0.5) / r1[0]
        X = (x - K1[0, 2]) * (Z / K1[0, 0])
        Y = (y - K1[1, 2]) * (Z / K1[1, 1])
        q = [((T[r, 0] * X + T[r, 1] * Y) + T[r, 2] * Z) + T[r, 3] for r in range(4)]
        Xc, Yc, Zc = q[0] / q[3], q[1] / q[3], q[2] / q[3]
        a = [(K2[r, 0] * Xc + K2[r, 1] * Yc) + K2[r, 2] * Zc for r in range(3)]
        u2 = (a[0] / a[2]) * r2[1] - b2[1] - 0.5
        v2 = (a[1] / a[2]) * r2[0] - b2[0] - 0.5
        inside = (u2 > -1.0) & (u2 < W2) & (v2 > -1.0) & (v2 < H2)        # trunc() in range; False for NaN
        near = np.isfinite(u2) & np.isfinite(v2) & (u2 > -2.0) & (u2 < W2 + 1.0) & (v2 > -2.0) & (v2 < H2 + 1.0)
    margin = np.inf
    if near.any():
        un, vn = u2[near], v2[near]
        margin = min(np.abs(un - np.round(un)).min(), np.abs(vn - np.round(vn)).min())
    i = np.trunc(u2[inside]).astype(np.int64)
    j = np.trunc(v2[inside]).astype(np.int64)
    dz = np.abs(Zc[inside] - d2[j, i])
    if dz.size:
        margin = min(margin, np.abs(dz - 0.5).min())
    inl = dz < 0.5
    uu, vv, ii, jj = u1[inside][inl], v1[inside][inl], i[inl], j[inl]
    count = int(inl.sum())
    box1 = box2 = np.zeros(4, np.int64)
    if count:
        box1 = np.array([uu.min(), vv.min(), uu.max(), vv.max()], np.int64)
        box2 = np.array([ii.min(), jj.min(), ii.max(), jj.max()], np.int64)
    return dict(box1=box1, box2=box2, valid=count > 0, count=count, margin=float(margin))


def view_args(view):
    """A view as one side of the reference's positional arguments (float64 depth map)."""
    return tuple(np.asarray(view[k], np.float64) for k in ('intrinsics', 'depth', 'pose', 'bbox', 'ratio'))


def restate_pair(views, i, j, T=None):
    return overlap_box_hw(*view_args(views[i]), *view_args(views[j]), T=T)


def as_scene(views, i, j):
    """Two views as a ``covis_oracle`` scene (the dataset's names with 1 / 2)."""
    return {f'{k}{s}': views[m][k] for s, m in (('1', i), ('2', j)) for k in SIDES}


# ------------------------------------------------------------------ the mining criterion
def _pymax(a, b):
    """Python's ``max(a, b)``: a unless b > a."""
    return b if b > a else a


def scale_diff(box1, box2):
    """The reference's ``scale_diff`` on two integer boxes, float64; a zero width gives numpy's inf / NaN."""
    b1, b2 = np.asarray(box1, np.int64), np.asarray(box2, np.int64)
    with np.errstate(all='ignore'):
        w = _pymax((b1[2] - b1[0]) / (b2[2] - b2[0]), (b2[2] - b2[0]) / (b1[2] - b1[0]))
        h = _pymax((b1[3] - b1[1]) / (b2[3] - b2[1]), (b2[3] - b2[1]) / (b1[3] - b1[1]))
    return np.float64(_pymax(w, h))


def keep(box1, box2, valid, min_scale_diff=2.0):
    return bool(valid and np.max(box1) > 0 and np.max(box2) > 0 and scale_diff(box1, box2) > min_scale_diff)


def select(boxes1, boxes2, valids, min_scale_diff=2.0, limit=None):
    """-> (kept int32 [P] (ascending pair numbers cut at ``limit``, then -1), n_kept, scale_diff float64 [P])."""
    n = len(valids)
    sd = np.array([scale_diff(a, b) for a, b in zip(boxes1, boxes2)], np.float64).reshape(n)
    chosen = [p for p in range(n) if keep(boxes1[p], boxes2[p], valids[p], min_scale_diff)]
    if limit is not None and limit > 0:
        chosen = chosen[:limit]
    kept = np.full(n, -1, np.int32)
    kept[:len(chosen)] = chosen
    return kept, len(chosen), sd


# ------------------------------------------------------------------ synthetic image sets
# Drawn like covis_oracle's scenes: elementwise float64 arithmetic, libm's scalar functions and numpy's seeded
# generator only, so a (sizes, seed) recipe gives the same bytes on every machine.
SIZES = ((48, 64), (64, 48), (56, 56), (40, 72), (33, 47), (64, 64))
ZOOM_VIEW, AWAY_VIEW = 1, 4        # focal length x 2.6 / another part of the plane


def make_set(sizes, seed):
    """One view per entry of ``sizes`` = ((h, w), ...) of one tilted world plane: per-view size, intrinsics, crop
    offset, resize ratio and pose, holes in every depth map.  View ``ZOOM_VIEW`` has its focal length x 2.6 (its
    pairs pass ``scale_diff > 2``), view ``AWAY_VIEW`` (where the set has that many) sees another part of the plane
    (its pairs have no inlier)."""
    rng = np.random.default_rng(seed)
    normal = np.array([0.1, 0.05, 1.0]) + 0.05 * rng.standard_normal(3)
    normal = normal / np.sqrt((normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2])
    d = 10.0 + rng.uniform(-1, 1)
    views = []
    for m, (h, w) in enumerate(sizes):
        s = min(h, w) / 640.0
        f = (640.0 + 60.0 * rng.uniform()) * s * (2.6 if m == ZOOM_VIEW else 1.0)
        K = np.array([[f, 0, (0.5 + 0.1 * rng.uniform()) * w], [0, f * 1.02, (0.45 + 0.1 * rng.uniform()) * h], [0, 0, 1]])
        bbox = np.array([12.0 * rng.uniform(), 20.0 * rng.uniform()]) * s
        ratio = np.array([0.9 + 0.2 * rng.uniform()] * 2)
        R = cvo._matmul3(cvo._rot(1, 0.12 * rng.standard_normal()), cvo._rot(0, 0.06 * rng.standard_normal()))
        t = np.array([0.8, 0.5, 0.3]) * rng.standard_normal(3)
        if m == AWAY_VIEW:
            t = t + np.array([-60.0, 0.0, 0.0])
        P = cvo._pose(R, t)
        depth = cvo.render_plane(K, P, h, w, normal, d, bbox, ratio)
        depth[rng.random(depth.shape) < 0.2] = 0                  # holes, 80 % coverage
        views.append(dict(depth=depth.astype(np.float32), intrinsics=K, pose=P, bbox=bbox, ratio=ratio))
    return views


def ordered_pairs(m):
    return [(i, j) for i in range(m) for j in range(m) if i != j]


def checked_set(sizes=SIZES, seed=0):
    """``make_set`` re-drawn (seed + 1000, ...) until every ordered pair's margin is >= MIN_MARGIN.
    -> (views, {(i, j): result of ``overlap_box_hw``} over all ordered pairs)."""
    for attempt in range(20):
        views = make_set(sizes, seed + 1000 * attempt)
        results = {(i, j): restate_pair(views, i, j) for i, j in ordered_pairs(len(views))}
        if min(r['margin'] for r in results.values()) >= MIN_MARGIN:
            return views, results
    raise AssertionError(f'no set of sizes {sizes} with every margin >= {MIN_MARGIN} in 20 draws from seed {seed}')


def set_record(views, results, min_scale_diff=2.0):
    """A checked set as JSON-able recorded values: input hashes, and per ordered pair boxes, valid, count,
    scale_diff (``repr`` of the float64: inf and nan survive) and the kept list."""
    pairs = sorted(results)
    kept, n_kept, sd = select([results[p]['box1'] for p in pairs], [results[p]['box2'] for p in pairs],
                              [results[p]['valid'] for p in pairs], min_scale_diff)
    return dict(depth_sha256=[cvo.sha(v['depth']) for v in views],
                camera_sha256=cvo.sha(np.concatenate([np.concatenate([v[k].reshape(-1) for k in SIDES[1:]]) for v in views])),
                pairs=[list(p) for p in pairs],
                box1=[[int(x) for x in results[p]['box1']] for p in pairs],
                box2=[[int(x) for x in results[p]['box2']] for p in pairs],
                valid=[bool(results[p]['valid']) for p in pairs], count=[int(results[p]['count']) for p in pairs],
                scale_diff=[repr(float(x)) for x in sd], kept=[int(k) for k in kept[:n_kept]])


# ------------------------------------------------------------------ the reference's own two functions
def load_reference(ref_dir):
    """``(numpy_overlap_box, scale_diff)`` of the reference snapshot in ``ref_dir`` (``oracle/_ref``), loaded from
    their two files alone: ``cv2`` and ``h5py`` are empty stand-ins and ``src.datasets.utils`` is the loaded file, for
    the duration of the load only - ``sys.modules`` is put back as it was."""
    import importlib.util
    import sys
    import types
    from pathlib import Path
    ref_dir = Path(ref_dir)
    names = ('cv2', 'h5py', 'src', 'src.datasets', 'src.datasets.utils')
    before = {n: sys.modules.get(n) for n in names}
    try:
        for n in ('cv2', 'h5py'):
            sys.modules.setdefault(n, types.ModuleType(n))
        spec = importlib.util.spec_from_file_location('ref_datasets_utils', ref_dir / 'src' / 'datasets' / 'utils.py')
        utils = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(utils)
        for n in ('src', 'src.datasets'):
            sys.modules[n] = types.ModuleType(n)
        sys.modules['src.datasets.utils'] = utils
        spec = importlib.util.spec_from_file_location('ref_megadepth_preprocess',
                                                      ref_dir / 'src' / 'utils' / 'megadepth_preprocess.py')
        prep = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(prep)
    finally:
        for n, m in before.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return utils.numpy_overlap_box, prep.scale_diff


def reference_pair(numpy_overlap_box, views, i, j):
    """The reference's ``numpy_overlap_box`` on two views of ONE square size -> dict like ``overlap_box_hw``'s."""
    assert views[i]['depth'].shape == views[j]['depth'].shape and views[i]['depth'].shape[0] == views[i]['depth'].shape[1]
    with np.errstate(all='ignore'):
        box1, mask1, box2, _, valid = numpy_overlap_box(*view_args(views[i]), *view_args(views[j]))
    return dict(box1=np.asarray(box1, np.int64), box2=np.asarray(box2, np.int64), valid=bool(valid),
                count=int((mask1 != 0).sum()))
