"""GPU test of the sharing itself: ``oetr_keypoint_repeatability`` and ``oetr_match_score`` project a keypoint through
ONE copy of the depth read and of the two projections (``csrc/depth_pose.h``), so the same keypoints scored through
both entries give the same bits.  ``score_keypoints`` finds, for every kept keypoint, its nearest partner and the squared
distance to it; the match list (keypoint, partner) goes through ``score_matches``, whose ``reproj12_sq`` / ``reproj21_sq``
are that very distance - ``(pu - u) * (pu - u) + (pv - v) * (pv - v)`` in both kernels.  No tolerance: bit for bit.

The smallest shape that can go wrong: two maps of different sizes (8 x 10 and 12 x 6), the pair and its reverse, 100
keypoints per picture (more than one wave), among them ``match_score_oracle.special_points`` (``.5`` ties, the edges,
+-inf, NaN) and random points a little outside the map."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import keypoint_score_oracle as kso  # noqa: E402
import match_score_oracle as mso  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES, SEED, N_KP = ((8, 10), (12, 6)), 1, 100
PAIRS = ((0, 1), (1, 0))


def make_inputs():
    """-> (views, keypoint sets float32 [100,2], parameter blocks float64 [2,20])."""
    views = mso.make_scene(SIZES, SEED, behind=None)
    rng = np.random.default_rng(SEED)
    kps = []
    for v in views:
        h, w = v['depth'].shape
        anywhere = np.stack([rng.uniform(-2, w + 2, N_KP - 16), rng.uniform(-2, h + 2, N_KP - 16)], 1)
        kps.append(np.concatenate([mso.off_tie(anywhere), mso.special_points((h, w))]).astype(np.float32))
    return views, kps, np.stack([mso.pair_block(views, i, j) for i, j in PAIRS])


def test_both_entries_give_one_keypoint_the_same_bits(gpu):
    import imagematching_oetr_amd as pkg
    views, kps, blocks = make_inputs()
    # the restatement alone keeps at least a quarter of every direction's rows: the comparison below is not empty
    for p, (i, j) in enumerate(PAIRS):
        for res in kso.score(views[i]['depth'], views[j]['depth'], blocks[p], kps[i], kps[j]):
            assert 4 * int(res['kept'].sum()) >= N_KP, (p, int(res['kept'].sum()))
    ds = pkg.DepthSet(gpu)
    for v in views:
        ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose'])
    out = pkg.score_keypoints(ds, list(PAIRS), kps, nearest=True, params=blocks)
    nearest, dist_sq = out['nearest'].cpu().numpy(), out['dist_sq'].cpu().numpy()
    assert nearest.shape == (2, 2, N_KP)

    # list 2 p + s: the kept rows of direction s of pair p, each with its nearest partner, as matches of pair p
    index, k1, k2, rows = [], [], [], []
    for p, (i, j) in enumerate(PAIRS):
        for s in range(2):
            src = np.flatnonzero(nearest[p, s] >= 0)
            assert 4 * len(src) >= N_KP, (p, s, len(src))
            partner = nearest[p, s, src]
            a, b = (src, partner) if s == 0 else (partner, src)         # a: rows of picture i, b: of picture j
            index.append((i, j))
            k1.append(kps[i][a])
            k2.append(kps[j][b])
            rows.append(src)
    scored = pkg.score_matches(ds, index, np.concatenate(k1), np.concatenate(k2), lengths=[len(r) for r in rows],
                               params=np.repeat(blocks, 2, axis=0))
    reproj = {0: scored['reproj12_sq'].cpu().numpy(), 1: scored['reproj21_sq'].cpu().numpy()}
    at = 0
    for n, src in enumerate(rows):
        p, s = divmod(n, 2)
        assert mso.equal_bits(reproj[s][at:at + len(src)], dist_sq[p, s, src]), (p, s)
        at += len(src)
