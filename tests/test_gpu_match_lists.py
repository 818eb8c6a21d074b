"""GPU test of the match-list seam (``csrc/match_list.h``): ``oetr_match_score`` and ``oetr_homography_match_score``
must give one call's rows the same list membership.  One ``offsets`` tensor whose lists start and end where a wave (64
rows) starts in one list and ends in another, or starts outside every list - lengths 0, 1, 63, 64, 65, 255, 256, 257, 0
with 70 rows before the first list and 67 after the last, 1098 rows - is scored by both entries; the rows each leaves
unscored must be exactly the rows ``numpy.searchsorted`` puts outside every list.  The keypoints are finite and the
restatement (``tests/match_score_oracle.py::score``) gives every in-list row a finite ``episym`` (asserted first), so
a NaN means "no list" and nothing else."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import match_score_oracle as mso  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 0)
BEFORE, AFTER = 70, 67
SIZES = ((40, 64), (56, 56))


def make_call(seed=0):
    """-> (views, pairs, offsets int32 [P+1], k1, k2 float32 [M,2], the list of every row or -1)."""
    views = mso.make_scene(SIZES, seed, behind=None)
    pairs = [(p % 2, 1 - p % 2) for p in range(len(LENGTHS))]
    offsets = (BEFORE + np.concatenate([[0], np.cumsum(LENGTHS)])).astype(np.int32)
    M = int(offsets[-1]) + AFTER
    parts = [mso.make_matches(views, 0, 1, BEFORE, seed=901)]
    parts += [mso.make_matches(views, i, j, n, seed=910 + p) for p, ((i, j), n) in enumerate(zip(pairs, LENGTHS))]
    parts.append(mso.make_matches(views, 1, 0, AFTER, seed=902))
    k1, k2 = (np.concatenate([part[side] for part in parts]).astype(np.float32) for side in (0, 1))
    assert k1.shape == k2.shape == (M, 2) and M < 1200
    owner = np.searchsorted(offsets, np.arange(M), 'right') - 1
    owner[(owner < 0) | (owner >= len(LENGTHS))] = -1
    return views, pairs, offsets, k1, k2, owner


def test_both_entries_give_rows_the_same_lists(gpu):
    import imagematching_oetr_amd as pkg
    views, pairs, offsets, k1, k2, owner = make_call()
    P, M = len(pairs), len(owner)
    assert [int((owner == p).sum()) for p in range(P)] == list(LENGTHS)
    assert (owner[:BEFORE] == -1).all() and (owner[M - AFTER:] == -1).all() and int((owner == -1).sum()) == BEFORE + AFTER
    # the inputs first: a NaN of the device must not be a NaN of the arithmetic
    assert np.isfinite(k1).all() and np.isfinite(k2).all()
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in pairs])
    for p, (i, j) in enumerate(pairs):
        rows = owner == p
        want = mso.score(views[i]['depth'], views[j]['depth'], blocks[p], k1[rows], k2[rows])
        assert np.isfinite(want['episym']).all(), p

    ds = pkg.DepthSet(gpu)
    for k, v in enumerate(views):
        assert ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose']) == k
    dk1, dk2, doff = (torch.from_numpy(a).to(gpu) for a in (k1, k2, offsets))
    hom = pkg.score_matches_homography(np.tile(np.eye(3), (P, 1, 1)), dk1, dk2, offsets=doff, thresholds=(1, 3))
    dep = pkg.score_matches(ds, pairs, dk1, dk2, offsets=doff, params=blocks)
    torch.cuda.synchronize()

    assert hom['counts'][:, 0].cpu().tolist() == list(LENGTHS)
    assert dep['counts'][:, 0].cpu().tolist() == list(LENGTHS)
    outside = owner == -1
    dist_sq, episym, flags = hom['dist_sq'].cpu().numpy(), dep['episym'].cpu().numpy(), dep['flags'].cpu().numpy()
    assert np.array_equal(np.isnan(dist_sq), outside), np.flatnonzero(np.isnan(dist_sq) != outside)
    unscored = np.isnan(episym) & (flags == 0)
    assert np.array_equal(unscored, outside), np.flatnonzero(unscored != outside)
    assert np.array_equal(np.isnan(episym), outside)                 # and no scored row of this call is NaN at all
