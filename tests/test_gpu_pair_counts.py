"""GPU tests of the evaluation entries at pair counts their other tests never reach: past one grid of pairs (the
y extent of a launch, ``COVIS_MAX_GRID_Y`` / ``HOM_MAX_GRID_Y``, read from the kernels' sources - every pointer of the
second launch is advanced by ``p0``), past one block of the one-thread-per-pair kernels (256 pairs; 128 for
``k_keypoint_finish``, 64 for ``k_crop_batch_geometry``), and 70 000 short match lists, up to seven with rows in one
wave and no wave inside one list, under a search over 70 000 offsets.  There is no tolerance: ALL pairs and rows of every call are compared for bit equality
(``np.array_equal`` / ``mso.equal_bits``) with the float64 specifications of ``tests/*_oracle.py``, computed for a
short cycle of distinct pairs and tiled (``tests/pair_counts_cases.py``; the tiling itself is checked without a GPU in
``tests/test_pair_counts_cpu.py``).  Every margin assertion of the pinned fixtures is made where the cycle is drawn.
Each test prints its pair count, launches and wall time."""
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import match_score_oracle as mso  # noqa: E402
import pair_counts_cases as pcc  # noqa: E402

pytestmark = pytest.mark.gpu
P_COVIS, P_HOM = pcc.COVIS_MAX_GRID_Y + 3, pcc.HOM_MAX_GRID_Y + 3
# the launch boundary falls inside a cycle
assert pcc.COVIS_MAX_GRID_Y % len(pcc.COVIS_KINDS) and pcc.COVIS_MAX_GRID_Y % 72 and pcc.HOM_MAX_GRID_Y % 56
BOX_KEYS = (('overlap_box1', 'box1'), ('overlap_box2', 'box2'), ('overlap_valid', 'valid'), ('overlap_count', 'count'))


class report:
    """Prints what a test ran and how long it took (the device work is waited for)."""

    def __init__(self, name, pairs, limit=None):
        self.text = f'pair_counts: {name}: {pairs} pairs' + (f', {pcc.launches(pairs, limit)} launches' if limit else '')

    def __enter__(self):
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        print(f'{self.text}, {time.perf_counter() - self.t0:.2f} s')


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def depth_set(gpu, views, cameras=('bbox', 'ratio')):
    import imagematching_oetr_amd as pkg
    ds = pkg.DepthSet(gpu)
    for k, v in enumerate(views):
        assert ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose'], *(v[c] for c in cameras if c in v)) == k
    return ds


def assert_boxes(out, want, tag):
    """Every pair of a boxes call: the boxes as float32, valid, count."""
    for key, name in BOX_KEYS:
        got = out[key].cpu().numpy()
        exp = want[name].astype(got.dtype)
        assert got.shape == exp.shape, (tag, key, got.shape, exp.shape)
        assert np.array_equal(got, exp), (tag, key, np.flatnonzero((got != exp).reshape(len(got), -1).any(1))[:8])


# ------------------------------------------------------------------ second launches over the grid's y extent
@pytest.mark.parametrize('masks', [False, True], ids=['boxes', 'masks'])
@pytest.mark.parametrize('size', pcc.COVIS_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_covis_boxes_past_one_grid_of_pairs(gpu, size, masks):
    """``oetr_covis_boxes``: the second launch's ``depth1 + off``, ``depth2 + off``, ``params + p0 * 40``,
    ``acc + p0 * 16``, ``mask1 + off``, ``mask2 + off``; block 1 .. 256 of ``k_covis_finish``."""
    from imagematching_oetr_amd.covis import covis_boxes
    limit = pcc.COVIS_MAX_GRID_Y
    cyc, src, want = pcc.covis_call(*size, P_COVIS)
    assert len(set(want['valid'][limit - 1:limit + 3].tolist())) == 2          # valid and invalid across the boundary
    assert (cyc['margin'] >= pcc.cvo.MIN_MARGIN).all()
    with report(f'covis_boxes {size} masks={masks}', P_COVIS, limit):
        at = dev(src, gpu)
        d1, d2, params = (dev(cyc[k], gpu).index_select(0, at).contiguous() for k in ('depth1', 'depth2', 'params'))
        out = covis_boxes(d1, d2, params, masks=masks)
        assert ('overlap_mask1' in out) == masks
        assert_boxes(out, want, size)
        if masks:
            for key, name in (('overlap_mask1', 'mask1'), ('overlap_mask2', 'mask2')):
                got = out[key].cpu().numpy()
                assert got.dtype == np.uint8 and got.shape == want[name].shape
                assert np.array_equal(got, want[name]), (key, np.flatnonzero((got != want[name]).reshape(P_COVIS, -1).any(1))[:8])


def test_indexed_boxes_and_mining_past_one_grid_of_pairs(gpu):
    """``oetr_covis_boxes_indexed``: the second launch's ``idx1 + p0``, ``idx2 + p0``, ``params``, ``acc``; three
    pairs that must not be dereferenced at the boundary; then ``mine_pairs`` on the same list, uncut and cut."""
    import imagematching_oetr_amd as pkg
    limit = pcc.COVIS_MAX_GRID_Y
    views, index, bad, want = pcc.indexed_call(limit)
    P = len(index)
    assert P == P_COVIS and bad[limit - 1:limit + 2].all() and bad.sum() == 3
    kept, n_kept, sd = pcc.tiled_select(want['box1'], want['box2'], want['valid'])
    assert kept[n_kept - 1] >= limit and n_kept > 1000               # a kept pair in the second launch
    with report('overlap_boxes_indexed + mine_pairs x 2', P, limit):
        ds = depth_set(gpu, views)
        pairs = dev(index, gpu)
        out = pkg.overlap_boxes_indexed(ds, pairs)
        assert_boxes(out, want, 'indexed')
        got = out['overlap_count'].cpu().numpy()
        assert (got[bad] == -1).all() and not out['overlap_box1'].cpu().numpy()[bad].any()
        for cut in (None, n_kept - 1):                                # the cut drops the second launch's kept pair
            mined = pkg.mine_pairs(ds, pairs, limit=cut)
            assert_boxes(mined, want, ('mine', cut))
            kept, n, sd = pcc.tiled_select(want['box1'], want['box2'], want['valid'], 2.0, cut)
            assert int(mined['n_kept']) == n == (n_kept if cut is None else cut), cut
            assert np.array_equal(mined['kept'].cpu().numpy(), kept), cut
            assert mso.equal_bits(mined['scale_diff'].cpu().numpy(), sd), cut


def test_homography_boxes_past_one_grid_of_pairs(gpu):
    """``oetr_homography_boxes``: the second launch's ``params + p0 * 16`` and ``acc + p0 * 16``; every kind and
    every size pair of ``homography_oracle.make_boxes``, the grid sized by the largest picture."""
    import imagematching_oetr_amd as pkg
    limit = pcc.HOM_MAX_GRID_Y
    params, top, src, want = pcc.homography_call(P_HOM)
    assert top == (480, 640) and len(set(src[limit - 1:limit + 3].tolist())) == 4
    with report('overlap_boxes_from_homography', P_HOM, limit):
        out = pkg.overlap_boxes_from_homography(dev(params, gpu), max_size1=top)
        assert_boxes(out, want, 'homography')


# ------------------------------------------------------------------ second blocks of the one-thread-per-pair kernels
@pytest.mark.parametrize('values', [True, False], ids=['values', 'bare'])
def test_score_matches_past_one_block_of_pairs(gpu, values):
    """280 pairs: block 1 of ``k_match_finish``."""
    import imagematching_oetr_amd as pkg
    c = pcc.match_score_call()
    P = len(c['pairs'])
    assert P == 280 > 256
    with report(f'score_matches values={values}', P):
        ds = depth_set(gpu, c['views'])
        out = pkg.score_matches(ds, c['pairs'], dev(c['k1'], gpu), dev(c['k2'], gpu), lengths=c['lengths'],
                                params=c['blocks'], values=values, **c['thr'])
        assert ('values' in out) == values
        assert np.array_equal(out['flags'].cpu().numpy(), c['want']['flags'])
        assert np.array_equal(out['counts'].cpu().numpy(), c['want']['counts'])
        for k in mso.VALUES if values else ():
            assert mso.equal_bits(out[k].cpu().numpy(), c['want'][k]), k


def test_score_matches_homography_past_one_block_of_pairs(gpu):
    """264 pairs, the degenerate lists among them: 17 blocks of ``k_homography_init`` (one thread per counter, 16
    counters a pair; the 12 pinned lists fill 192 threads of block 0)."""
    import imagematching_oetr_amd as pkg
    c = pcc.homography_score_call()
    P = len(c['lengths'])
    assert P == 264 > 256
    with report('score_matches_homography', P):
        out = pkg.score_matches_homography(dev(c['params'], gpu), dev(c['k1'], gpu), dev(c['k2'], gpu), lengths=c['lengths'])
        assert mso.equal_bits(out['dist_sq'].cpu().numpy(), c['want']['dist_sq'])
        assert np.array_equal(out['counts'].cpu().numpy(), c['want']['counts'])


def test_score_keypoints_past_one_block_of_pairs(gpu):
    """144 pairs over the same 12 pictures: block 1 of ``k_keypoint_finish`` (two threads a pair) starts at 129."""
    import imagematching_oetr_amd as pkg
    c = pcc.keypoint_call()
    P = len(c['pairs'])
    assert P == 144 > 128
    with report('score_keypoints', P):
        ds = depth_set(gpu, c['views'])
        out = pkg.score_keypoints(ds, c['pairs'], [dev(k, gpu) for k in c['kps']], c['thr'], params=c['blocks'])
        assert tuple(out['nearest'].shape) == (P, 2, c['max_kp'])
        for k in ('counts', 'nearest', 'dist_sq'):
            assert mso.equal_bits(out[k].cpu().numpy(), c['want'][k]), k


def test_estimate_poses_past_one_block_of_pairs(gpu):
    """272 pairs, ``pair_ids = p % 16``: every copy draws the samples of its pinned list."""
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd.pose_ransac import workspace_views
    c = pcc.pose_call()
    P = len(c['lengths'])
    assert P == 272 > 256
    with report('estimate_poses', P):
        out = pkg.estimate_poses(dev(c['blocks'], gpu), dev(c['k1'], gpu), dev(c['k2'], gpu), lengths=c['lengths'],
                                 n_hyp=c['n_hyp'], seed=c['seed'], pair_ids=dev(c['pair_ids'], gpu))
        models, model_counts = workspace_views(out)
        got = dict(models=models, model_counts=model_counts, **{k: out[k] for k in ('model', 'pose', 'cosines', 'counts', 'inliers')})
        for k, v in got.items():
            assert mso.equal_bits(v.cpu().numpy(), c['want'][k]), k


def test_overlap_crop_batch_past_one_block_of_pairs(gpu):
    """70 pairs of one mode in one call: block 1 of ``k_crop_batch_geometry`` (64 threads) starts at pair 64.  Pair k
    is the per-pair ``overlap_crop`` of its case, record fields and pixels, bit for bit."""
    import imagematching_oetr_amd as pkg
    from tests.test_gpu_crop_batch import fuzz_cases, image, info_fields
    groups = {}
    for case in fuzz_cases():
        groups.setdefault(case['mode'], []).append(case)
    (keep, div, pp), cases = max(groups.items(), key=lambda kv: len(kv[1]))
    P = 70
    assert 64 % len(cases) and len(cases) >= 5
    with report(f'overlap_crop_batch mode={(keep, div, pp)}, {len(cases)} distinct', P):
        ims = [(image(c['hw0']).to(gpu), image(c['hw1']).to(gpu)) for c in cases]
        ones = [pkg.overlap_crop(ims[n][0], ims[n][1], c['b0'].to(gpu), c['b1'].to(gpu), c['sc0'], c['sc1'], keep, div, pp)
                for n, c in enumerate(cases)]
        src = [p % len(cases) for p in range(P)]
        table = pkg.crop_pair_table([ims[n][0] for n in src], [ims[n][1] for n in src], [cases[n]['sc0'] for n in src],
                                    [cases[n]['sc1'] for n in src])
        box0 = torch.stack([cases[n]['b0'] for n in src]).to(gpu)
        box1 = torch.stack([cases[n]['b1'] for n in src]).to(gpu)
        batch = pkg.overlap_crop_batch(table, box0, box1, keep_aspect=keep, size_divisor=div, pragueparks=pp)
        geometry = batch.geometry()
        assert len(batch) == len(geometry) == P
        wants = [info_fields(one.geometry()) for one in ones]
        assert any(w['valid'] > 0 for w in wants)
        for p, n in enumerate(src):
            assert info_fields(geometry[p]) == wants[n], (p, n)
            if wants[n]['valid'] < 0:
                continue
            for side in (0, 1):
                assert torch.equal(batch.crop(p, side), ones[n].crop(side)), (p, n, side)


# ------------------------------------------------------------------ many short lists in one wave
def test_score_matches_over_many_short_lists(gpu):
    """70 000 lists of 0 .. 64 rows: the per-lane search over 70 001 offsets and the per-lane atomics of
    ``match_list.h``, pairs alternating between two combinations of maps."""
    import imagematching_oetr_amd as pkg
    c = pcc.short_match_call()
    P, M = len(c['pairs']), len(c['owner'])
    assert P == 70000 and M > 600000 and (c['owner'][:pcc.SHORT_BEFORE] == -1).all() and (c['owner'][-pcc.SHORT_AFTER:] == -1).all()
    with report(f'score_matches, {M} rows in short lists', P):
        ds = depth_set(gpu, c['views'])
        out = pkg.score_matches(ds, dev(c['pairs'], gpu), dev(c['k1'], gpu), dev(c['k2'], gpu), offsets=dev(c['offsets'], gpu),
                                params=dev(c['blocks'], gpu), **c['thr'])
        flags = out['flags'].cpu().numpy()
        assert np.array_equal(flags, c['want']['flags']), np.flatnonzero(flags != c['want']['flags'])[:8]
        for k in mso.VALUES:
            assert mso.equal_bits(out[k].cpu().numpy(), c['want'][k]), k
        counts = out['counts'].cpu().numpy()
        assert np.array_equal(counts, c['want']['counts']), np.flatnonzero((counts != c['want']['counts']).any(1))[:8]
        outside = c['owner'] < 0                                    # rows outside every list are left unscored
        assert np.array_equal(np.isnan(out['episym'].cpu().numpy()) & (flags == 0), outside)


def test_score_matches_homography_over_many_short_lists(gpu):
    import imagematching_oetr_amd as pkg
    c = pcc.short_homography_call()
    P, M = len(c['params']), len(c['owner'])
    assert P == 70000 and M > 600000
    with report(f'score_matches_homography, {M} rows in short lists', P):
        out = pkg.score_matches_homography(dev(c['params'], gpu), dev(c['k1'], gpu), dev(c['k2'], gpu),
                                           offsets=dev(c['offsets'], gpu), thresholds=pcc.SHORT_HOM_THRESHOLDS)
        dist_sq = out['dist_sq'].cpu().numpy()
        assert mso.equal_bits(dist_sq, c['want']['dist_sq']), np.flatnonzero(dist_sq != c['want']['dist_sq'])[:8]
        counts = out['counts'].cpu().numpy()
        assert np.array_equal(counts, c['want']['counts']), np.flatnonzero((counts != c['want']['counts']).any(1))[:8]
        assert np.array_equal(np.isnan(dist_sq), c['owner'] < 0)
