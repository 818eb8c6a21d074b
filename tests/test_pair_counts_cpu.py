"""The tiled calls of ``tests/pair_counts_cases.py`` are code too: their expected arrays are checked here, without a
GPU, against the float64 specifications run DIRECTLY on the tiled calls' own inputs - on the pairs around the boundary
(the grid's y extent, or pair 256 / 128 of the one-thread-per-pair kernels) and on one full cycle - and, for the
many-short-lists calls, against ``score_lists`` / ``score`` on a 200-list slice."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_set_oracle as cso  # noqa: E402
import homography_oracle as hmo  # noqa: E402
import keypoint_score_oracle as kso  # noqa: E402
import match_score_oracle as mso  # noqa: E402
import pair_counts_cases as pcc  # noqa: E402
import pose_ransac_oracle as pro  # noqa: E402


def rows_to_check(boundary, cycle_length, n):
    """One full cycle and the pairs around the boundary."""
    return sorted(set(range(cycle_length)) | {p for p in range(boundary - 3, boundary + 4) if 0 <= p < n})


def test_grid_limits_are_read_from_the_sources_and_cut_inside_a_cycle():
    assert pcc.COVIS_MAX_GRID_Y == pcc.HOM_MAX_GRID_Y == 65535          # the y extent of a HIP grid
    assert pcc.COVIS_MAX_GRID_Y % len(pcc.COVIS_KINDS) != 0 and pcc.COVIS_MAX_GRID_Y % 72 != 0
    assert pcc.HOM_MAX_GRID_Y % len(pcc.homography_boxes()) != 0
    assert pcc.launches(pcc.COVIS_MAX_GRID_Y + 3, pcc.COVIS_MAX_GRID_Y) == 2 == pcc.launches(65536, 65535)
    assert pcc.launches(65535, 65535) == 1
    assert set(pcc.COVIS_KINDS) == set(pcc.cvo.KINDS) and len(pcc.COVIS_KINDS) == 7


def test_stacked_covis_call_is_the_restatement_of_its_own_inputs():
    limit = pcc.COVIS_MAX_GRID_Y
    P = limit + 3
    for h, w in pcc.COVIS_SIZES:
        cyc, src, want = pcc.covis_call(h, w, P)
        assert cyc['valid'].any() and not cyc['valid'].all() and (cyc['margin'] >= pcc.cvo.MIN_MARGIN).all()
        assert all(want[k].shape[0] == P for k in want)
        for p in rows_to_check(limit, len(pcc.COVIS_KINDS), P):
            res = pcc.covis_from_block(cyc['depth1'][src[p]], cyc['depth2'][src[p]], cyc['params'][src[p]])
            assert np.array_equal(want['box1'][p], res['box1'].astype(np.float32)), (h, w, p)
            assert np.array_equal(want['box2'][p], res['box2'].astype(np.float32)), (h, w, p)
            assert bool(want['valid'][p]) == res['valid'] and int(want['count'][p]) == res['count'], (h, w, p)
            assert np.array_equal(want['mask1'][p], res['mask1']) and np.array_equal(want['mask2'][p], res['mask2'])


def test_indexed_call_and_its_selection_are_the_restatement_of_their_own_inputs():
    limit = pcc.COVIS_MAX_GRID_Y
    views, index, bad, want = pcc.indexed_call(limit)
    P = len(index)
    assert P == limit + 3 and np.flatnonzero(bad).tolist() == [limit - 1, limit, limit + 1]
    for p in rows_to_check(limit, 72, P):
        i, j = (int(v) for v in index[p])
        if bad[p]:
            assert not (0 <= i < len(views) and 0 <= j < len(views))
            assert int(want['count'][p]) == -1 and not want['valid'][p] and not want['box1'][p].any() and not want['box2'][p].any()
            continue
        res = cso.restate_pair(views, i, j)
        assert res['margin'] >= cso.MIN_MARGIN
        assert np.array_equal(want['box1'][p], res['box1']) and np.array_equal(want['box2'][p], res['box2']), p
        assert bool(want['valid'][p]) == res['valid'] and int(want['count'][p]) == res['count'], p
    # the criterion evaluated once per distinct row and tiled IS covis_set_oracle.select on the whole list
    kept, n_kept, sd = cso.select(want['box1'], want['box2'], want['valid'], 2.0)
    assert kept[n_kept - 1] >= limit
    for cut, ref in ((None, (kept, n_kept, sd)), (n_kept - 1, cso.select(want['box1'], want['box2'], want['valid'], 2.0, n_kept - 1))):
        mine = pcc.tiled_select(want['box1'], want['box2'], want['valid'], 2.0, cut)
        assert mine[1] == ref[1] and np.array_equal(mine[0], ref[0]) and mso.equal_bits(mine[2], ref[2]), cut
    assert n_kept - 1 == int((kept[:n_kept] < limit).sum())             # that cut drops the second launch's kept pair


def test_homography_boxes_call_is_the_restatement_of_its_own_inputs():
    limit = pcc.HOM_MAX_GRID_Y
    P = limit + 3
    params, top, src, want = pcc.homography_call(P)
    assert params.shape == (P, 16) and top == (480, 640)
    assert {b['kind'] for b in pcc.homography_boxes()} == set(hmo.KINDS)
    for p in rows_to_check(limit, 56, P):
        b = params[p]
        assert b[10] <= top[0] and b[9] <= top[1]
        res = hmo.overlap_box(b[0:9].reshape(3, 3), b[9], b[10], b[11], b[12])
        assert res['margin'] >= pcc.cvo.MIN_MARGIN
        assert np.array_equal(want['box1'][p], res['box1'].astype(np.float32)), p
        assert np.array_equal(want['box2'][p], res['box2'].astype(np.float32)), p
        assert bool(want['valid'][p]) == res['valid'] and int(want['count'][p]) == res['count'], p


def test_tiled_match_score_call_is_the_specification_of_its_own_inputs():
    c = pcc.match_score_call()
    bounds = np.concatenate([[0], np.cumsum(c['lengths'])])
    P = len(c['pairs'])
    assert P == 280 and bounds[-1] == len(c['k1']) == len(c['want']['flags']) == 2610 * 20
    for p in rows_to_check(256, 14, P):
        (i, j), lo, hi = c['pairs'][p], bounds[p], bounds[p + 1]
        res = mso.score(c['views'][i]['depth'], c['views'][j]['depth'], c['blocks'][p], c['k1'][lo:hi], c['k2'][lo:hi], **c['thr'])
        assert np.array_equal(c['want']['flags'][lo:hi], res['flags']) and np.array_equal(c['want']['counts'][p], res['counts']), p
        for k in mso.VALUES:
            assert mso.equal_bits(c['want'][k][lo:hi], res[k]), (p, k)


def test_tiled_homography_score_call_is_the_specification_of_its_own_inputs():
    c = pcc.homography_score_call()
    bounds = np.concatenate([[0], np.cumsum(c['lengths'])])
    P = len(c['lengths'])
    assert P == 264 and bounds[-1] == len(c['k1']) == len(c['want']['dist_sq'])
    for p in rows_to_check(256, 12, P):
        lo, hi = bounds[p], bounds[p + 1]
        res = hmo.score(c['params'][p][:9], c['k1'][lo:hi], c['k2'][lo:hi])
        assert mso.equal_bits(c['want']['dist_sq'][lo:hi], res['dist_sq']), p
        assert np.array_equal(c['want']['counts'][p], res['counts']), p


def test_tiled_keypoint_call_is_the_specification_of_its_own_inputs():
    c = pcc.keypoint_call()
    P = len(c['pairs'])
    assert P == 144 and c['max_kp'] == 600 and c['want']['nearest'].shape == (P, 2, 600)
    for p in sorted(set(range(0, 48, 5)) | set(range(125, 132)) | {P - 1}):
        i, j = c['pairs'][p]
        res = kso.score(c['views'][i]['depth'], c['views'][j]['depth'], c['blocks'][p], c['kps'][i], c['kps'][j], c['thr'])
        counts, nearest, dist_sq = kso.padded([res], c['max_kp'])
        assert np.array_equal(c['want']['counts'][p], counts[0]) and np.array_equal(c['want']['nearest'][p], nearest[0]), p
        assert mso.equal_bits(c['want']['dist_sq'][p], dist_sq[0]), p


def test_tiled_pose_call_is_the_specification_of_its_own_inputs():
    c = pcc.pose_call()
    bounds = np.concatenate([[0], np.cumsum(c['lengths'])])
    P = len(c['lengths'])
    assert P == 272 and c['n_hyp'] == 1 and c['pair_ids'].tolist() == [p % 16 for p in range(P)]
    for p in rows_to_check(256, 16, P):
        lo, hi = bounds[p], bounds[p + 1]
        res = pro.estimate(c['blocks'][p], c['k1'][lo:hi], c['k2'][lo:hi], c['n_hyp'], c['seed'], pair_id=int(c['pair_ids'][p]))
        for k in ('models', 'model_counts', 'model', 'pose', 'cosines', 'counts'):
            assert mso.equal_bits(np.asarray(c['want'][k][p]), np.asarray(res[k])), (p, k)
        assert np.array_equal(c['want']['inliers'][lo:hi], res['inliers']), p


def test_short_lists_counters_equal_score_lists_on_a_slice():
    c = pcc.short_match_call()
    offsets, owner, want = c['offsets'], c['owner'], c['want']
    P = len(c['pairs'])
    assert P == pcc.SHORT_LISTS and np.diff(offsets)[:8].tolist() == list(pcc.SHORT_LENGTHS)
    assert offsets[0] == pcc.SHORT_BEFORE and len(owner) == offsets[-1] + pcc.SHORT_AFTER
    waves = owner[:len(owner) // 64 * 64].reshape(-1, 64)
    in_a_wave = (np.diff(waves, axis=1) != 0).sum(1) + 1               # lists with a row in the wave (owners ascend)
    assert in_a_wave.min() >= 2 and in_a_wave.max() >= 7                # every wave straddles lists: the per-lane path
    first = 34001                                                      # an odd start: both combinations, every length
    pairs = [tuple(int(v) for v in pr) for pr in c['pairs'][first:first + 200]]
    lists = [(c['k1'][offsets[p]:offsets[p + 1]], c['k2'][offsets[p]:offsets[p + 1]]) for p in range(first, first + 200)]
    results = mso.score_lists(c['views'], pairs, lists, blocks=c['blocks'][first:first + 200], **c['thr'])
    assert {len(a) for a, _ in lists} == set(pcc.SHORT_LENGTHS) and set(pairs) == set(pcc.SHORT_COMBOS)
    for n, res in enumerate(results):
        p = first + n
        lo, hi = offsets[p], offsets[p + 1]
        assert np.array_equal(want['counts'][p], res['counts']), p
        assert np.array_equal(want['flags'][lo:hi], res['flags']), p
        for k in mso.VALUES:
            assert mso.equal_bits(want[k][lo:hi], res[k]), (p, k)
    outside = owner < 0
    assert outside.sum() == pcc.SHORT_BEFORE + pcc.SHORT_AFTER and np.isnan(want['episym'][outside]).all()
    assert not want['flags'][outside].any() and not np.isnan(want['episym'][~outside]).any()
    assert want['counts'][:, 1:].max() > 10 and (want['counts'][:, 0] == np.resize(pcc.SHORT_LENGTHS, P)).all()


def test_short_homography_lists_counters_equal_score_on_a_slice():
    c = pcc.short_homography_call()
    offsets, owner, want = c['offsets'], c['owner'], c['want']
    first = 51003
    for p in range(first, first + 200):
        lo, hi = offsets[p], offsets[p + 1]
        res = hmo.score(c['params'][p][:9], c['k1'][lo:hi], c['k2'][lo:hi], pcc.SHORT_HOM_THRESHOLDS)
        assert np.array_equal(want['counts'][p], res['counts']), p
        assert mso.equal_bits(want['dist_sq'][lo:hi], res['dist_sq']), p
    assert not np.array_equal(c['params'][first], c['params'][first + 1])
    assert np.array_equal(np.isnan(want['dist_sq']), owner < 0)
    assert want['counts'].shape == (pcc.SHORT_LISTS, 1 + len(pcc.SHORT_HOM_THRESHOLDS)) and want['counts'][:, 1].sum() > 1000
