"""GPU tests of the pose-refit extension (``oetr_pose_refit``, ``csrc/pose_refit.hip``; ``pose_refit.py``;
``evaluate.pose_errors`` / ``match_pose_auc`` on its result).  There is no tolerance anywhere: every output -
``model``, ``pose``, ``cosines``, ``counts``, ``inliers`` - is compared BIT FOR BIT (``mso.equal_bits``: NaN equals NaN
whatever its payload) with the float64 specification ``tests/pose_refit_oracle.py``, whose pinned lists keep every
inlier and cheirality decision away from last-bit differences (asserted in ``tests/test_pose_refit_cpu.py``, where
the same arithmetic compiled for the host equals the specification).  The device's float64 square root is pinned by
``tests/test_gpu_pose_ransac.py``.  The fixture is 16 lists, 3557 matches."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import match_score_oracle as mso  # noqa: E402
import pose_ransac_oracle as pro  # noqa: E402
import pose_refit_oracle as pfo  # noqa: E402

pytestmark = pytest.mark.gpu
EXPECTED = json.loads((REPO / 'tests' / 'pose_refit_expected.json').read_text())
KEYS = ('model', 'pose', 'cosines', 'counts', 'inliers')


def host(out):
    return {k: out[k].cpu().numpy() for k in KEYS if k in out}


def assert_pairs(got, wants, bounds, tag=None):
    """Every pair of a call against its specified result, by bits."""
    for p, want in enumerate(wants):
        lo, hi = int(bounds[p]), int(bounds[p + 1])
        for k in ('model', 'pose', 'cosines'):
            assert mso.equal_bits(got[k][p], want[k]), (tag, p, k, got[k][p], want[k])
        assert got['counts'][p].tolist() == want['counts'].tolist(), (tag, p, got['counts'][p], want['counts'])
        if 'inliers' in got:
            assert np.array_equal(got['inliers'][lo:hi], want['inliers']), (tag, p, 'inliers')


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert mso.equal_bits(a[k], b[k]), k


def joined(lists):
    return np.concatenate([a for a, _ in lists]), np.concatenate([b for _, b in lists])


@pytest.fixture(scope='module')
def pinned(gpu):
    """The pinned lists, the two sets of ``model_in``, their specified results per source and ``refit_iters`` and the
    device inputs: made once, shared, never modified."""
    rec = EXPECTED['pinned']
    blocks, lists, models, _ = pfo.pinned_call(rec['draws'])
    assert [cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists] == rec['kpts_sha256']
    assert cvo.sha(blocks) == rec['blocks_sha256']                       # a wrong input cannot pass as a wrong kernel
    assert {s: cvo.sha(np.nan_to_num(models[s], nan=-7.0)) for s in pfo.PINNED_SOURCES} == rec['models_sha256']
    lengths = [len(k1) for k1, _ in lists]
    k1, k2 = joined(lists)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    wants = {(s, r): pfo.refit_lists(blocks, lists, models[s], 1.0, r)
             for s in pfo.PINNED_SOURCES for r in pfo.PINNED_REFITS}
    return dict(blocks=blocks, lists=lists, lengths=lengths, bounds=np.concatenate([[0], np.cumsum(lengths)]),
                params=t(blocks), k1=t(k1), k2=t(k2), host_k=(k1, k2), models=models,
                dmodels={s: t(models[s]) for s in pfo.PINNED_SOURCES}, wants=wants)


@pytest.mark.parametrize('refit_iters', pfo.PINNED_REFITS)
@pytest.mark.parametrize('source', pfo.PINNED_SOURCES)
def test_pinned_call_equals_the_specification_and_the_fixture(gpu, pinned, source, refit_iters):
    import imagematching_oetr_amd as pkg
    assert pinned['lengths'][:11] == [0, 7, 8, 9, 63, 64, 65, 255, 256, 257, 600] and len(pinned['lengths']) == 16
    out = pkg.refine_poses(pinned['params'], pinned['k1'], pinned['k2'], pinned['dmodels'][source],
                           lengths=pinned['lengths'], refit_iters=refit_iters)
    M = int(pinned['bounds'][-1])
    assert out['model'].dtype == torch.float64 and out['model'].shape == (16, 9) and out['model'].is_cuda
    assert out['pose'].shape == (16, 12) and out['cosines'].shape == (16, 2)
    assert out['counts'].dtype == torch.int32 and out['counts'].shape == (16, 5)
    assert out['inliers'].dtype == torch.uint8 and out['inliers'].shape == (M,)
    got = host(out)
    wants = pinned['wants'][source, refit_iters]
    assert_pairs(got, wants, pinned['bounds'], (source, refit_iters))
    records = EXPECTED['pinned']['records'][source][str(refit_iters)]
    sha, z = (lambda a: cvo.sha(a)[:16]), (lambda a: np.nan_to_num(a, nan=-7.0))
    assert got['counts'].tolist() == [rec['counts'] for rec in records]
    for p, rec in enumerate(records):
        lo, hi = pinned['bounds'][p], pinned['bounds'][p + 1]
        assert sha(z(got['model'][p])) == rec['model'] and sha(z(got['pose'][p])) == rec['pose'], p
        assert sha(z(got['cosines'][p])) == rec['cosines'] and sha(got['inliers'][lo:hi]) == rec['inliers'], p
    # the list of 0 rows: no pose
    assert got['counts'][0].tolist() == [0, 0, -1, 0, 0]
    assert np.isnan(got['model'][0]).all() and np.isnan(got['pose'][0]).all() and np.isnan(got['cosines'][0]).all()
    assert (got['counts'][:, 3] >= got['counts'][:, 1]).all() and (got['counts'][:, 2] <= refit_iters).all()
    # the summaries take the result as it is and equal the specification's
    errs = pkg.pose_errors(out)
    spec = pro.pose_errors(np.stack([w['cosines'] for w in wants]), np.stack([w['counts'] for w in wants]))
    for k, want in zip(('err_R', 'err_t', 'pose_error'), spec):
        assert mso.equal_bits(errs[k], want), k
    assert np.isinf(errs['pose_error'][0]) and np.isfinite(errs['pose_error'][2:]).all()
    auc = pkg.match_pose_auc(out)
    assert auc['auc'] == [100.0 * a for a in pro.pose_auc(spec[2])] and auc['n_no_pose'] == int(np.isinf(spec[2]).sum())
    assert [a / 100.0 for a in auc['auc']] == pytest.approx(EXPECTED['pinned']['summaries'][source][str(refit_iters)]['auc'],
                                                            abs=1e-15)


def test_estimates_model_straight_into_the_refit(gpu, pinned):
    """``estimate_poses(...)['model']`` handed on as it is, with device offsets and rows in no list before the first
    and after the last list, into a reused ``out`` filled with garbage; ``refit_iters=0`` gives ``estimate_poses``' own
    ``pose`` / ``cosines`` / ``inliers`` / ``counts[3:]`` bit for bit."""
    import imagematching_oetr_amd as pkg
    head, tail = 70, 67
    filler = lambda m: torch.full((m, 2), 3.0, device=gpu)
    k1 = torch.cat([filler(head), pinned['k1'], filler(tail)])
    k2 = torch.cat([filler(head), pinned['k2'], filler(tail)])
    offsets = torch.from_numpy((pinned['bounds'] + head).astype(np.int32)).to(gpu)
    est = pkg.estimate_poses(pinned['params'], k1, k2, offsets=offsets, n_hyp=pfo.PINNED_HYPOTHESES, seed=pfo.PINNED_SEED)
    assert mso.equal_bits(est['model'].cpu().numpy(), pinned['models']['estimate'])
    out = pkg.refine_poses(pinned['params'], k1, k2, est['model'], offsets=offsets, refit_iters=2)
    for k in KEYS:
        out[k].fill_(9 if k == 'inliers' else -5)
    again = pkg.refine_poses(pinned['params'], k1, k2, est['model'], offsets=offsets, refit_iters=4, out=out)
    assert again is out
    got = host(out)
    assert not got['inliers'][:head].any() and not got['inliers'][-tail:].any()
    got['inliers'] = got['inliers'][head:-tail]
    assert_pairs(got, pinned['wants']['estimate', 4], pinned['bounds'], 'straight')
    with pytest.raises(ValueError, match='other sizes'):
        pkg.refine_poses(pinned['params'], k1, k2, est['model'], offsets=offsets, inliers=False, out=out)
    with pytest.raises(ValueError, match='overlap'):
        pkg.refine_poses(pinned['params'], k1, k2, out['model'], offsets=offsets, out=out)
    # no round: the tail of estimate_poses
    zero, e = host(pkg.refine_poses(pinned['params'], k1, k2, est['model'], offsets=offsets, refit_iters=0)), host(est)
    assert_same(zero, e, ('model', 'pose', 'cosines', 'inliers'))
    assert np.array_equal(zero['counts'][:, 3:], e['counts'][:, 3:]) and np.array_equal(zero['counts'][:, 0], e['counts'][:, 0])
    posed = e['counts'][:, 2] >= 0
    assert np.array_equal(zero['counts'][:, 2] >= 0, posed) and (zero['counts'][posed, 2] == 0).all()
    assert np.array_equal(zero['counts'][:, 1], e['counts'][:, 3])


def test_host_inputs_no_inliers_float16_and_another_threshold(gpu, pinned):
    import imagematching_oetr_amd as pkg
    full = host(pkg.refine_poses(pinned['params'], pinned['k1'], pinned['k2'], pinned['dmodels']['estimate'],
                                 lengths=pinned['lengths']))
    assert_pairs(full, pinned['wants']['estimate', 4], pinned['bounds'], 'default refit_iters')
    # host arrays, uploaded
    got = host(pkg.refine_poses(pinned['blocks'], *pinned['host_k'], pinned['models']['estimate'],
                                lengths=pinned['lengths']))
    assert_same(got, full)
    # inliers=False: the same everything else
    bare = pkg.refine_poses(pinned['params'], pinned['k1'], pinned['k2'], pinned['dmodels']['estimate'],
                            lengths=pinned['lengths'], inliers=False)
    assert 'inliers' not in bare
    assert_same(host(bare), full, ('model', 'pose', 'cosines', 'counts'))
    # float16 keypoints are widened exactly
    h1, h2 = pinned['k1'].half(), pinned['k2'].half()
    a = host(pkg.refine_poses(pinned['params'], h1, h2, pinned['dmodels']['true'], lengths=pinned['lengths']))
    b = host(pkg.refine_poses(pinned['params'], h1.float(), h2.float(), pinned['dmodels']['true'],
                              lengths=pinned['lengths']))
    assert_same(a, b)
    # another threshold, eight rounds: two lists of the noisy scenes of the CPU tests
    scenes = [pro.noisy_scene(1, 0.3), pro.noisy_scene(4, 0.6)]
    blocks = np.stack([s[0] for s in scenes])
    lists = [s[1:] for s in scenes]
    models = np.stack([pro.estimate(P, a, b, 64, 1, 2.5, i)['model'] for i, (P, a, b) in enumerate(scenes)])
    wants = pfo.refit_lists(blocks, lists, models, 2.5, 8)
    assert all(pfo.margins_hold(w) for w in wants) and any(w['counts'][2] > 0 for w in wants)
    got = host(pkg.refine_poses(blocks, *joined(lists), models, lengths=[150, 150], px_thr=2.5, refit_iters=8))
    assert_pairs(got, wants, [0, 150, 300], 'px_thr')


def test_refusals_and_edges_in_one_call(gpu):
    """Fewer than 8 inliers, an EXACT zero pivot, a rejected candidate, a NaN ``model_in``, a list of 0 rows, a tie of
    the held entry: one call, each list its own specified result."""
    import imagematching_oetr_amd as pkg
    cases = pfo.edge_cases()
    names = list(cases)
    assert set(names) == {'few', 'zero_pivot', 'rejected', 'nan', 'empty', 'tie'}
    assert {cases[n][4] for n in names} == {1.0}
    blocks = np.stack([cases[n][0] for n in names])
    lists = [cases[n][1:3] for n in names]
    models = np.stack([cases[n][3] for n in names])
    lengths = [len(a) for a, _ in lists]
    wants = [pfo.refit(*cases[n][:4], 1.0, 4) for n in names]
    got = host(pkg.refine_poses(blocks, *joined(lists), models, lengths=lengths, refit_iters=4))
    assert_pairs(got, wants, np.concatenate([[0], np.cumsum(lengths)]), names)
    for p, n in enumerate(names):
        assert got['counts'][p].tolist() == EXPECTED['edges'][n]['counts'], n
        if n in ('nan', 'empty'):
            assert got['counts'][p][2] == -1 and np.isnan(got['pose'][p]).all() and np.isnan(got['model'][p]).all()
        if n in ('few', 'zero_pivot', 'rejected'):
            assert got['counts'][p][2] == 0 and mso.equal_bits(got['model'][p], cases[n][3]), n
        if n == 'tie':
            assert got['counts'][p][2] == 4


def test_run_to_run_and_capture(gpu, pinned):
    import imagematching_oetr_amd as pkg
    lengths, bounds = pinned['lengths'], pinned['bounds']
    models = pinned['dmodels']['estimate']
    want = pinned['wants']['estimate', 4]
    runs = [host(pkg.refine_poses(pinned['params'], pinned['k1'], pinned['k2'], models, lengths=lengths))
            for _ in range(3)]
    assert_pairs(runs[0], want, bounds, 'run 0')
    assert_same(runs[1], runs[0]), assert_same(runs[2], runs[0])
    # captured with default settings: device inputs only; a replay refits what the buffers hold at replay time
    offsets = torch.from_numpy(bounds.astype(np.int32)).to(gpu)
    k1d, k2d = pinned['k1'].clone(), pinned['k2'].clone()
    out = pkg.refine_poses(pinned['params'], k1d, k2d, models, offsets=offsets)
    torch.cuda.synchronize(gpu)
    for k in KEYS:
        out[k].fill_(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.device(gpu):
        with torch.cuda.graph(graph):
            pkg.refine_poses(pinned['params'], k1d, k2d, models, offsets=offsets, out=out)
            with pytest.raises(ValueError, match='inside a graph capture'):
                pkg.refine_poses(pinned['params'], k1d, k2d, models, lengths=lengths, out=out)
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert_same(host(out), runs[0])
        k1d.copy_(pinned['k1'].flip(0))                                   # other rows: other results on replay
        graph.replay()
        torch.cuda.synchronize(gpu)
    moved = host(out)
    assert not mso.equal_bits(moved['inliers'], runs[0]['inliers']) and not mso.equal_bits(moved['pose'], runs[0]['pose'])
    flipped = pinned['host_k'][0][::-1]
    for p in (4, 11):                      # two lists of the replay, specified (no margins were drawn for them)
        w = pfo.refit(pinned['blocks'][p], flipped[bounds[p]:bounds[p + 1]], pinned['lists'][p][1],
                      pinned['models']['estimate'][p], 1.0, 4)
        assert moved['counts'][p].tolist() == w['counts'].tolist() and mso.equal_bits(moved['model'][p], w['model'])


def test_more_pairs_than_one_grid_dimension_of_65535(gpu, pinned):
    """65 538 pairs of 9-row lists in one call: four distinct lists in turn, every pair its list's specified result."""
    import imagematching_oetr_amd as pkg
    n_pairs, p9 = 65538, 3
    assert pinned['lengths'][p9] == 9
    zp = pfo.edge_cases()['zero_pivot']
    P, (a, b) = pinned['blocks'][p9], pinned['lists'][p9]
    bases = [(P, a, b, pinned['models']['estimate'][p9]), (P, a, b, pinned['models']['true'][p9]),
             (zp[0], zp[1], zp[2], zp[3]), (P, a, b, np.full(9, np.nan))]
    wants = [pfo.refit(*base, 1.0, 4) for base in bases]
    assert [int(w['counts'][2]) for w in wants][2:] == [0, -1] and wants[0]['counts'][2] > 0
    reps = -(-n_pairs // len(bases))
    tile = lambda rows: np.tile(np.stack(rows), (reps,) + (1,) * (np.stack(rows).ndim - 1))
    blocks = tile([base[0] for base in bases])[:n_pairs]
    k1 = tile([base[1] for base in bases]).reshape(-1, 2)[:9 * n_pairs]
    k2 = tile([base[2] for base in bases]).reshape(-1, 2)[:9 * n_pairs]
    models = tile([base[3] for base in bases])[:n_pairs]
    out = pkg.refine_poses(blocks, k1, k2, models, lengths=[9] * n_pairs)
    got = host(out)
    for k in ('model', 'pose', 'cosines', 'counts', 'inliers'):
        want = tile([w[k] for w in wants])
        want = want.reshape(-1)[:9 * n_pairs] if k == 'inliers' else want[:n_pairs]
        assert mso.equal_bits(got[k], want), k
