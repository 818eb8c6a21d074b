"""GPU tests of the match-scoring extension (``oetr_match_score``, ``csrc/match_score.hip``; ``match_score.py``;
``evaluate.match_precision``).  There is no tolerance anywhere: flags and counters are compared for equality and
every value array BIT FOR BIT (``mso.equal_bits``: NaN equals NaN whatever its payload) with the float64 restatement
``tests/match_score_oracle.py::score``, whose pinned lists keep every thresholded value >= 1e-6 relative from its
threshold and every coordinate off a ``.5`` tie (asserted in ``tests/test_match_score_cpu.py``).  The whole fixture
is 2610 matches over maps of at most 56 x 56."""
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

pytestmark = pytest.mark.gpu
EXPECTED = json.loads((REPO / 'tests' / 'match_score_expected.json').read_text())
THR = EXPECTED['thresholds']
PAIRS, LENGTHS = list(mso.PAIRS), list(mso.LENGTHS)
BOUNDS = np.concatenate([[0], np.cumsum(LENGTHS)])


def depth_set(gpu, views):
    import imagematching_oetr_amd as pkg
    ds = pkg.DepthSet(gpu)
    for k, v in enumerate(views):
        assert ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose']) == k
    return ds


def joined(lists, gpu):
    """The lists concatenated -> device float32 ``(k1 [M,2], k2 [M,2])``."""
    k1 = np.concatenate([a for a, _ in lists]).astype(np.float32).reshape(-1, 2)
    k2 = np.concatenate([b for _, b in lists]).astype(np.float32).reshape(-1, 2)
    return torch.from_numpy(k1).to(gpu), torch.from_numpy(k2).to(gpu)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items() if k in mso.VALUES + ('flags', 'counts')}


def assert_lists(got, wants, bounds=None, tag=None):
    """Every list of a call against one restated result each: flags, the four value arrays by bits, counters."""
    bounds = np.concatenate([[0], np.cumsum([len(w['flags']) for w in wants])]) if bounds is None else bounds
    for p, want in enumerate(wants):
        lo, hi = int(bounds[p]), int(bounds[p + 1])
        assert np.array_equal(got['flags'][lo:hi], want['flags']), (tag, p)
        for k in mso.VALUES:
            if k in got:
                assert mso.equal_bits(got[k][lo:hi], want[k]), (tag, p, k)
        assert got['counts'][p].tolist() == want['counts'].tolist(), (tag, p, got['counts'][p], want['counts'])


def assert_same(a, b, keys=mso.VALUES + ('flags', 'counts')):
    for k in keys:
        assert mso.equal_bits(a[k], b[k]), k


@pytest.fixture(scope='module')
def pinned(gpu):
    """The fixture's scene and lists, their restated results, the set on the device and the ONE call that scores all
    14 lists with the restatement's parameter blocks: computed once, shared, never modified."""
    import imagematching_oetr_amd as pkg
    views = mso.make_scene(tuple(tuple(s) for s in EXPECTED['sizes']), EXPECTED['seed'])
    lists = mso.make_lists(views, seed=EXPECTED['seed'])
    # the inputs first, so that a wrong input cannot pass as a wrong kernel
    assert [cvo.sha(v['depth']) for v in views] == EXPECTED['depth_sha256']
    assert [cvo.sha(np.concatenate([k1, k2])) for k1, k2 in lists] == EXPECTED['kpts_sha256']
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in PAIRS])
    assert [cvo.sha(b) for b in blocks] == EXPECTED['params_sha256']
    assert [len(k1) for k1, _ in lists] == LENGTHS and sum(LENGTHS) == 2610
    wants = mso.score_lists(views, PAIRS, lists, **THR)
    ds = depth_set(gpu, views)
    k1, k2 = joined(lists, gpu)
    out = pkg.score_matches(ds, PAIRS, k1, k2, lengths=LENGTHS, params=blocks, **THR)
    torch.cuda.synchronize()
    return dict(views=views, lists=lists, blocks=blocks, wants=wants, ds=ds, k1=k1, k2=k2, out=out, got=host(out))


def test_pinned_lists_equal_the_restatement_and_the_fixture(pinned):
    out, got = pinned['out'], pinned['got']
    assert out['flags'].dtype == torch.uint8 and out['counts'].dtype == torch.int32 and out['counts'].shape == (14, 5)
    assert out['values'].dtype == torch.float64 and out['values'].shape == (4, 2610) and out['flags'].device.type == 'cuda'
    for k, name in enumerate(mso.VALUES):
        assert out[name].data_ptr() == out['values'][k].data_ptr() and out[name].shape == (2610,)
    assert_lists(got, pinned['wants'], BOUNDS, 'pinned')
    assert got['counts'].tolist() == [rec['counts'] for rec in EXPECTED['lists']]
    assert got['counts'][8].tolist() == [0, 0, 0, 0, 0]                          # the empty list


def test_special_rows(gpu, pinned):
    """``.5`` ties both ways, -0.5 / -0.51, ``W - 0.5`` / ``W - 0.49``, +-inf and NaN, on even, odd and 1 x 1 maps."""
    import imagematching_oetr_amd as pkg
    views = pinned['views']
    slot = {tuple(s): k for k, s in enumerate(EXPECTED['sizes'])}
    shapes = (((40, 64), (7, 5)), ((7, 5), (1, 1)), ((56, 56), (56, 56)))
    pairs = [(slot[a], slot[b]) for a, b in shapes]
    lists = [mso.special_matches(a, b) for a, b in shapes]
    assert all(len(k1) == 48 for k1, _ in lists)
    wants = mso.score_lists(views, pairs, lists, **THR)
    assert sum(int(np.isnan(w['epi_ref']).sum()) for w in wants) > 10 and sum(int(w['counts'][3]) for w in wants) > 5
    k1, k2 = joined(lists, gpu)
    blocks = np.stack([mso.pair_block(views, i, j) for i, j in pairs])
    got = host(pkg.score_matches(pinned['ds'], pairs, k1, k2, lengths=[48] * 3, params=blocks, **THR))
    assert_lists(got, wants, tag='special')
    for p, want in enumerate(wants):                                             # the depth look-up itself, row by row
        assert ((got['flags'][48 * p:48 * p + 48] & 1) != 0).tolist() == (want['d1'] != 0).tolist(), p
        assert ((got['flags'][48 * p:48 * p + 48] & 2) != 0).tolist() == (want['d2'] != 0).tolist(), p


def test_thresholds_off_and_each_alone(pinned):
    import imagematching_oetr_amd as pkg
    args = (pinned['ds'], PAIRS, pinned['k1'], pinned['k2'])
    kw = dict(lengths=LENGTHS, params=pinned['blocks'])
    got = host(pkg.score_matches(*args, epi_thr=None, sym_thr=None, px_thr=None, **kw))
    both = [int(w['counts'][3]) for w in pinned['wants']]
    assert got['counts'].tolist() == [[n, -1, -1, b, -1] for n, b in zip(LENGTHS, both)]
    assert (got['flags'] & 28 == 0).all() and np.array_equal(got['flags'], pinned['got']['flags'] & 3)
    assert_same(got, pinned['got'], mso.VALUES)                                  # the values do not depend on thresholds
    for name, bit in (('epi_thr', 4), ('sym_thr', 8), ('px_thr', 16)):
        thr = dict(epi_thr=None, sym_thr=None, px_thr=None)
        thr[name] = THR[name]
        got = host(pkg.score_matches(*args, **thr, **kw))
        assert_lists(got, mso.score_lists(pinned['views'], PAIRS, pinned['lists'], **thr), BOUNDS, name)
        assert np.array_equal(got['flags'], pinned['got']['flags'] & (3 | bit)), name
        assert (got['flags'] & bit).any(), name


def test_depth_set_route_with_the_devices_own_blocks(pinned):
    """``params=None``: the blocks come from the set's cameras (``match_params``); restated with those very blocks,
    everything is equal - self pairs, whose ``t`` is a rounding residue, included."""
    import imagematching_oetr_amd as pkg
    ds = pinned['ds']
    index = torch.tensor(PAIRS, dtype=torch.int32, device=ds.device)
    blocks = pkg.match_params(ds, index[:, 0].contiguous(), index[:, 1].contiguous())
    assert blocks.dtype == torch.float64 and blocks.shape == (14, 20) and blocks.is_cuda
    blocks = blocks.cpu().numpy()
    assert np.allclose(blocks, pinned['blocks'], rtol=1e-9, atol=1e-9)             # the same cameras ...
    assert np.array_equal(blocks[:, :8], pinned['blocks'][:, :8])                   # ... the intrinsics copied
    got = host(pkg.score_matches(ds, index, pinned['k1'], pinned['k2'], lengths=LENGTHS, **THR))
    wants = mso.score_lists(pinned['views'], PAIRS, pinned['lists'], blocks=blocks, **THR)
    assert_lists(got, wants, BOUNDS, 'depth set')
    assert sum(i == j for i, j in PAIRS) == 4


def test_pairs_that_are_not_vouched_for(pinned):
    """Indices -1 and ``len(ds)`` among good pairs: flags 0, NaN values, all five counters -1; every other pair is
    what it is in a call without them."""
    import imagematching_oetr_amd as pkg
    ds, n = pinned['ds'], len(pinned['ds'])
    bad = {2: (-1, 2), 5: (2, n), 9: (n, -1)}                                      # lists of 256, 64 and 600 rows
    pairs = [bad.get(p, pair) for p, pair in enumerate(PAIRS)]
    got = host(pkg.score_matches(ds, pairs, pinned['k1'], pinned['k2'], lengths=LENGTHS, params=pinned['blocks'], **THR))
    for p in range(len(PAIRS)):
        lo, hi = int(BOUNDS[p]), int(BOUNDS[p + 1])
        if p in bad:
            assert got['counts'][p].tolist() == [-1] * 5, p
            assert not got['flags'][lo:hi].any(), p
            assert all(np.isnan(got[k][lo:hi]).all() for k in mso.VALUES), p
        else:
            assert got['counts'][p].tolist() == pinned['got']['counts'][p].tolist(), p
            assert np.array_equal(got['flags'][lo:hi], pinned['got']['flags'][lo:hi]), p
            for k in mso.VALUES:
                assert mso.equal_bits(got[k][lo:hi], pinned['got'][k][lo:hi]), (p, k)
    summary = pkg.match_precision({'counts': torch.from_numpy(got['counts'])})
    assert (summary['n_pairs'], summary['n_not_scored']) == (11, 3)


def test_rows_outside_every_list_are_left_unscored(gpu, pinned):
    """``offsets[0] > 0`` and ``offsets[P] < M``: rows before the first and after the last list get flags 0 and NaN
    values; the rows inside and the counters are those of the plain call."""
    import imagematching_oetr_amd as pkg
    head, tail = 5, 70
    pad = lambda k, n: pinned['k1' if k == 1 else 'k2'][:n].clone()
    k1 = torch.cat([pad(1, head), pinned['k1'], pad(1, tail)])
    k2 = torch.cat([pad(2, head), pinned['k2'], pad(2, tail)])
    offsets = torch.from_numpy((BOUNDS + head).astype(np.int32)).to(gpu)
    got = host(pkg.score_matches(pinned['ds'], PAIRS, k1, k2, offsets=offsets, params=pinned['blocks'], **THR))
    M = 2610
    assert got['flags'].shape == (head + M + tail,)
    outside = np.r_[0:head, head + M:head + M + tail]
    assert not got['flags'][outside].any() and all(np.isnan(got[k][outside]).all() for k in mso.VALUES)
    inside = {k: (got[k][head:head + M] if k != 'counts' else got[k]) for k in got}
    assert_same(inside, pinned['got'])


def test_runs_are_identical_and_do_not_depend_on_the_order_of_the_list(gpu, pinned):
    import imagematching_oetr_amd as pkg
    ds, kw = pinned['ds'], dict(lengths=LENGTHS, params=pinned['blocks'])
    again = host(pkg.score_matches(ds, PAIRS, pinned['k1'], pinned['k2'], **kw, **THR))
    assert_same(again, pinned['got'])
    for k in mso.VALUES:                                                           # one device: the NaN payloads too
        assert np.array_equal(again[k].view(np.uint64), pinned['got'][k].view(np.uint64)), k
    order = np.random.default_rng(4).permutation(len(PAIRS))
    lists = [pinned['lists'][k] for k in order]
    k1, k2 = joined(lists, gpu)
    got = host(pkg.score_matches(ds, [PAIRS[k] for k in order], k1, k2, lengths=[LENGTHS[k] for k in order],
                                 params=pinned['blocks'][order], **THR))
    assert_lists(got, [pinned['wants'][k] for k in order], tag='permuted')
    at = 0
    for k in order:                                                                # and bit-identical to the plain call
        lo, hi = int(BOUNDS[k]), int(BOUNDS[k + 1])
        for name in mso.VALUES:
            assert np.array_equal(got[name][at:at + hi - lo].view(np.uint64), pinned['got'][name][lo:hi].view(np.uint64))
        at += hi - lo
    # without the value arrays: the same flags and counters
    bare = pkg.score_matches(ds, PAIRS, pinned['k1'], pinned['k2'], values=False, **kw, **THR)
    assert sorted(k for k in bare if not k.startswith('_')) == ['counts', 'flags']
    assert_same(host(bare), pinned['got'], ('flags', 'counts'))
    # float16 keypoints are widened: the score of the float32 keypoints of the same values
    h1, h2 = pinned['k1'][:700].half(), pinned['k2'][:700].half()
    lengths = [600, 100]
    a = host(pkg.score_matches(ds, PAIRS[:2], h1, h2, lengths=lengths, params=pinned['blocks'][:2], **THR))
    b = host(pkg.score_matches(ds, PAIRS[:2], h1.float(), h2.float(), lengths=lengths, params=pinned['blocks'][:2], **THR))
    assert_same(a, b)
    wants = mso.score_lists(pinned['views'], PAIRS[:2], [(h1[:600].cpu().numpy(), h2[:600].cpu().numpy()),
                                                         (h1[600:].cpu().numpy(), h2[600:].cpu().numpy())], **THR)
    for p, (lo, hi) in enumerate(((0, 600), (600, 700))):                          # values only: no margin is promised here
        for k in mso.VALUES:
            assert mso.equal_bits(a[k][lo:hi], wants[p][k]), (p, k)


def test_empty_calls(gpu, pinned):
    import imagematching_oetr_amd as pkg
    ds = pinned['ds']
    none = torch.zeros(0, 2, device=gpu)
    out = pkg.score_matches(ds, PAIRS[:3] + [(-1, 0)], none, none, lengths=[0] * 4, **THR)
    assert out['counts'].tolist() == [[0] * 5] * 3 + [[-1] * 5] and out['flags'].shape == (0,) and out['values'].shape == (4, 0)
    out = pkg.score_matches(ds, PAIRS[:2], none, none, lengths=[0, 0], epi_thr=None)
    assert out['counts'].tolist() == [[0, -1, -1, 0, -1]] * 2
    out = pkg.score_matches(ds, [], pinned['k1'][:9], pinned['k2'][:9], offsets=torch.zeros(1, dtype=torch.int32, device=gpu))
    assert out['counts'].shape == (0, 5) and not out['flags'].any() and torch.isnan(out['values']).all()
    with pytest.raises(ValueError, match='summing'):
        pkg.score_matches(ds, PAIRS[:2], pinned['k1'][:9], pinned['k2'][:9], lengths=[4, 4])


def test_out_is_reused_and_the_call_is_captured_and_replayed_on_new_data(gpu, pinned):
    """Enqueue-only, no host read: captured with default settings; a replay scores what the keypoint and offset
    tensors hold at replay time."""
    import imagematching_oetr_amd as pkg
    ds, views = pinned['ds'], pinned['views']
    index = torch.tensor(PAIRS, dtype=torch.int32, device=gpu)
    k1, k2 = pinned['k1'].clone(), pinned['k2'].clone()
    offsets = torch.from_numpy(BOUNDS.astype(np.int32)).to(gpu)
    out = pkg.score_matches(ds, index, k1, k2, offsets=offsets, **THR)            # also uploads the table
    first = host(out)
    ptrs = {k: out[k].data_ptr() for k in ('values', 'flags', 'counts') + mso.VALUES}
    for k in ('values', 'flags', 'counts'):
        out[k].fill_(1)
    assert pkg.score_matches(ds, index, k1, k2, offsets=offsets, out=out, **THR) is out
    assert {k: out[k].data_ptr() for k in ptrs} == ptrs
    assert_same(host(out), first)
    with pytest.raises(ValueError, match='other sizes'):
        pkg.score_matches(ds, index[:3], k1, k2, offsets=offsets[:4], out=out, **THR)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.score_matches(ds, index, k1, k2, offsets=offsets, **THR)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(host(captured), first)
    # new keypoints and other list boundaries of the same total
    lengths = [500, 357] + LENGTHS[2:]
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    n1, n2 = joined(mso.make_lists(views, lengths=lengths, seed=1), gpu)
    assert n1.shape == k1.shape and not torch.equal(n1, k1)
    k1.copy_(n1)
    k2.copy_(n2)
    offsets.copy_(torch.from_numpy(bounds.astype(np.int32)))
    graph.replay()
    torch.cuda.synchronize()
    fresh = host(pkg.score_matches(ds, PAIRS, n1, n2, lengths=lengths, **THR))
    replayed = host(captured)
    assert_same(replayed, fresh)
    assert replayed['counts'][:, 0].tolist() == lengths and not np.array_equal(replayed['flags'], first['flags'])


def test_match_precision_of_the_pinned_call(pinned):
    import imagematching_oetr_amd as pkg
    res = pkg.match_precision(pinned['out'])
    counts = np.array([rec['counts'] for rec in EXPECTED['lists']], np.float64)
    want = np.array([c[1] / c[0] if c[0] else 0.0 for c in counts])
    assert np.array_equal(res['precision'], want) and res['mean_precision'] == float(want.mean())
    want_px = np.array([c[4] / c[3] if c[3] else 0.0 for c in counts])
    assert np.array_equal(res['reproj_precision'], want_px)
    assert (res['n_pairs'], res['n_not_scored'], res['n_matches']) == (14, 0, 2610)
