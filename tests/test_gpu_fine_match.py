"""GPU tests of the fine-level refinement (``oetr_fine_windows`` / ``oetr_fine_refine``, ``csrc/fine_match.hip``;
``fine_match.py``, ``dloc_matcher.CoarseToFine``).  There is no tolerance anywhere: every output of every call is
compared for equality - the floats by their bits - with the numpy specification ``tests/fine_match_oracle.py`` on ALL
rows, on the pinned calls of ``tests/fine_match_cases.py`` (checked against the fixture in
``tests/test_fine_match_cpu.py``) at three capacities each: room for every match, a cut in the middle of a pair, none."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dual_softmax_cases as dsc  # noqa: E402
import dual_softmax_oracle as dso  # noqa: E402
import fine_match_cases as fmc  # noqa: E402
import fine_match_oracle as fmo  # noqa: E402
import match_assembly_oracle as mao  # noqa: E402

pytestmark = pytest.mark.gpu
WINDOW_OUTPUTS = ('rows', 'moffsets', 'counts', 'win0', 'win1')
FINE_OUTPUTS = ('expec', 'mkpts0', 'mkpts1', 'keypoints1', 'counts')
F32 = np.float32


def t(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def upload(call, gpu):
    """``(coarse, fine keywords)``: the call on the device in the form ``match_dense`` leaves and ``fine_windows`` takes."""
    coarse = dict(matches0=t(call['matches0'], gpu), keypoints0=t(call['kp0'], gpu), keypoints1=t(call['kp1'], gpu),
                  _inputs=(None, None, t(call['off0'], gpu), t(call['off1'], gpu), t(call['grids0'], gpu),
                           t(call['grids1'], gpu)))
    kw = dict(fine0=t(call['fine0'], gpu), fine1=t(call['fine1'], gpu), fine_offsets0=t(call['foff0'], gpu),
              fine_offsets1=t(call['foff1'], gpu), fine_grids0=t(call['fgrids0'], gpu), fine_grids1=t(call['fgrids1'], gpu),
              window=call['W'], stride=call['stride'], max_k0=call['max_k0'])
    return coarse, kw


def host(res, keys):
    return {k: res[k].cpu().numpy() for k in keys}


def assert_equal(got, want, tag, keys):
    for k in keys:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            rows = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(1))[0]
            raise AssertionError((tag, k, len(rows), rows[:8].tolist(), g[rows[:8]].reshape(len(rows[:8]), -1)[:, :6].tolist(),
                                  w[rows[:8]].reshape(len(rows[:8]), -1)[:, :6].tolist()))


def capacities(call):
    total = fmc.matched_total(call)
    return [total + 2, max(total // 2, 1), 0]


@pytest.fixture(scope='module')
def device_calls(gpu):
    """Every pinned call on the device: made once, shared, never modified."""
    return {name: upload(fmc.make_call(name), gpu) for name in fmc.SHAPES}


@pytest.mark.parametrize('name', list(fmc.SHAPES))
def test_every_capacity_equals_the_specification_bit_for_bit(gpu, device_calls, name):
    import imagematching_oetr_amd as pkg
    call = fmc.make_call(name)
    coarse, kw = device_calls[name]
    for cap in capacities(call):
        win = pkg.fine_windows(coarse, max_matches=cap, **kw)
        fine = pkg.refine_matches(win, coarse, fine_cell=fmc.CELL / call['stride'])
        want_win, want_fine = fmc.expected(call, cap, fine_cell=fmc.CELL / call['stride'])
        assert_equal(host(win, WINDOW_OUTPUTS), want_win, (name, cap), WINDOW_OUTPUTS)
        assert_equal(host(fine, FINE_OUTPUTS), want_fine, (name, cap), FINE_OUTPUTS)
        assert np.array_equal(pkg.fine_match_counts(fine), want_fine['counts'])
        assert np.array_equal(pkg.fine_match_counts(win), want_win['counts'])
        assert fine['keypoints0'] is coarse['keypoints0'] or torch.equal(fine['keypoints0'], coarse['keypoints0'])


def test_non_finite_window_entries_and_windows_without_a_candidate(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    call = fmc.make_call('c8w5s2')
    coarse, kw = device_calls['c8w5s2']
    cap = fmc.matched_total(call)
    win = pkg.fine_windows(coarse, max_matches=cap, **kw)
    want_win = fmc.windows(call, cap)
    w0, w1 = want_win['win0'].copy(), want_win['win1'].copy()
    w1[0, 3, 2] = np.nan                                             # one position drops out
    w1[1, :, 0] = np.nan                                             # no candidate
    w1[2, 7, 1], w1[3, 9, 5] = np.inf, -np.inf
    w0[4, 12, 3] = np.inf                                            # the centre: every product non-finite or NaN
    w0[5, 0, 0] = np.nan                                             # not the centre: changes nothing
    w0[6], w1[6] = fmc.one_hot_windows(5, 8, 6, np.random.default_rng(1))
    w1[7] = 0                                                        # a uniform window
    fine = pkg.refine_matches(win, coarse, win0=t(w0, gpu), win1=t(w1, gpu), fine_cell=4.0)
    want = fmc.refine(call, want_win, w0, w1, fine_cell=4.0)
    assert_equal(host(fine, FINE_OUTPUTS), want, 'non-finite', FINE_OUTPUTS)
    assert int(want['counts'][:, 2].sum()) == 2 and np.isnan(want['expec'][[1, 4], 2]).all()
    assert (want['expec'][[1, 4], :2] == 0).all() and want['expec'][6, 0] == fmo.grid(5)[1] == want['expec'][6, 1]


def test_pairs_that_are_not_vouched_for_are_not_read_and_guards_stay(gpu, device_calls):
    """The ``mixed`` call: pairs without a match, with every token matched, with a coarse or a fine grid that does not
    multiply to its rows, beyond ``max_k0``, with an empty fine map, and out-of-range ``matches0`` values.  Every
    output and the workspace sit between guard rows that no launch may touch."""
    import imagematching_oetr_amd as pkg
    call = fmc.make_call('mixed')
    coarse, kw = device_calls['mixed']
    P, N1, W, C, guard = len(call['pairs']), len(call['kp1']), call['W'], call['C'], 16
    need = int(pkg.load_library().oetr_fine_match_workspace_bytes(P))
    for cap in capacities(call):
        shapes = dict(rows=((cap, 3), torch.int32), moffsets=((P + 1,), torch.int32), counts=((P, 2), torch.int32),
                      win0=((cap, W * W, C), torch.float32), win1=((cap, W * W, C), torch.float32),
                      workspace=((need,), torch.uint8))
        fine_shapes = dict(expec=((cap, 3), torch.float32), mkpts0=((cap, 2), torch.float32),
                           mkpts1=((cap, 2), torch.float32), keypoints1=((N1, 2), torch.float32),
                           counts=((P, 3), torch.int32))
        whole, outs = [{}, {}], [{}, {}]
        for k, table in enumerate((shapes, fine_shapes)):
            for key, (shape, dtype) in table.items():
                whole[k][key] = torch.full((shape[0] + 2 * guard,) + shape[1:], 77, dtype=dtype, device=gpu)
                outs[k][key] = whole[k][key][guard:guard + shape[0]]
        win = pkg.fine_windows(coarse, max_matches=cap, out=outs[0], **kw)
        fine = pkg.refine_matches(win, coarse, out=outs[1])
        assert win is outs[0] and fine is outs[1]
        want_win, want_fine = fmc.expected(call, cap)
        assert_equal(host(win, WINDOW_OUTPUTS), want_win, ('mixed', cap), WINDOW_OUTPUTS)
        assert_equal(host(fine, FINE_OUTPUTS), want_fine, ('mixed', cap), FINE_OUTPUTS)
        for k, table in enumerate((shapes, fine_shapes)):
            for key, (shape, _) in table.items():
                assert (whole[k][key][:guard] == 77).all() and (whole[k][key][guard + shape[0]:] == 77).all(), (cap, key)
    assert want_fine['counts'][3:6].tolist() == [[-1, -1, -1]] * 3 and want_fine['counts'][1].tolist() == [0, 0, 0]


def many_small_pairs(P=65538):
    """``P`` pairs of 1 x 1 coarse grids over 1 x 1 fine grids: about half of them matched."""
    rng = np.random.default_rng(3)
    steps = np.arange(P + 1, dtype=np.int32)
    ones = np.ones((P, 2), np.int32)
    m = np.where(rng.random(P) < 0.5, 0, rng.choice([-1, 1, 7, -3], P)).astype(np.int32)
    kp = (rng.integers(0, 80, (P, 2)) * 8).astype(F32)
    return dict(name='many', C=4, W=3, stride=1, matches0=m, off0=steps, off1=steps, grids0=ones, grids1=ones,
                foff0=steps, foff1=steps, fgrids0=ones, fgrids1=ones, kp0=kp, kp1=kp[::-1].copy(),
                fine0=rng.standard_normal((P, 4)).astype(F32), fine1=rng.standard_normal((P, 4)).astype(F32), max_k0=1)


def test_more_pairs_than_one_grid_dimension(gpu):
    import imagematching_oetr_amd as pkg
    call = many_small_pairs()
    assert len(call['off0']) - 1 == 65538
    coarse, kw = upload(call, gpu)
    cap = 40000
    win = pkg.fine_windows(coarse, max_matches=cap, **kw)
    fine = pkg.refine_matches(win, coarse, fine_cell=2.0)
    want_win, want_fine = fmc.expected(call, cap)
    assert_equal(host(win, WINDOW_OUTPUTS), want_win, '65538 pairs', WINDOW_OUTPUTS)
    assert_equal(host(fine, FINE_OUTPUTS), want_fine, '65538 pairs', FINE_OUTPUTS)
    assert 30000 < want_win['moffsets'][-1] < cap and (want_win['counts'][:, 0] >= 0).all()


def test_a_list_longer_than_one_grid_of_workgroups(gpu):
    """One pair of 131 x 129 tokens, every token matched: 16 899 list rows against the 16 384 workgroups of the two
    grid-stride loops, and 17 chunks of 1024 rows in the walk that places them."""
    import imagematching_oetr_amd as pkg
    g = (131, 129)
    K = g[0] * g[1]
    rng = np.random.default_rng(9)
    i32 = lambda v: np.asarray(v, np.int32)                            # noqa: E731
    call = dict(name='long', C=4, W=3, stride=1, matches0=rng.permutation(K).astype(np.int32), off0=i32([0, K]),
                off1=i32([0, K]), grids0=i32([g]), grids1=i32([g]), foff0=i32([0, K]), foff1=i32([0, K - g[1]]),
                fgrids0=i32([g]), fgrids1=i32([(g[0] - 1, g[1])]), kp0=dso.keypoints(*g, 8), kp1=dso.keypoints(*g, 8),
                fine0=rng.standard_normal((K, 4)).astype(F32), fine1=rng.standard_normal((K - g[1], 4)).astype(F32),
                max_k0=K)
    assert K > 16384
    coarse, kw = upload(call, gpu)
    for cap in (K + 5, K - 300):
        win = pkg.fine_windows(coarse, max_matches=cap, **kw)
        fine = pkg.refine_matches(win, coarse, fine_cell=8.0)
        want_win, want_fine = fmc.expected(call, cap, fine_cell=8.0)
        assert_equal(host(win, WINDOW_OUTPUTS), want_win, ('long', cap), WINDOW_OUTPUTS)
        assert_equal(host(fine, FINE_OUTPUTS), want_fine, ('long', cap), FINE_OUTPUTS)
    assert want_fine['counts'].tolist() == [[K, K - 300, 0]]


def test_two_calls_give_equal_bits_out_is_reused_and_a_graph_replays(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    call = fmc.make_call('c128w5s4')
    coarse, kw = device_calls['c128w5s4']
    coarse = dict(coarse, matches0=coarse['matches0'].clone())
    cap = fmc.matched_total(call) - 3
    want_win, want_fine = fmc.expected(call, cap)

    def both(**out):
        win = pkg.fine_windows(coarse, max_matches=cap, out=out.get('win'), **kw)
        return win, pkg.refine_matches(win, coarse, out=out.get('fine'))

    def as_host(win, fine):
        return host(win, WINDOW_OUTPUTS), host(fine, FINE_OUTPUTS)

    first, again = as_host(*both()), as_host(*both())
    for k, keys in enumerate((WINDOW_OUTPUTS, FINE_OUTPUTS)):
        assert_equal(again[k], first[k], 'two eager calls', keys)
        assert_equal(first[k], (want_win, want_fine)[k], 'specification', keys)
    win, fine = both()
    ptrs = {k: win[k].data_ptr() for k in WINDOW_OUTPUTS + ('workspace',)} | {k: fine[k].data_ptr() for k in FINE_OUTPUTS}
    win['win0'].fill_(5), fine['expec'].fill_(5), win['rows'].fill_(5)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    win2, fine2 = both(win=win, fine=fine)
    assert win2 is win and fine2 is fine and torch.cuda.memory_allocated() == before
    assert {k: win[k].data_ptr() for k in WINDOW_OUTPUTS + ('workspace',)} | {k: fine[k].data_ptr() for k in FINE_OUTPUTS} == ptrs
    got = as_host(win, fine)
    assert_equal(got[0], want_win, 'reused', WINDOW_OUTPUTS)
    assert_equal(got[1], want_fine, 'reused', FINE_OUTPUTS)
    with pytest.raises(ValueError, match='other sizes'):
        pkg.fine_windows(coarse, max_matches=cap + 1, out=win, **kw)
    # captured, replayed, replayed on other matches, and on the first ones again
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cwin, cfine = both()
        with pytest.raises(ValueError, match='inside a graph capture'):              # host offsets: refused, nothing enqueued
            pkg.fine_windows(coarse, max_matches=cap, **dict(kw, fine_offsets0=call['foff0']))
    graph.replay()
    torch.cuda.synchronize()
    got = as_host(cwin, cfine)
    assert_equal(got[0], want_win, 'replay', WINDOW_OUTPUTS)
    assert_equal(got[1], want_fine, 'replay', FINE_OUTPUTS)
    kept = coarse['matches0'].clone()
    other = dict(call, matches0=np.where(np.arange(len(call['matches0'])) % 3 == 0, -1, call['matches0']).astype(np.int32))
    coarse['matches0'].copy_(t(other['matches0'], gpu))
    graph.replay()
    torch.cuda.synchronize()
    moved = as_host(cwin, cfine)
    want2 = fmc.expected(other, cap)
    assert_equal(moved[0], want2[0], 'replay on other matches', WINDOW_OUTPUTS)
    assert_equal(moved[1], want2[1], 'replay on other matches', FINE_OUTPUTS)
    assert want2[0]['moffsets'][-1] < want_win['moffsets'][-1]
    coarse['matches0'].copy_(kept)
    graph.replay()
    torch.cuda.synchronize()
    got = as_host(cwin, cfine)
    assert_equal(got[0], want_win, 'replay on the first matches', WINDOW_OUTPUTS)
    assert_equal(got[1], want_fine, 'replay on the first matches', FINE_OUTPUTS)


def test_device_sqrtf_division_and_e_on_a_sweep(gpu):
    """The assumptions the parity rests on - the device's float32 ``sqrtf`` and ``/`` are the correctly rounded ones
    and its ``e`` is the specification's - on 2^16 hand-made windows whose softmax runs from flat to one-hot, so that
    the two variances under the square roots sweep ``1e-10 .. 1``: ``std`` equals the ``np.sqrt`` specification bit
    for bit on every row."""
    import imagematching_oetr_amd as pkg
    rng = np.random.default_rng(17)
    M, W, C = 1 << 16, 3, 4
    win0 = rng.standard_normal((M, W * W, C)).astype(F32)
    win1 = (rng.standard_normal((M, W * W, C)) * np.exp(rng.uniform(-3, 3, (M, 1, 1)))).astype(F32)
    i32 = lambda v: np.asarray(v, np.int32)                            # noqa: E731
    rows = np.stack([np.zeros(M), np.arange(M), np.arange(M)], -1).astype(np.int32)
    kp = (rng.random((M, 2)) * 640).astype(F32)
    off = t(i32([0, M]), gpu)
    windows = dict(rows=t(rows, gpu), moffsets=off, counts=t(i32([[M, M]]), gpu), window=W, win0=t(win0, gpu),
                   win1=t(win1, gpu), _inputs=(None, off, off))
    coarse = dict(matches0=None, keypoints0=t(kp, gpu), keypoints1=t(kp, gpu))
    fine = pkg.refine_matches(windows, coarse, fine_cell=2.6667)
    want = fmo.refine_call(win0, win1, rows, i32([0, M]), i32([[M, M]]), kp, i32([0, M]), kp, i32([0, M]), W=W,
                           fine_cell=2.6667)
    sd = want['expec'][:, 2]
    print('std over %d rows: %.3g .. %.3g, %d at the floor' % (M, sd.min(), sd.max(), int((sd < 3e-5).sum())))
    assert sd.min() < 1e-4 and sd.max() > 1.5 and len(np.unique(sd)) > M // 2
    assert_equal(host(fine, FINE_OUTPUTS), want, 'sweep', FINE_OUTPUTS)


def test_per_pair_form_and_channels_first(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    call = fmc.make_call('c64w5s4')
    coarse, _ = device_calls['c64w5s4']
    C, cap = call['C'], fmc.matched_total(call)
    maps0 = [call['fine0'][a:b].reshape(*g, C) for a, b, g in zip(call['foff0'][:-1], call['foff0'][1:], call['fgrids0'])]
    maps1 = [call['fine1'][a:b].reshape(*g, C) for a, b, g in zip(call['foff1'][:-1], call['foff1'][1:], call['fgrids1'])]
    want_win = fmc.windows(call, cap)
    kw = dict(window=call['W'], stride=call['stride'], max_matches=cap)
    win = pkg.fine_windows(coarse, [t(a, gpu) for a in maps0], [t(b, gpu) for b in maps1], **kw)
    assert_equal(host(win, WINDOW_OUTPUTS), want_win, 'device maps per pair', WINDOW_OUTPUTS)
    win = pkg.fine_windows(coarse, [np.array(a.transpose(2, 0, 1)) for a in maps0],
                           [torch.from_numpy(np.array(b.transpose(2, 0, 1))) for b in maps1], channels_first=True, **kw)
    assert_equal(host(win, WINDOW_OUTPUTS), want_win, 'host [C,hf,wf] per pair', WINDOW_OUTPUTS)
    with pytest.raises(ValueError, match='C % 4'):
        pkg.fine_windows(coarse, [torch.zeros(8, 8, 6, device=gpu)] * 2, [torch.zeros(8, 8, 6, device=gpu)] * 2, **kw)


def test_the_chain_from_match_dense_to_assemble_matches_equals_the_oracles(gpu):
    """``match_dense -> fine_windows -> refine_matches -> assemble_matches`` on a crop call equals the specifications
    chained on the host; ``CoarseToFine`` on a batch returns the same refined matches."""
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd.dloc_matcher import CoarseToFine
    call = dsc.make_call('ragged64', 'gauss')
    dev = dict(feat0=t(call['feat0'], gpu), feat1=t(call['feat1'], gpu), offsets0=t(call['off0'], gpu),
               offsets1=t(call['off1'], gpu), grids0=t(call['grids0'], gpu), grids1=t(call['grids1'], gpu),
               max_k0=call['max_k0'], max_k1=call['max_k1'])
    P, W, stride, C = len(call['pairs']), 5, 2, 8
    rng = np.random.default_rng(4)
    fg0, fg1 = np.asarray(call['grids0']) * stride, np.asarray(call['grids1']) * stride - 1
    fg1 = np.maximum(fg1, 0)
    foff0 = np.concatenate([[0], np.cumsum(fg0[:, 0] * fg0[:, 1])]).astype(np.int32)
    foff1 = np.concatenate([[0], np.cumsum(fg1[:, 0] * fg1[:, 1])]).astype(np.int32)
    fine0 = rng.standard_normal((foff0[-1], C)).astype(F32)
    fine1 = rng.standard_normal((foff1[-1], C)).astype(F32)
    coarse = pkg.match_dense(**dev, temperature=0.1, threshold=0.0, border_rm=0, cell=dsc.CELL)
    spec = dsc.expected(call, 0.1, 0.0, 0)
    cap = int((spec['matches0'] > -1).sum()) + 1
    win = pkg.fine_windows(coarse, t(fine0, gpu), t(fine1, gpu), fine_offsets0=t(foff0, gpu), fine_offsets1=t(foff1, gpu),
                           fine_grids0=t(fg0.astype(np.int32), gpu), fine_grids1=t(fg1.astype(np.int32), gpu), window=W,
                           stride=stride, max_matches=cap, max_k0=call['max_k0'])
    fine = pkg.refine_matches(win, coarse, fine_cell=dsc.CELL / stride)
    want_win = fmo.windows_call(spec['matches0'], call['off0'], call['off1'], call['grids0'], call['grids1'],
                                len(call['feat1']), fine0, foff0, fg0, fine1, foff1, fg1, W=W, stride=stride,
                                max_matches=cap, max_k0=call['max_k0'])
    want_fine = fmo.refine_call(want_win['win0'], want_win['win1'], want_win['rows'], want_win['moffsets'],
                                want_win['counts'], spec['keypoints0'], call['off0'], spec['keypoints1'], call['off1'], W=W,
                                fine_cell=dsc.CELL / stride)
    assert_equal(host(win, WINDOW_OUTPUTS), want_win, 'chain', WINDOW_OUTPUTS)
    assert_equal(host(fine, FINE_OUTPUTS), want_fine, 'chain', FINE_OUTPUTS)
    assert want_win['moffsets'][-1] == cap - 1 > 100
    moved = np.abs(want_fine['keypoints1'] - spec['keypoints1']).max(-1)
    assert (moved > 0).sum() >= cap // 2 and moved.max() <= (W // 2) * dsc.CELL / stride
    geometry = mao.make_call(5, tuple((L, S, 'none', 1) for L, S in call['pairs']))       # hand-made records
    records = torch.from_numpy(np.ascontiguousarray(geometry['info']).view(np.uint8).reshape(len(geometry['info']), -1)
                               .copy()).to(gpu)
    lists = pkg.assemble_matches(records, t(geometry['scales'], gpu), coarse['keypoints0'], fine['keypoints1'],
                                 coarse['matches0'], coarse['matching_scores0'], offsets0=dev['offsets0'],
                                 offsets1=dev['offsets1'])
    want = mao.assemble(**dict(geometry, kp0=spec['keypoints0'], kp1=want_fine['keypoints1'], matches=spec['matches0'],
                               conf=spec['matching_scores0']))
    for k, w in want.items():
        assert mao.equal_bits(lists[k].cpu().numpy(), w), k
    assert lists['offsets'].cpu().tolist() == want_win['moffsets'].tolist()               # the same lists, pair by pair

    # the plug-in on a batch with a stub net: pairs 1 and 2 of the call have the same shapes on neither side, so the
    # batch is one pair's maps twice
    p = int(np.argmax([L * S for L, S in call['pairs']]))
    g0, g1 = tuple(call['grids0'][p]), tuple(call['grids1'][p])
    c0 = t(call['feat0'][call['off0'][p]:call['off0'][p + 1]].reshape(*g0, -1).transpose(2, 0, 1), gpu)
    c1 = t(call['feat1'][call['off1'][p]:call['off1'][p + 1]].reshape(*g1, -1).transpose(2, 0, 1), gpu)
    f0 = t(fine0[foff0[p]:foff0[p + 1]].reshape(*fg0[p], C).transpose(2, 0, 1), gpu)
    f1 = t(fine1[foff1[p]:foff1[p + 1]].reshape(*fg1[p], C).transpose(2, 0, 1), gpu)
    stub = lambda a, b: (torch.stack([c0, c0]), torch.stack([c1, c1]), torch.stack([f0, f0]), torch.stack([f1, f1]))  # noqa: E731
    model = CoarseToFine({'threshold': 0.0, 'border_rm': 0, 'cell': dsc.CELL, 'window': W, 'stride': stride},
                         net=stub, fine_net=lambda a, b: (a, b))
    res = model({'image0': torch.zeros(2, 1, 8, 8, device=gpu), 'image1': torch.zeros(2, 1, 8, 8, device=gpu)})
    lo, hi = want_win['moffsets'][p], want_win['moffsets'][p + 1]
    for b in range(2):
        assert np.array_equal(res['keypoints0'][b].cpu().numpy(), want_fine['mkpts0'][lo:hi])
        assert np.array_equal(res['keypoints1'][b].cpu().numpy(), want_fine['mkpts1'][lo:hi])
        assert res['matches0'][b].cpu().tolist() == list(range(hi - lo))
        rows = want_win['rows'][lo:hi, 1]
        assert np.array_equal(res['matching_scores0'][b].cpu().numpy(),
                              spec['matching_scores0'][call['off0'][p]:call['off0'][p + 1]][rows])
    assert hi - lo > 10
