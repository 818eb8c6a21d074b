"""GPU tests of the dual-softmax coarse matcher (``oetr_dual_softmax_match``, ``csrc/dual_softmax.hip``;
``dense_match.py``, ``dloc_matcher.DualSoftmax``).  There is no tolerance anywhere: every output of every call is
compared for equality - the scores and keypoints by their bits - with the numpy specification
``tests/dual_softmax_oracle.py`` on ALL rows, on the pinned calls of ``tests/dual_softmax_cases.py`` (checked against
the fixture in ``tests/test_dual_softmax_cpu.py``).  The Gaussian calls hold the device's f32-input MFMA, its ``e``, its
sums and its divisions to the specification; the grid calls, whose similarities are exact in any order, hold ties in
both directions to "the lowest index wins"."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dual_softmax_cases as dsc  # noqa: E402
import dual_softmax_oracle as dso  # noqa: E402
import match_assembly_oracle as mao  # noqa: E402
import nn_match_oracle as nmo  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ('matches0', 'matching_scores0', 'matches1', 'keypoints0', 'keypoints1', 'counts')
F32 = np.float32


def t(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def upload(call, gpu):
    return dict(feat0=t(call['feat0'], gpu), feat1=t(call['feat1'], gpu), offsets0=t(call['off0'], gpu),
                offsets1=t(call['off1'], gpu), grids0=t(call['grids0'], gpu), grids1=t(call['grids1'], gpu),
                max_k0=call['max_k0'], max_k1=call['max_k1'])


def host(res):
    return {k: res[k].cpu().numpy() for k in OUTPUTS}


def assert_equal(got, want, tag=None, keys=OUTPUTS):
    for k in keys:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            rows = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(1))[0]
            raise AssertionError((tag, k, len(rows), rows[:8].tolist(), g[rows[:8]].tolist(), w[rows[:8]].tolist()))


def settings(temperature, threshold, border_rm):
    return dict(temperature=temperature, threshold=threshold, border_rm=border_rm, cell=dsc.CELL)


def one_pair(A, B, g0, g1, gpu, **kw):
    """One pair in the joined form, and the specification's result of it."""
    import imagematching_oetr_amd as pkg
    L, S = len(A), len(B)
    res = pkg.match_dense(t(A, gpu), t(B, gpu), t(np.array([0, L], np.int32), gpu), t(np.array([0, S], np.int32), gpu),
                          t(np.array([g0], np.int32), gpu), t(np.array([g1], np.int32), gpu), max_k0=L, max_k1=S, **kw)
    tt = (nmo.similarity(A, B) * dso.scale_of(A.shape[1], kw.get('temperature', 0.1))).astype(F32)
    want = dso.match_call([tt], [g0], [g1], L, S, [0, L], [0, S], kw.get('threshold', 0.2), kw.get('border_rm', 2),
                          kw.get('cell', 8))
    return host(res), want, tt


@pytest.fixture(scope='module')
def device_calls(gpu):
    """Every pinned call on the device: made once, shared, never modified."""
    return {key: upload(dsc.make_call(*key), gpu) for key in dsc.CALLS}


@pytest.mark.parametrize('name,kind', dsc.CALLS)
def test_every_setting_equals_the_specification_bit_for_bit(gpu, device_calls, name, kind):
    import imagematching_oetr_amd as pkg
    call, dev = dsc.make_call(name, kind), device_calls[(name, kind)]
    for setting in dsc.SETTINGS:
        res = pkg.match_dense(**dev, **settings(*setting))
        assert_equal(host(res), dsc.expected(call, *setting), (name, kind, setting))
        assert np.array_equal(pkg.dense_match_counts(res), host(res)['counts'])


def test_ties_go_to_the_lowest_index_in_both_directions(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    for name in ('ragged64', 'd256'):
        call = dsc.make_call(name, 'grid')
        got = host(pkg.match_dense(**device_calls[(name, 'grid')], **settings(0.1, 0.0, 0)))
        tied = [0, 0]
        for p, tt in enumerate(dsc.ts_of(call, 0.1)):
            if min(tt.shape) < 2:
                continue
            conf, cand = dso.confidence(tt)
            for side, (c, k) in enumerate(((conf, cand), (conf.T, cand.T))):
                top, first = dso.best(c, k)
                attained = k & (c == top[:, None])
                rows = np.nonzero(attained.sum(1) >= 2)[0]                       # the maximum is attained at least twice
                tied[side] += len(rows)
                assert np.array_equal(first[rows], np.argmax(attained[rows], 1))
                if side:                                                         # direction 1's argmax, before the tests
                    assert np.array_equal(got['matches1'][call['off1'][p]:call['off1'][p + 1]], first), (name, p)
                else:                                                            # a kept row kept its lowest index
                    mine = got['matches0'][call['off0'][p]:call['off0'][p + 1]]
                    assert np.array_equal(mine[mine > -1], first[mine > -1]), (name, p)
        assert tied[0] >= 4 and tied[1] >= 4, (name, tied)


def test_an_all_equal_map_gives_one_over_l_times_s(gpu):
    A, B, g0, g1 = dsc.all_equal_call()
    got, want, _ = one_pair(A, B, g0, g1, gpu, temperature=0.1, threshold=0.0, border_rm=0)
    assert_equal(got, want, 'all equal')
    L, S = len(A), len(B)
    assert np.allclose(got['matching_scores0'], 1.0 / (L * S), rtol=1e-6, atol=0)
    assert (got['matches1'] == 0).all() and got['matches0'].tolist() == [0] + [-1] * (L - 1)    # ties: the lowest index
    assert got['counts'].tolist() == [[L, S, L, 1]]


def test_rows_that_cross_the_cut_off_of_e(gpu):
    A, B, g0, g1 = dsc.cutoff_pair()
    got, want, tt = one_pair(A, B, g0, g1, gpu, temperature=0.1, threshold=0.2, border_rm=0)
    assert_equal(got, want, 'cut-off')
    d = tt - tt.max(1, keepdims=True)
    assert (d < dso.E_CUT).any(1).all() and ((d > dso.E_CUT) & (d < 0)).any()       # every row has terms that are 0
    assert ((d > F32(-90)) & (d < F32(-84))).sum() >= 1                              # and the call has terms at the cut-off
    conf, cand = dso.confidence(tt)
    assert (np.isfinite(tt) & ~cand).any()                                           # factors below 2^-62: no candidates
    assert got['counts'][0, 3] > 10


def test_a_nan_row_and_an_infinite_entry_are_never_matched(gpu):
    call = dsc.make_call('d68', 'gauss')
    A = call['feat0'][call['off0'][0]:call['off0'][1]].copy()      # 65 x 129, D = 68
    B = call['feat1'][call['off1'][0]:call['off1'][1]].copy()
    A[5, 40] = np.nan                                              # row 5 of t is NaN
    B[9, ::7] = np.nan                                             # column 9 of t is NaN
    A[11, 3], B[100, 3] = np.inf, 1.0                              # t[11][100] = +inf, t[11][others] NaN or +-inf
    B[64, 1] = -np.inf                                             # column 64: -inf, +inf or NaN
    got, want, tt = one_pair(A, B, (5, 13), (3, 43), gpu, temperature=0.1, threshold=0.0, border_rm=0)
    assert np.isnan(tt[5]).all() and np.isnan(tt[:, 9]).all() and np.isinf(tt[11, 100]) and not np.isfinite(tt[:, 64]).any()
    assert_equal(got, want, 'non-finite')
    for i in (5, 11):
        assert got['matches0'][i] == -1 and got['matching_scores0'][i] == 0 and not (got['matches1'] == i).any()
    for j in (9, 64):
        assert got['matches1'][j] == -1 and not (got['matches0'] == j).any()
    assert (got['matches0'] > -1).sum() > 10
    # absent from every sum: the other rows' results are those of the call without row 5 / 11 and column 9 / 64
    keep0, keep1 = np.setdiff1d(np.arange(65), (5, 11)), np.setdiff1d(np.arange(129), (9, 64))
    conf, _ = dso.confidence(tt[np.ix_(keep0, keep1)])
    full, _ = dso.confidence(tt)
    sub = full[np.ix_(keep0, keep1)]
    both = (sub >= 0) & (conf >= 0)
    assert both.mean() > 0.2 and np.allclose(sub[both], conf[both], rtol=1e-5, atol=0)


def test_pairs_that_are_not_vouched_for_are_not_read_and_guards_stay(gpu, device_calls):
    """A pair beyond ``max_k*`` and pairs whose ``grids`` disagree with their rows: -1 counters, rows -1 / 0 / NaN.
    Every output and the workspace sit between guard rows that no launch may touch."""
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd import hip_engine
    lib = pkg.load_library()
    call, dev = dsc.make_call('ragged64', 'gauss'), device_calls[('ragged64', 'gauss')]
    N0, N1, P, guard = len(call['feat0']), len(call['feat1']), len(call['pairs']), 64
    grids0, grids1 = call['grids0'].copy(), call['grids1'].copy()
    grids0[4] = (5, 12)                                             # 60 != 65 rows
    grids1[5] = (-3, -43)                                           # negative, product 129
    grids1[6] = (127, 2)                                            # twice its rows
    wrong = [4, 5, 6]
    # rows no pair owns: three in front of side 0, two behind side 1
    feat0 = torch.cat([torch.full((3, 64), float('nan'), device=gpu), dev['feat0']])
    feat1 = torch.cat([dev['feat1'], torch.full((2, 64), float('nan'), device=gpu)])
    off0 = call['off0'] + 3
    need = lib.oetr_dual_softmax_workspace_bytes(N0 + 3, N1 + 2)
    shapes = dict(matches0=(N0 + 3,), matching_scores0=(N0 + 3,), matches1=(N1 + 2,), keypoints0=(N0 + 3, 2),
                  keypoints1=(N1 + 2, 2), counts=(P, 4))
    ints = ('matches0', 'matches1', 'counts')
    for max_k0, max_k1 in ((300, 300), (129, 300), (300, 128)):
        whole, out = {}, {}
        for key, shape in shapes.items():
            whole[key] = torch.full((shape[0] + 2 * guard,) + shape[1:], 77,
                                    dtype=torch.int32 if key in ints else torch.float32, device=gpu)
            out[key] = whole[key][guard:guard + shape[0]]
        whole['workspace'] = torch.full((need + 512,), 0x5a, dtype=torch.uint8, device=gpu)
        out['workspace'] = whole['workspace'][256:256 + need]
        res = pkg.match_dense(feat0, feat1, t(off0, gpu), dev['offsets1'], t(grids0, gpu), t(grids1, gpu), max_k0=max_k0,
                              max_k1=max_k1, out=out, **settings(0.1, 0.2, 1))
        assert res is out
        ts = dsc.ts_of(call, 0.1)
        want = dso.match_call(ts, grids0, grids1, N0 + 3, N1 + 2, off0, call['off1'], 0.2, 1, dsc.CELL, max_k0, max_k1)
        got = host(res)
        assert_equal(got, want, (max_k0, max_k1))
        beyond = [p for p, (L, S) in enumerate(call['pairs']) if L > max_k0 or S > max_k1]
        assert (got['counts'][wrong + beyond] == -1).all() and (got['counts'][:, 0] >= 0).sum() == P - len(set(wrong + beyond))
        for p in wrong + beyond:
            rows = slice(off0[p], off0[p + 1])
            assert (got['matches0'][rows] == -1).all() and (got['matching_scores0'][rows] == 0).all()
            assert np.isnan(got['keypoints0'][rows]).all()
        assert np.isnan(got['keypoints0'][:3]).all() and np.isnan(got['keypoints1'][-2:]).all()
        for key, shape in shapes.items():
            assert (whole[key][:guard] == 77).all() and (whole[key][guard + shape[0]:] == 77).all(), key
        assert (whole['workspace'][:256] == 0x5a).all() and (whole['workspace'][256 + need:] == 0x5a).all()
    assert len(beyond) >= 1 and hip_engine.DUAL_SOFTMAX_COUNTERS == 4


def test_two_calls_give_equal_bits_out_is_reused_and_a_graph_replays(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    call = dsc.make_call('d256', 'gauss')
    dev = dict(device_calls[('d256', 'gauss')])
    dev['feat0'] = dev['feat0'].clone()
    kw = settings(0.1, 0.0, 0)
    first, again = host(pkg.match_dense(**dev, **kw)), host(pkg.match_dense(**dev, **kw))
    assert_equal(again, first, 'two eager calls')
    assert_equal(first, dsc.expected(call, 0.1, 0.0, 0), 'specification')
    out = pkg.match_dense(**dev, **kw)
    ptrs = {k: out[k].data_ptr() for k in OUTPUTS + ('workspace',)}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert pkg.match_dense(**dev, **settings(1.0, 0.0, 1), out=out) is out
    assert torch.cuda.memory_allocated() == before and {k: out[k].data_ptr() for k in OUTPUTS + ('workspace',)} == ptrs
    assert_equal(host(out), dsc.expected(call, 1.0, 0.0, 1), 'reused')
    with pytest.raises(ValueError, match='other sizes'):
        pkg.match_dense(**device_calls[('d4', 'gauss')], out=out)
    # captured, replayed, replayed on other features, and on the first ones again
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.match_dense(**dev, **kw)
        with pytest.raises(ValueError, match='inside a graph capture'):              # host offsets: refused, nothing enqueued
            pkg.match_dense(dev['feat0'], dev['feat1'], call['off0'], call['off1'], dev['grids0'], dev['grids1'],
                            max_k0=300, max_k1=300)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal(host(captured), first, 'replay')
    kept = dev['feat0'].clone()
    dev['feat0'][:300] = kept[:300].roll(37, 0)                    # within the first pair: the grids still hold
    graph.replay()
    torch.cuda.synchronize()
    moved = host(captured)
    assert_equal(moved, host(pkg.match_dense(**dev, **kw)), 'replay on other features')
    assert not np.array_equal(moved['matches0'], first['matches0'])
    dev['feat0'].copy_(kept)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal(host(captured), first, 'replay on the first features')


def test_without_a_matches1_output_direction_one_lives_in_the_workspace(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd import hip_engine
    lib = pkg.load_library()
    call, dev = dsc.make_call('ragged64', 'grid'), device_calls[('ragged64', 'grid')]
    N0, N1, P = len(call['feat0']), len(call['feat1']), len(call['pairs'])
    ws_bytes = lib.oetr_dual_softmax_workspace_bytes(N0, N1)
    pad = lambda b: (b + 255) // 256 * 256
    assert ws_bytes == pad(8 * N0) + pad(8 * N1) + pad(4 * N1)
    ws = torch.full((ws_bytes + 256,), 0x5a, dtype=torch.uint8, device=gpu)
    m0 = torch.full((N0,), 77, dtype=torch.int32, device=gpu)
    s0 = torch.full((N0,), 77.0, device=gpu)
    kp0, kp1 = torch.full((N0, 2), 77.0, device=gpu), torch.full((N1, 2), 77.0, device=gpu)
    counts = torch.full((P, 4), 77, dtype=torch.int32, device=gpu)
    status = lib.oetr_dual_softmax_match(
        dev['feat0'].data_ptr(), dev['offsets0'].data_ptr(), dev['grids0'].data_ptr(), N0, dev['feat1'].data_ptr(),
        dev['offsets1'].data_ptr(), dev['grids1'].data_ptr(), N1, P, call['D'], call['max_k0'], call['max_k1'],
        float(dso.scale_of(call['D'], 0.1)), 0.2, 2, dsc.CELL, ws.data_ptr(), ws_bytes, m0.data_ptr(), s0.data_ptr(),
        None, kp0.data_ptr(), kp1.data_ptr(), counts.data_ptr(), hip_engine._stream(gpu))
    assert status == 0, lib.oetr_last_error()
    torch.cuda.synchronize()
    at = pad(8 * N0) + pad(8 * N1)
    got = dict(matches0=m0.cpu().numpy(), matching_scores0=s0.cpu().numpy(), counts=counts.cpu().numpy(),
               keypoints0=kp0.cpu().numpy(), keypoints1=kp1.cpu().numpy(),
               matches1=ws[at:at + 4 * N1].cpu().numpy().view(np.int32))
    assert_equal(got, dsc.expected(call, 0.1, 0.2, 2), 'matches1 = NULL')
    assert (ws[ws_bytes:] == 0x5a).all()                            # nothing behind the workspace is touched


def test_more_pairs_than_one_grid_dimension(gpu):
    import imagematching_oetr_amd as pkg
    many = dsc.many_small_pairs()
    assert len(many['off0']) - 1 == 65538
    grids = t(many['grids'], gpu)
    res = pkg.match_dense(t(many['feat0'], gpu), t(many['feat1'], gpu), t(many['off0'], gpu), t(many['off1'], gpu), grids,
                          grids, max_k0=4, max_k1=4, cell=dsc.CELL, **many['settings'])
    want = many['expected']
    assert_equal(host(res), want, '65538 pairs')
    assert (want['counts'][-3:, 0] == 4).all() and 0 < (want['matches0'] > -1).sum() < len(want['matches0'])


def test_per_pair_form_and_channels_first(gpu):
    import imagematching_oetr_amd as pkg
    call = dsc.make_call('borders', 'gauss')
    D = call['D']
    maps0 = [call['feat0'][a:b].reshape(*g, D) for a, b, g in zip(call['off0'][:-1], call['off0'][1:], call['grids0'])]
    maps1 = [call['feat1'][a:b].reshape(*g, D) for a, b, g in zip(call['off1'][:-1], call['off1'][1:], call['grids1'])]
    for setting in ((0.1, 0.2, 2), (0.1, 0.0, 1)):
        want = dsc.expected(call, *setting)
        kw = settings(*setting)
        assert_equal(host(pkg.match_dense([t(a, gpu) for a in maps0], [t(b, gpu) for b in maps1], **kw)), want,
                     'device maps per pair')
        assert_equal(host(pkg.match_dense([np.array(a.transpose(2, 0, 1)) for a in maps0],
                                          [torch.from_numpy(np.array(b.transpose(2, 0, 1))) for b in maps1],
                                          channels_first=True, **kw)), want, 'host [D,h,w] per pair')
    assert (want['counts'][:, 3] > 0).any() and (want['counts'][:, 3] == 0).any()
    with pytest.raises(ValueError, match='D % 4'):
        pkg.match_dense([torch.zeros(3, 3, 6, device=gpu)], [torch.zeros(3, 3, 6, device=gpu)])


def test_the_result_feeds_assemble_matches_and_the_homography_score_as_it_is(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    call, dev = dsc.make_call('ragged64', 'gauss'), device_calls[('ragged64', 'gauss')]
    geometry = mao.make_call(5, tuple((L, S, 'none', 1) for L, S in call['pairs']))       # hand-made records
    assert np.array_equal(geometry['off0'], call['off0']) and np.array_equal(geometry['off1'], call['off1'])
    res = pkg.match_dense(**dev, **settings(0.1, 0.0, 0))
    records = torch.from_numpy(np.ascontiguousarray(geometry['info']).view(np.uint8).reshape(len(geometry['info']), -1)
                               .copy()).to(gpu)
    lists = pkg.assemble_matches(records, t(geometry['scales'], gpu), res['keypoints0'], res['keypoints1'],
                                 res['matches0'], res['matching_scores0'], offsets0=dev['offsets0'],
                                 offsets1=dev['offsets1'])
    spec = dsc.expected(call, 0.1, 0.0, 0)
    want = mao.assemble(**dict(geometry, kp0=spec['keypoints0'], kp1=spec['keypoints1'], matches=spec['matches0'],
                               conf=spec['matching_scores0']))
    assert want['offsets'][-1] == (spec['matches0'] > -1).sum() > 100
    for k, w in want.items():
        assert mao.equal_bits(lists[k].cpu().numpy(), w), k
    P = len(call['pairs'])
    scored = pkg.score_matches_homography(np.tile(np.eye(3), (P, 1, 1)), lists['k1'], lists['k2'],
                                          offsets=lists['offsets'], thresholds=(1, 3))
    assert scored['counts'][:, 0].cpu().tolist() == spec['counts'][:, 3].tolist()


def test_the_plug_in_on_a_batch_with_a_stub_net(gpu):
    from imagematching_oetr_amd.dloc_matcher import DualSoftmax
    rng = np.random.default_rng(17)
    pairs = [dsc.gauss_pair(rng, 63, 20, 32) for _ in range(2)]     # 7 x 9 and 4 x 5 grids
    f0 = t(np.stack([a.reshape(7, 9, 32).transpose(2, 0, 1) for a, _ in pairs]), gpu)    # [2,32,7,9]
    f1 = t(np.stack([b.reshape(4, 5, 32).transpose(2, 0, 1) for _, b in pairs]), gpu)    # [2,32,4,5]
    seen = []

    def net(image0, image1):
        seen.append((tuple(image0.shape), tuple(image1.shape)))
        return f0, f1

    data = {'image0': torch.zeros(2, 1, 56, 72, device=gpu), 'image1': torch.zeros(2, 1, 32, 40, device=gpu)}
    assert DualSoftmax.required_inputs == ['image0', 'image1']
    for conf in ({}, {'threshold': 0.0, 'border_rm': 0}, {'temperature': 1.0, 'border_rm': 1, 'cell': 4}):
        out = DualSoftmax(conf, net=net)(data)
        full = {**DualSoftmax.default_conf, **conf}
        assert sorted(out) == ['keypoints0', 'keypoints1', 'matches0', 'matching_scores0']
        for b, (A, B) in enumerate(pairs):
            want = dso.match_pair(A, B, (7, 9), (4, 5), full['temperature'], full['threshold'], full['border_rm'])
            assert out['matches0'][b].dtype == torch.int64 and tuple(out['matches0'][b].shape) == (63,)
            assert np.array_equal(out['matches0'][b].cpu().numpy(), want['matches0'].astype(np.int64)), (conf, b)
            assert out['matching_scores0'][b].cpu().numpy().tobytes() == want['matching_scores0'].tobytes(), (conf, b)
            assert np.array_equal(out['keypoints0'][b].cpu().numpy(), dso.keypoints(7, 9, full['cell']))
            assert np.array_equal(out['keypoints1'][b].cpu().numpy(), dso.keypoints(4, 5, full['cell']))
    assert seen[0] == ((2, 1, 56, 72), (2, 1, 32, 40)) and (want['matches0'] == -1).any()
