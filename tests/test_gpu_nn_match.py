"""GPU tests of the nearest-neighbour matcher (``oetr_nn_match``, ``csrc/nn_match.hip``; ``nn_match.py``,
``dloc_matcher.py``).  There is no tolerance anywhere: every output of every call is compared for equality - the scores
by their bits - with the numpy specification ``tests/nn_match_oracle.py`` on ALL rows, on the pinned calls of
``tests/nn_match_cases.py`` (checked against the fixture in ``tests/test_nn_match_cpu.py``).  The unit-norm calls hold
the device's f32-input MFMA to the specification's ``fmaf`` chain; the grid calls, exact in any order, hold ties and
the mutual check under ties to "the lowest index wins"."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import match_assembly_oracle as mao  # noqa: E402
import nn_match_cases as nmc  # noqa: E402
import nn_match_oracle as nmo  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ('matches0', 'matching_scores0', 'matches1', 'counts')
F32 = np.float32


def t(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def upload(call, gpu):
    return dict(desc0=t(call['desc0'], gpu), desc1=t(call['desc1'], gpu), offsets0=t(call['off0'], gpu),
                offsets1=t(call['off1'], gpu), max_k0=call['max_k0'], max_k1=call['max_k1'])


def host(res):
    return {k: res[k].cpu().numpy() for k in OUTPUTS}


def assert_equal(got, want, tag=None):
    for k in OUTPUTS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, g.shape)
        if g.tobytes() != w.tobytes():
            rows = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(1))[0]
            raise AssertionError((tag, k, len(rows), rows[:8].tolist(), g[rows[:8]].tolist(), w[rows[:8]].tolist()))


def settings(ratio, distance, mutual):
    return dict(ratio_threshold=ratio, distance_threshold=distance, do_mutual_check=mutual)


@pytest.fixture(scope='module')
def device_calls(gpu):
    """Every pinned call on the device: made once, shared, never modified."""
    return {key: upload(nmc.make_call(*key), gpu) for key in nmc.CALLS}


@pytest.mark.parametrize('name,kind', nmc.CALLS)
def test_every_setting_equals_the_specification_bit_for_bit(gpu, device_calls, name, kind):
    import imagematching_oetr_amd as pkg
    call, dev = nmc.make_call(name, kind), device_calls[(name, kind)]
    for setting in nmc.SETTINGS:
        res = pkg.match_descriptors(**dev, **settings(*setting))
        assert_equal(host(res), nmc.expected(call, *setting), (name, kind, setting))
        assert np.array_equal(pkg.match_counts(res), host(res)['counts'])


def test_ties_go_to_the_lowest_index_in_both_directions(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    for name in ('ragged128', 'wide256'):
        call = nmc.make_call(name, 'grid')
        got = host(pkg.match_descriptors(**device_calls[(name, 'grid')], do_mutual_check=False))
        tied = 0
        for p, sim in enumerate(call['sims']):
            for m, s, off in ((got['matches0'], sim, call['off0']), (got['matches1'], sim.T, call['off1'])):
                if s.shape[1] < 2:
                    continue
                b1, i1, b2 = nmo.top2(s)
                rows = np.nonzero(b1 == b2)[0]                       # the maximum is attained at least twice
                tied += len(rows)
                mine = m[off[p]:off[p + 1]]
                assert np.array_equal(mine[rows], np.argmax(s[rows] == b1[rows, None], 1)), (name, p)
                assert np.array_equal(mine, i1), (name, p)
        assert tied >= 8, (name, tied)


def test_a_nan_row_is_never_matched_and_is_nobodys_neighbour(gpu):
    import imagematching_oetr_amd as pkg
    call = nmc.make_call('d512', 'unit')
    desc0, desc1 = call['desc0'].copy(), call['desc1'].copy()
    bad0, bad1 = int(call['off0'][0]) + 5, int(call['off1'][0]) + 9   # both in the first pair (65 x 64)
    desc0[bad0, 300] = np.nan
    desc1[bad1, ::7] = np.nan
    sims = [nmo.similarity(desc0[:65], desc1[:64])] + list(call['sims'][1:])
    for setting in ((None, None, True), (0.8, 0.7, False)):
        want = nmo.match_call(sims, len(desc0), len(desc1), call['off0'], call['off1'], *setting)
        got = host(pkg.match_descriptors(t(desc0, gpu), t(desc1, gpu), t(call['off0'], gpu), t(call['off1'], gpu),
                                         max_k0=65, max_k1=65, **settings(*setting)))
        assert_equal(got, want, setting)
        assert got['matches0'][bad0] == -1 and got['matching_scores0'][bad0] == 0 and got['matches1'][bad1] == -1
        assert not (got['matches0'][:65] == 9).any() and not (got['matches1'][:64] == 5).any()
    assert (got['matches0'][:65] > -1).sum() > 0


def test_a_pair_beyond_max_k_is_not_matched_and_every_row_is_written(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    call = nmc.make_call('ragged128', 'unit')
    dev = dict(device_calls[('ragged128', 'unit')])
    # rows no pair owns: four in front of side 0, three behind side 1
    desc0 = torch.cat([torch.full((4, 128), float('nan'), device=gpu), dev['desc0']])
    desc1 = torch.cat([dev['desc1'], torch.full((3, 128), float('nan'), device=gpu)])
    off0 = call['off0'] + 4
    for max_k0, max_k1 in ((129, 300), (300, 129), (64, 64)):
        out = pkg.match_descriptors(desc0, desc1, t(off0, gpu), dev['offsets1'], max_k0=max_k0, max_k1=max_k1,
                                    ratio_threshold=0.8)
        for k in OUTPUTS:                                            # poison: "written on every call" is seen
            out[k].fill_(77)
        res = pkg.match_descriptors(desc0, desc1, t(off0, gpu), dev['offsets1'], max_k0=max_k0, max_k1=max_k1,
                                    ratio_threshold=0.8, out=out)
        want = nmc.expected(call, 0.8, None, True, max_k0=max_k0, max_k1=max_k1)
        want['matches0'] = np.concatenate([np.full(4, -1, np.int32), want['matches0']])
        want['matching_scores0'] = np.concatenate([np.zeros(4, F32), want['matching_scores0']])
        want['matches1'] = np.concatenate([want['matches1'], np.full(3, -1, np.int32)])
        got = host(res)
        assert_equal(got, want, (max_k0, max_k1))
        beyond = [p for p, (K0, K1) in enumerate(call['pairs']) if K0 > max_k0 or K1 > max_k1]
        assert beyond and (got['counts'][beyond] == -1).all() and (got['counts'][:, 0] >= 0).sum() == 12 - len(beyond)
        for p in beyond:
            assert (got['matches0'][off0[p]:off0[p + 1]] == -1).all() and (got['matching_scores0'][off0[p]:off0[p + 1]] == 0).all()


def test_two_calls_give_equal_bits_out_is_reused_and_a_graph_replays(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    call = nmc.make_call('wide256', 'unit')
    dev = dict(device_calls[('wide256', 'unit')])
    dev['desc0'] = dev['desc0'].clone()
    kw = settings(0.8, 0.7, True)
    first, again = host(pkg.match_descriptors(**dev, **kw)), host(pkg.match_descriptors(**dev, **kw))
    assert_equal(again, first, 'two eager calls')
    assert_equal(first, nmc.expected(call, 0.8, 0.7, True), 'specification')
    out = pkg.match_descriptors(**dev, **kw)
    ptrs = {k: out[k].data_ptr() for k in OUTPUTS}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert pkg.match_descriptors(**dev, **settings(None, None, False), out=out) is out
    assert torch.cuda.memory_allocated() == before and {k: out[k].data_ptr() for k in OUTPUTS} == ptrs
    assert_equal(host(out), nmc.expected(call, None, None, False), 'reused')
    with pytest.raises(ValueError, match='other sizes'):
        pkg.match_descriptors(**device_calls[('d4', 'unit')], out=out)
    # captured, replayed, replayed on other descriptors, and on the first ones again
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.match_descriptors(**dev, **kw)
        with pytest.raises(ValueError, match='inside a graph capture'):              # host offsets: refused, nothing enqueued
            pkg.match_descriptors(dev['desc0'], dev['desc1'], call['off0'], call['off1'], max_k0=300, max_k1=300)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal(host(captured), first, 'replay')
    kept = dev['desc0'].clone()
    dev['desc0'].copy_(kept.roll(37, 0))
    graph.replay()
    torch.cuda.synchronize()
    moved = host(captured)
    assert_equal(moved, host(pkg.match_descriptors(**dev, **kw)), 'replay on other descriptors')
    assert not np.array_equal(moved['matches0'], first['matches0'])
    dev['desc0'].copy_(kept)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal(host(captured), first, 'replay on the first descriptors')


def test_without_a_matches1_output_direction_one_lives_in_the_workspace(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    from imagematching_oetr_amd import hip_engine
    lib = pkg.load_library()
    call, dev = nmc.make_call('ragged128', 'grid'), device_calls[('ragged128', 'grid')]
    N0, N1, P = len(call['desc0']), len(call['desc1']), len(call['pairs'])
    ws_bytes = lib.oetr_nn_match_workspace_bytes(N1)
    assert ws_bytes >= 4 * N1
    ws = torch.full((ws_bytes,), 0x5a, dtype=torch.uint8, device=gpu)
    m0 = torch.full((N0,), 77, dtype=torch.int32, device=gpu)
    s0 = torch.full((N0,), 77.0, device=gpu)
    counts = torch.full((P, 4), 77, dtype=torch.int32, device=gpu)
    flags = hip_engine.NN_MATCH_RATIO | hip_engine.NN_MATCH_MUTUAL
    status = lib.oetr_nn_match(dev['desc0'].data_ptr(), dev['offsets0'].data_ptr(), N0, dev['desc1'].data_ptr(),
                               dev['offsets1'].data_ptr(), N1, P, call['D'], call['max_k0'], call['max_k1'],
                               float(F32(0.8 * 0.8)), 0.0, flags, ws.data_ptr(), ws_bytes, m0.data_ptr(), s0.data_ptr(),
                               None, counts.data_ptr(), hip_engine._stream(gpu))
    assert status == 0, lib.oetr_last_error()
    torch.cuda.synchronize()
    got = dict(matches0=m0.cpu().numpy(), matching_scores0=s0.cpu().numpy(), counts=counts.cpu().numpy(),
               matches1=ws[:4 * N1].cpu().numpy().view(np.int32))
    assert_equal(got, nmc.expected(call, 0.8, None, True), 'matches1 = NULL')
    assert (ws[4 * N1:] == 0x5a).all()                              # nothing behind direction 1's rows is touched


def test_more_pairs_than_one_grid_dimension(gpu):
    import imagematching_oetr_amd as pkg
    many = nmc.many_small_pairs()
    assert len(many['off0']) - 1 == 65538
    res = pkg.match_descriptors(t(many['desc0'], gpu), t(many['desc1'], gpu), t(many['off0'], gpu), t(many['off1'], gpu),
                                max_k0=3, max_k1=3, **many['settings'])
    want = many['expected']
    assert_equal(host(res), want, '65538 pairs')
    assert (want['counts'][-3:, 2] >= 0).all() and 0 < (want['matches0'] > -1).sum() < len(want['matches0'])


def test_per_pair_form_channels_first_and_float16(gpu):
    import imagematching_oetr_amd as pkg
    call = nmc.make_call('d4', 'grid')                               # k / 64: exact in float16 too
    parts0 = [call['desc0'][a:b] for a, b in zip(call['off0'][:-1], call['off0'][1:])]
    parts1 = [call['desc1'][a:b] for a, b in zip(call['off1'][:-1], call['off1'][1:])]
    want = nmc.expected(call, 0.8, None, True)
    assert_equal(host(pkg.match_descriptors([t(a, gpu) for a in parts0], [t(b, gpu) for b in parts1],
                                            ratio_threshold=0.8)), want, 'device tensors per pair')
    assert_equal(host(pkg.match_descriptors([a.T.copy() for a in parts0], [torch.from_numpy(b.T.copy()) for b in parts1],
                                            ratio_threshold=0.8, channels_first=True)), want, 'host [D,K] per pair')
    assert_equal(host(pkg.match_descriptors([t(a, gpu).half() for a in parts0], [t(b, gpu).half() for b in parts1],
                                            ratio_threshold=0.8)), want, 'float16')
    flat = torch.empty(call['desc0'].size + 1, device=gpu)          # a view at an odd float: rows off the 16-byte grid
    odd = flat[1:].view(-1, 4)
    odd.copy_(t(call['desc0'], gpu))
    assert odd.data_ptr() % 16 == 4
    assert_equal(host(pkg.match_descriptors(odd, t(call['desc1'], gpu), t(call['off0'], gpu), t(call['off1'], gpu),
                                            max_k0=65, max_k1=65, ratio_threshold=0.8)), want, 'odd view')
    with pytest.raises(ValueError, match='D % 4'):
        pkg.match_descriptors([torch.zeros(3, 6, device=gpu)], [torch.zeros(3, 6, device=gpu)])


def test_the_result_feeds_assemble_matches_as_it_is(gpu, device_calls):
    import imagematching_oetr_amd as pkg
    call = nmc.make_call('ragged128', 'unit')
    geometry = mao.make_call(5, tuple((K0, K1, 'none', 1) for K0, K1 in call['pairs']))   # hand-made records
    assert np.array_equal(geometry['off0'], call['off0']) and np.array_equal(geometry['off1'], call['off1'])
    res = pkg.match_descriptors(**device_calls[('ragged128', 'unit')], ratio_threshold=0.8, distance_threshold=0.7)
    records = torch.from_numpy(np.ascontiguousarray(geometry['info']).view(np.uint8).reshape(len(geometry['info']), -1)
                               .copy()).to(gpu)
    lists = pkg.assemble_matches(records, t(geometry['scales'], gpu), t(geometry['kp0'], gpu), t(geometry['kp1'], gpu),
                                 res['matches0'], res['matching_scores0'],
                                 offsets0=device_calls[('ragged128', 'unit')]['offsets0'],
                                 offsets1=device_calls[('ragged128', 'unit')]['offsets1'])
    spec = nmc.expected(call, 0.8, 0.7, True)
    want = mao.assemble(**dict(geometry, matches=spec['matches0'], conf=spec['matching_scores0']))
    assert want['offsets'][-1] == (spec['matches0'] > -1).sum() > 100
    for k, w in want.items():
        assert mao.equal_bits(lists[k].cpu().numpy(), w), k


def test_the_plug_in_on_a_batch(gpu):
    from imagematching_oetr_amd.dloc_matcher import NearestNeighbor
    rng = np.random.default_rng(17)
    pairs = [nmc.unit_pair(rng, 200, 180, 128) for _ in range(2)]
    sims = [nmo.similarity(a, b) for a, b in pairs]
    data = {'descriptors0': t(np.stack([a.T for a, _ in pairs]), gpu),           # [2,128,200]
            'descriptors1': t(np.stack([b.T for _, b in pairs]), gpu)}           # [2,128,180]
    assert tuple(data['descriptors0'].shape) == (2, 128, 200) and tuple(data['descriptors1'].shape) == (2, 128, 180)
    for conf in ({}, {'ratio_threshold': 0.8, 'distance_threshold': 0.7}, {'ratio_threshold': 0.8, 'do_mutual_check': False}):
        out = NearestNeighbor(conf)(data)
        assert out['matches0'].dtype == torch.int64 and tuple(out['matches0'].shape) == (2, 200)
        assert out['matching_scores0'].dtype == torch.float32 and tuple(out['matching_scores0'].shape) == (2, 200)
        for b, sim in enumerate(sims):
            want = nmo.match_similarity(sim, conf.get('ratio_threshold'), conf.get('distance_threshold'),
                                        conf.get('do_mutual_check', True))
            assert np.array_equal(out['matches0'][b].cpu().numpy(), want['matches0'].astype(np.int64)), (conf, b)
            assert out['matching_scores0'][b].cpu().numpy().tobytes() == want['matching_scores0'].tobytes(), (conf, b)
