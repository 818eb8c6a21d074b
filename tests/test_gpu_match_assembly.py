"""GPU tests of the match-assembly extension (``oetr_assemble_matches``, ``csrc/match_assembly.hip``;
``match_assembly.py``).  There is no tolerance anywhere: every output is compared for equality or BIT FOR BIT
(``mao.equal_bits``: NaN equals NaN) with the numpy specification ``tests/match_assembly_oracle.py``, whose pinned call
(17 pairs; ``K0`` up to 2049, three chunks of a workgroup) is checked in ``tests/test_match_assembly_cpu.py``."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import match_assembly_oracle as mao  # noqa: E402
import match_score_oracle as mso  # noqa: E402

pytestmark = pytest.mark.gpu
EXPECTED = json.loads((REPO / 'tests' / 'match_assembly_expected.json').read_text())
OUTPUTS = ('origin0', 'origin1', 'index0', 'index1', 'k1', 'k2', 'mconf', 'offsets', 'counts', 'few', 'n_few')
DTYPES = dict(origin0=torch.float64, origin1=torch.float64, index0=torch.int32, index1=torch.int32, k1=torch.float32,
              k2=torch.float32, mconf=torch.float32, offsets=torch.int32, counts=torch.int32, few=torch.int32,
              n_few=torch.int32)


def records(info, gpu):
    """``INFO_DTYPE [P]`` -> the device tensor of the records, byte for byte."""
    return torch.from_numpy(np.ascontiguousarray(info).view(np.uint8).reshape(len(info), -1).copy()).to(gpu)


def upload(call, gpu, match_dtype=np.int32):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return dict(crops=records(call['info'], gpu), scales=t(call['scales']), kp0=t(call['kp0']), kp1=t(call['kp1']),
                matches=t(call['matches'].astype(match_dtype)), conf=t(call['conf']), offsets0=t(call['off0']),
                offsets1=t(call['off1']))


def host(res):
    return {k: res[k].cpu().numpy() for k in OUTPUTS if k in res}


def assert_equal(got, want, tag=None):
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for k in want:
        assert mao.equal_bits(got[k], want[k]), (tag, k)


@pytest.fixture(scope='module')
def pinned(gpu):
    """The pinned call, its specified result and the device inputs: made once, shared, never modified."""
    call = mao.make_call(EXPECTED['seed'])
    assert mao.input_hashes(call) == EXPECTED['inputs_sha256']      # a wrong input cannot pass as a wrong kernel
    return dict(call=call, want=mao.assemble(**call), dev=upload(call, gpu))


@pytest.mark.parametrize('match_dtype', [np.int32, np.int64])
def test_pinned_call_equals_the_specification(gpu, pinned, match_dtype):
    import imagematching_oetr_amd as pkg
    dev = dict(pinned['dev'], matches=pinned['dev']['matches'].to({np.int32: torch.int32, np.int64: torch.int64}[match_dtype]))
    res = pkg.assemble_matches(**dev)
    for k in OUTPUTS:
        assert res[k].dtype == DTYPES[k] and res[k].is_cuda, k
    N0, N1, P = len(pinned['call']['kp0']), len(pinned['call']['kp1']), len(mao.PAIRS)
    assert res['origin0'].shape == (N0, 2) and res['origin1'].shape == (N1, 2) and res['k2'].shape == (N0, 2)
    assert res['index0'].shape == (N0,) and res['offsets'].shape == (P + 1,) and res['counts'].shape == (P, 4)
    got = host(res)
    assert_equal(got, pinned['want'], match_dtype)
    assert got['counts'].tolist() == EXPECTED['counts'] and got['offsets'].tolist() == EXPECTED['offsets']
    assert got['few'].tolist() == EXPECTED['few'] and int(got['n_few'][0]) == EXPECTED['n_few']
    total = EXPECTED['offsets'][-1]                                  # the tail, spelled out
    assert 0 < total < N0 and (got['index0'][total:] == -1).all() and (got['index1'][total:] == -1).all()
    assert all(np.isnan(got[k][total:]).all() for k in ('k1', 'k2', 'mconf'))
    assert pkg.few_match_pairs(res) == EXPECTED['few'][:EXPECTED['n_few']]
    # k2 is the rounded origin1 row, by construction
    for p in range(P):
        lo, hi = got['offsets'][p], got['offsets'][p + 1]
        rows = int(pinned['call']['off1'][p]) + got['index1'][lo:hi]
        assert mao.equal_bits(got['k2'][lo:hi], got['origin1'][rows].astype(np.float32)), p
    # without conf and without the selection: the same lists
    bare = pkg.assemble_matches(**dict(dev, conf=None), min_matches=None)
    assert sorted(k for k in bare if not k.startswith('_')) == sorted(set(OUTPUTS) - {'mconf', 'few', 'n_few'})
    assert_equal(host(bare), {k: v for k, v in pinned['want'].items() if k not in ('mconf', 'few', 'n_few')}, 'bare')
    other = host(pkg.assemble_matches(**dev, min_matches=21))
    assert other['few'][:int(other['n_few'][0])].tolist() == [p for p, c in enumerate(EXPECTED['counts']) if c[2] < 21]


def test_the_real_chain_on_tiny_images(gpu):
    """``overlap_crop_batch`` records straight from the device (a cropping pair, a failed gate, a degenerate box, a
    pair with other scales), one tensor per pair: the origin arrays equal the per-pair ``to_origin`` route, and scoring
    the device lists by ``offsets`` equals scoring the host-assembled float32 lists by ``lengths``."""
    import imagematching_oetr_amd as pkg
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(3)
    im = torch.rand(1, 1, 64, 64, generator=g).to(gpu)
    other = torch.rand(1, 1, 50, 77, generator=g).to(gpu)
    inside, outside = [5.0, 5.0, 60.0, 60.0], [70.0, 10.0, 100.0, 50.0]
    thin = [10.0, 10.0, 11.9, 50.0]
    ims0, ims1 = [im, im, im, other], [other, other, im, im]
    box0 = torch.tensor([inside, thin, outside, [3.3, 4.1, 33.0, 31.0]]).to(gpu)
    box1 = torch.tensor([[3.0, 4.0, 70.0, 45.0], inside, inside, [11.5, 2.25, 40.0, 38.0]]).to(gpu)
    crop_scales = [(1.0, 1.0)] * 3 + [(1.6, 1.3)], [(1.0, 1.0)] * 3 + [(0.75, 0.6)]
    table = pkg.crop_pair_table(ims0, ims1, *crop_scales)
    batch = pkg.overlap_crop_batch(table, box0, box1, keep_aspect=True, size_divisor=1)
    scales = np.array([[(1.6, 1.6), (0.75, 0.8)], [(1.0, 1.0), (1.25, 1.25)], [(1.0, 1.0), (1.0, 1.0)],
                       [(0.9, 1.1), (1.6, 0.75)]])
    K0, K1 = (70, 257, 33, 300), (64, 100, 40, 1)
    kp0 = [rng.uniform(0, 60, size=(n, 2)).astype(np.float32) for n in K0]
    kp1 = [rng.uniform(0, 60, size=(n, 2)).astype(np.float32) for n in K1]
    matches = [np.where(rng.random(a) < 0.6, rng.integers(0, b, size=a), -1) for a, b in zip(K0, K1)]
    conf = [rng.random(n).astype(np.float32) for n in K0]
    dev = lambda seq: [torch.from_numpy(a).to(gpu) for a in seq]
    assert batch._geo is None
    res = pkg.assemble_matches(batch, torch.from_numpy(scales).to(gpu), dev(kp0), dev(kp1), dev(matches), dev(conf))
    assert batch._geo is None                                        # the records were not read
    got = host(res)
    assert batch.valid == [1, 0, -1, 1]
    off0, off1 = np.concatenate([[0], np.cumsum(K0)]), np.concatenate([[0], np.cumsum(K1)])
    k1_host, k2_host, lengths = [], [], []
    for p in range(4):
        rows0, rows1 = slice(off0[p], off0[p + 1]), slice(off1[p], off1[p + 1])
        if batch.valid[p] < 0:
            assert np.isnan(got['origin0'][rows0]).all() and np.isnan(got['origin1'][rows1]).all()
            assert got['counts'][p].tolist() == [-1] * 4
            lengths.append(0)
            continue
        o0 = batch.to_origin(p, 0, kp0[p], tuple(scales[p, 0]))
        o1 = batch.to_origin(p, 1, kp1[p], tuple(scales[p, 1]))
        assert o0.dtype == np.float64 and mao.equal_bits(got['origin0'][rows0], o0), p
        assert mao.equal_bits(got['origin1'][rows1], o1), p
        valid = matches[p] > -1
        k1_host.append(o0[np.nonzero(valid)[0]].astype(np.float32))
        k2_host.append(o1[matches[p][valid]].astype(np.float32))
        lengths.append(int(valid.sum()))
        lo, hi = got['offsets'][p], got['offsets'][p + 1]
        assert hi - lo == lengths[-1] and mao.equal_bits(got['k1'][lo:hi], k1_host[-1]), p
        assert mao.equal_bits(got['k2'][lo:hi], k2_host[-1]) and mao.equal_bits(got['mconf'][lo:hi], conf[p][valid]), p
    assert got['counts'][:, 2].tolist() == [lengths[0], lengths[1], -1, lengths[3]]
    assert pkg.few_match_pairs(res) == [p for p in range(4) if batch.valid[p] < 0 or lengths[p] < 30] == [2]

    views = mso.make_scene()
    ds = pkg.DepthSet(gpu)
    for v in views:
        ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose'])
    index = [(2, 3), (3, 2), (2, 2), (3, 3)]
    thr = mso.THRESHOLDS
    a = pkg.score_matches(ds, index, res['k1'], res['k2'], offsets=res['offsets'], **thr)
    b = pkg.score_matches(ds, index, torch.from_numpy(np.concatenate(k1_host)).to(gpu),
                          torch.from_numpy(np.concatenate(k2_host)).to(gpu), lengths=lengths, **thr)
    total = sum(lengths)
    assert a['counts'].tolist() == b['counts'].tolist() and a['counts'][:, 0].tolist() == lengths
    assert torch.equal(a['flags'][:total], b['flags']) and not a['flags'][total:].any() and b['flags'].any()
    for k in mso.VALUES:
        assert mso.equal_bits(a[k][:total].cpu().numpy(), b[k].cpu().numpy()), k
        assert torch.isnan(a[k][total:]).all(), k


def test_out_of_range_indices_are_dropped_and_counted(gpu):
    """Only values whose unguarded address would still lie inside ``kp1`` - another pair's rows: a missing guard would
    show as wrong values.  (``INT_MAX`` and int64 values beyond int32 fail the same unsigned compare,
    ``(unsigned)v < (unsigned)K1`` in ``asm_keep``, as huge unsigned numbers; they are not run on the device.)"""
    import imagematching_oetr_amd as pkg
    pairs = ((80, 50, 'dup', 1), (300, 50, 'dup', 1), (64, 120, 'dup', 1))
    call = mao.make_call(7, pairs)
    m = call['matches']
    m[:80] = np.arange(80) % 50                                      # pair 0: in range
    m[80:380] = 50 + np.arange(300) % 100                            # pair 1: every b in [K1, K1 + 100): pair 2's rows
    m[380:] = np.where(np.arange(64) % 2 == 0, np.arange(64), -3)    # pair 2: every other row unmatched
    m[100] = 49                                                       # one good row among the bad
    want = mao.assemble(**call)
    assert want['counts'].tolist() == [[80, 50, 80, 0], [300, 50, 1, 299], [64, 120, 32, 0]]
    for dtype in (np.int32, np.int64):
        res = pkg.assemble_matches(**upload(call, gpu, dtype))
        assert_equal(host(res), want, dtype)
        assert pkg.few_match_pairs(res) == [1]


def test_more_pairs_than_one_chunk_of_the_scan(gpu):
    """1500 tiny pairs: ``k_asm_scan`` walks two chunks of 1024 pairs, so the running bases of ``offsets`` and ``few``
    and both of its LDS buffers are used; pairs with too few matches and pairs without crops lie in both chunks."""
    import imagematching_oetr_amd as pkg
    rng = np.random.default_rng(11)
    pairs = tuple((int(rng.integers(0, 6)), int(rng.integers(1, 5)), ('dup', 'random', 'none')[int(rng.integers(0, 3))],
                   -1 if rng.random() < 0.05 else 1) for _ in range(1500))
    call = mao.make_call(12, pairs)
    want = mao.assemble(**call, min_matches=2)
    few = want['few'][:int(want['n_few'][0])]
    assert (few < 1024).sum() > 100 and (few >= 1024).sum() > 100 and len(few) < 1400
    assert want['offsets'][1024] > 500 and want['offsets'][-1] > want['offsets'][1024] + 200
    res = pkg.assemble_matches(**upload(call, gpu), min_matches=2)
    assert_equal(host(res), want, '1500 pairs')
    assert pkg.few_match_pairs(res) == few.tolist()


def test_out_is_reused_with_fewer_matches_and_nothing_is_allocated(gpu, pinned):
    import imagematching_oetr_amd as pkg
    dev = dict(pinned['dev'])
    out = pkg.assemble_matches(**dev)
    assert_equal(host(out), pinned['want'], 'first')
    fewer = pinned['call']['matches'].copy()
    fewer[::2] = -1
    dev['matches'] = torch.from_numpy(fewer).to(gpu)
    want = mao.assemble(**dict(pinned['call'], matches=fewer))
    assert 0 < want['offsets'][-1] < pinned['want']['offsets'][-1]
    ptrs = {k: out[k].data_ptr() for k in OUTPUTS}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert pkg.assemble_matches(**dev, out=out) is out
    assert torch.cuda.memory_allocated() == before
    assert {k: out[k].data_ptr() for k in OUTPUTS} == ptrs
    assert_equal(host(out), want, 'reused')                          # the tail was rewritten: no row of the first call
    assert_equal(host(out), host(pkg.assemble_matches(**dev)), 'fresh')
    with pytest.raises(ValueError, match='other sizes'):
        pkg.assemble_matches(**dict(dev, conf=None), out=out)


def test_the_joined_form_is_captured_and_replayed_on_new_matches(gpu, pinned):
    import imagematching_oetr_amd as pkg
    dev = dict(pinned['dev'], matches=pinned['dev']['matches'].clone())
    first = host(pkg.assemble_matches(**dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.assemble_matches(**dev)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal(host(captured), first, 'replay')
    changed = np.roll(pinned['call']['matches'], 17)
    changed[::3] = -1
    dev['matches'].copy_(torch.from_numpy(changed))
    graph.replay()
    torch.cuda.synchronize()
    replayed = host(captured)
    eager = host(pkg.assemble_matches(**dev))
    assert_equal(replayed, eager, 'new contents')
    assert_equal(replayed, mao.assemble(**dict(pinned['call'], matches=changed)), 'specification')
    assert not np.array_equal(replayed['index0'], first['index0'])


def test_two_calls_give_equal_bits_and_one_empty_pair_works(gpu, pinned):
    import imagematching_oetr_amd as pkg
    a, b = host(pkg.assemble_matches(**pinned['dev'])), host(pkg.assemble_matches(**pinned['dev']))
    for k in OUTPUTS:                                                # one device: the NaN payloads too
        assert a[k].tobytes() == b[k].tobytes(), k
    call = mao.make_call(3, ((0, 3, 'none', 1),))
    want = mao.assemble(**call)
    assert want['offsets'].tolist() == [0, 0] and want['counts'].tolist() == [[0, 3, 0, 0]] and want['few'].tolist() == [0]
    res = pkg.assemble_matches(**upload(call, gpu))
    assert res['origin0'].shape == (0, 2) and res['k1'].shape == (0, 2) and res['origin1'].shape == (3, 2)
    assert_equal(host(res), want, 'one empty pair')
    assert pkg.few_match_pairs(res) == [0]
    # keypoints that are a view at an odd float (rows off the 8-byte grid the kernel needs) are taken all the same
    flat = torch.empty(2 * len(pinned['call']['kp0']) + 1, device=gpu)
    odd = flat[1:].view(-1, 2)
    odd.copy_(pinned['dev']['kp0'])
    assert odd.data_ptr() % 8 == 4
    assert_equal(host(pkg.assemble_matches(**dict(pinned['dev'], kp0=odd))), a, 'odd view')
    # float16 keypoints are widened: the result of the float32 keypoints of the same values
    dev = pinned['dev']
    h0, h1 = dev['kp0'].half(), dev['kp1'].half()
    assert_equal(host(pkg.assemble_matches(**dict(dev, kp0=h0, kp1=h1))),
                 host(pkg.assemble_matches(**dict(dev, kp0=h0.float(), kp1=h1.float()))), 'float16')
