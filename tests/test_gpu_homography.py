"""GPU tests of the homography extension (``oetr_homography_match_score`` / ``oetr_homography_boxes``,
``csrc/homography.hip``; ``homography.py``; ``evaluate_dummy(gt='homography')``).  There is no tolerance anywhere:
counters, boxes and counts are compared for equality and ``dist_sq`` BIT FOR BIT (``mso.equal_bits``: NaN equals NaN
whatever its payload) with the float64 restatement ``tests/homography_oracle.py``, whose pinned lists and pairs keep
every decision away from last-bit differences (asserted in ``tests/test_homography_cpu.py``).  The fixture is 2033
matches and 56 pairs of pictures of at most 480 x 640."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import homography_oracle as ho  # noqa: E402
import match_assembly_oracle as mao  # noqa: E402
import match_score_oracle as mso  # noqa: E402

pytestmark = pytest.mark.gpu
EXPECTED = json.loads((REPO / 'tests' / 'homography_expected.json').read_text())
COVIS = json.loads((REPO / 'tests' / 'covis_expected.json').read_text())
TEN = len(ho.LENGTHS)                                   # the ten regular lists; the two degenerate ones follow


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items() if k in ('dist_sq', 'counts')}


def assert_lists(got, wants, bounds, tag=None):
    """Every list of a call against its restated result: ``dist_sq`` by bits, the counters."""
    for p, want in enumerate(wants):
        lo, hi = int(bounds[p]), int(bounds[p + 1])
        if 'dist_sq' in got:
            assert mso.equal_bits(got['dist_sq'][lo:hi], want['dist_sq']), (tag, p)
        assert got['counts'][p].tolist() == want['counts'].tolist(), (tag, p, got['counts'][p], want['counts'])


def assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert mso.equal_bits(a[k], b[k]), k


@pytest.fixture(scope='module')
def pinned(gpu):
    """The pinned lists, their restated results and the device inputs: made once, shared, never modified."""
    lists = ho.make_lists(EXPECTED['seed'])
    assert [cvo.sha(np.concatenate([e['k1'], e['k2']])) for e in lists] == EXPECTED['kpts_sha256']
    assert [cvo.sha(e['H']) for e in lists] == EXPECTED['list_H_sha256']    # a wrong input cannot pass as a wrong kernel
    params, k1, k2, lengths = ho.concatenate(lists)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return dict(lists=lists, wants=[ho.score(e['H'], e['k1'], e['k2']) for e in lists], params=t(params), k1=t(k1),
                k2=t(k2), lengths=lengths, bounds=np.concatenate([[0], np.cumsum(lengths)]), host_params=params,
                host_k=(k1, k2))


def test_pinned_lists_equal_the_restatement_and_the_fixture(gpu, pinned):
    import imagematching_oetr_amd as pkg
    n, M = TEN, int(pinned['bounds'][TEN])
    assert pinned['lengths'][:n] == [0, 1, 63, 64, 65, 255, 256, 257, 1000, 0]
    out = pkg.score_matches_homography(pinned['params'][:n], pinned['k1'][:M], pinned['k2'][:M], lengths=pinned['lengths'][:n])
    assert out['dist_sq'].dtype == torch.float64 and out['dist_sq'].shape == (M,) and out['dist_sq'].is_cuda
    assert out['counts'].dtype == torch.int32 and out['counts'].shape == (n, 16) and out['thresholds'] == tuple(range(1, 16))
    got = host(out)
    assert_lists(got, pinned['wants'][:n], pinned['bounds'], 'lengths')
    assert got['counts'].tolist() == [rec['counts'] for rec in EXPECTED['lists'][:n]]
    for p in range(n):
        lo, hi = pinned['bounds'][p], pinned['bounds'][p + 1]
        assert cvo.sha(got['dist_sq'][lo:hi]) == EXPECTED['lists'][p]['dist_sq_sha256'], p
    # all twelve, the degenerate lists included, from host inputs and H alone ([P,3,3])
    H = np.stack([e['H'] for e in pinned['lists']])
    full = host(pkg.score_matches_homography(H, *pinned['host_k'], lengths=pinned['lengths']))
    assert_lists(full, pinned['wants'], pinned['bounds'], 'all twelve')
    assert full['counts'][10].tolist() == [8] + [4] * 15                   # a2 == 0: four rows fail every threshold
    assert not np.isfinite(full['dist_sq'][pinned['bounds'][10]:pinned['bounds'][10] + 4]).any()
    assert full['counts'][11].tolist() == [64] + [0] * 15                  # NaN in H
    assert np.isnan(full['dist_sq'][pinned['bounds'][11]:]).all()
    # values=False: the same counters
    bare = pkg.score_matches_homography(pinned['params'], pinned['k1'], pinned['k2'], lengths=pinned['lengths'], values=False)
    assert 'dist_sq' not in bare and np.array_equal(bare['counts'].cpu().numpy(), full['counts'])
    # keypoints that start on 4 bytes, not 8 (a view at an odd float): taken as they are, the same bits
    odd = lambda k: torch.cat([k.new_zeros(1), k.reshape(-1)])[1:].view(-1, 2)
    o1, o2 = odd(pinned['k1']), odd(pinned['k2'])
    assert o1.data_ptr() % 8 == 4 and o1.is_contiguous() and pinned['k1'].data_ptr() % 8 == 0
    assert_same(host(pkg.score_matches_homography(pinned['params'], o1, o2, lengths=pinned['lengths'])), full)
    assert_same(host(pkg.score_matches_homography(pinned['params'], o1, pinned['k2'], lengths=pinned['lengths'])), full)
    # float16 keypoints are widened exactly
    h1, h2 = pinned['k1'][:M].half(), pinned['k2'][:M].half()
    assert_same(host(pkg.score_matches_homography(pinned['params'][:n], h1, h2, lengths=pinned['lengths'][:n])),
                host(pkg.score_matches_homography(pinned['params'][:n], h1.float(), h2.float(), lengths=pinned['lengths'][:n])))


def test_device_offsets_with_unlisted_rows_before_between_and_after(gpu, pinned):
    """The ten lists through device ``offsets``, with rows that belong to no list BEFORE ``offsets[0]`` and AFTER
    ``offsets[P]``: NaN there, the rows inside and the counters those of the ``lengths`` call.  Under the row -> list
    rule consecutive lists share their boundary, so a stretch BETWEEN two lists cannot be in no list at all: it is
    spelled as the list of an extra pair, here one whose parameter block is NaN throughout - its rows are NaN as
    well and fail every threshold, and its neighbours are unaffected."""
    import imagematching_oetr_amd as pkg
    n = TEN
    k1, k2 = pinned['host_k']
    filler = lambda m: np.full((m, 2), 3.0, np.float32)
    head, tail, between = 70, 67, {3: 5, 6: 300}                          # `between[p]` rows before list p
    params, wants, rows1, rows2, bounds = [], [], [filler(head)], [filler(head)], [head]
    for p in range(n):
        if p in between:
            m = between[p]
            params.append(np.full(16, np.nan))
            wants.append(dict(dist_sq=np.full(m, np.nan), counts=np.array([m] + [0] * 15, np.int32)))
            rows1.append(filler(m)), rows2.append(filler(m))
            bounds.append(bounds[-1] + m)
        lo, hi = pinned['bounds'][p], pinned['bounds'][p + 1]
        params.append(pinned['host_params'][p])
        wants.append(pinned['wants'][p])
        rows1.append(k1[lo:hi]), rows2.append(k2[lo:hi])
        bounds.append(bounds[-1] + int(hi - lo))
    rows1.append(filler(tail)), rows2.append(filler(tail))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    d1, d2, dp = t(np.concatenate(rows1)), t(np.concatenate(rows2)), t(np.stack(params))
    got = host(pkg.score_matches_homography(dp, d1, d2, offsets=t(np.array(bounds, np.int32))))
    assert got['dist_sq'].shape == (bounds[-1] + tail,) and got['counts'].shape == (n + 2, 16)
    assert_lists(got, wants, bounds, 'offsets')
    assert np.isnan(got['dist_sq'][:head]).all() and np.isnan(got['dist_sq'][bounds[-1]:]).all()  # before and after
    finite = int(np.isfinite(np.concatenate([w['dist_sq'] for w in pinned['wants'][:n]])).sum())
    assert int(np.isfinite(got['dist_sq']).sum()) == finite > 1900                                # nothing else is scored
    # offsets that end early: the rows at or after offsets[P] are unscored, the lists before them as they were
    cut = host(pkg.score_matches_homography(dp[:4], d1, d2, offsets=t(np.array(bounds[:5], np.int32))))
    assert np.isnan(cut['dist_sq'][bounds[4]:]).all() and mso.equal_bits(cut['dist_sq'][:bounds[4]], got['dist_sq'][:bounds[4]])
    assert cut['counts'].tolist() == got['counts'][:4].tolist()


def test_thresholds_of_length_0_1_and_16_and_a_nan_threshold(gpu, pinned):
    import imagematching_oetr_amd as pkg
    args = (pinned['params'], pinned['k1'], pinned['k2'])
    for thresholds in ((), (3,), tuple(0.5 * k for k in range(1, 17)), (1.0, float('nan'), 2.0, 15.0)):
        out = pkg.score_matches_homography(*args, lengths=pinned['lengths'], thresholds=thresholds)
        assert out['counts'].shape == (12, 1 + len(thresholds)) and out['thresholds'] == tuple(thresholds)
        wants = [ho.score(e['H'], e['k1'], e['k2'], thresholds) for e in pinned['lists']]
        assert_lists(host(out), wants, pinned['bounds'], thresholds)
    assert (out['counts'][:, 2] == 0).all().item() and (out['counts'][8, 1] > 0).item()           # the NaN threshold
    with pytest.raises(ValueError, match='at most 16'):
        pkg.score_matches_homography(*args, lengths=pinned['lengths'], thresholds=range(17))


def test_empty_calls(gpu, pinned):
    import imagematching_oetr_amd as pkg
    none = torch.zeros(0, 2, device=gpu)
    out = pkg.score_matches_homography(pinned['params'][:3], none, none, lengths=[0, 0, 0])       # n_matches == 0
    assert out['dist_sq'].shape == (0,) and out['counts'].cpu().tolist() == [[0] * 16] * 3
    out = pkg.score_matches_homography(torch.zeros(0, 16, dtype=torch.float64, device=gpu), pinned['k1'][:5],
                                       pinned['k2'][:5], offsets=torch.zeros(1, dtype=torch.int32, device=gpu))   # P == 0
    assert out['counts'].shape == (0, 16) and torch.isnan(out['dist_sq']).all().item()
    with pytest.raises(ValueError, match='summing'):
        pkg.score_matches_homography(pinned['params'][:2], pinned['k1'][:9], pinned['k2'][:9], lengths=[4, 4])


def test_out_is_reused_two_calls_agree_and_a_captured_call_replays_on_new_keypoints(gpu, pinned):
    """Enqueue-only, no host read: captured with default settings; a replay scores what the keypoint tensors hold at
    replay time, under the thresholds of the capture."""
    import imagematching_oetr_amd as pkg
    params, k1, k2 = pinned['params'], pinned['k1'].clone(), pinned['k2'].clone()
    offsets = torch.from_numpy(pinned['bounds'].astype(np.int32)).to(gpu)
    out = pkg.score_matches_homography(params, k1, k2, offsets=offsets)
    first = host(out)
    again = host(pkg.score_matches_homography(params, k1, k2, offsets=offsets))
    assert_same(first, again)                                             # two calls give equal bits
    ptrs = {k: out[k].data_ptr() for k in ('dist_sq', 'counts')}
    out['dist_sq'].fill_(1)
    out['counts'].fill_(1)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    assert pkg.score_matches_homography(params, k1, k2, offsets=offsets, out=out) is out
    assert torch.cuda.memory_allocated(gpu) == before                     # nothing was allocated
    assert {k: out[k].data_ptr() for k in ptrs} == ptrs
    assert_same(host(out), first)
    with pytest.raises(ValueError, match='other sizes'):
        pkg.score_matches_homography(params[:3], k1, k2, offsets=offsets[:4], out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pkg.score_matches_homography(params, k1, k2, offsets=offsets)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(host(captured), first)
    # new keypoints: the lists of another seed under the same homographies
    fresh_lists = [dict(e, **dict(zip(('k1', 'k2'), ho.make_matches(e['H'] if np.isfinite(e['H']).all() else np.eye(3),
                                                                    ho.LIST_SIZES, len(e['k1']), seed=9000 + p))))
                   for p, e in enumerate(pinned['lists'])]
    _, n1, n2, _ = ho.concatenate(fresh_lists)
    assert n1.shape == tuple(k1.shape) and not np.array_equal(n1, pinned['host_k'][0])
    k1.copy_(torch.from_numpy(n1))
    k2.copy_(torch.from_numpy(n2))
    graph.replay()
    torch.cuda.synchronize()
    wants = [ho.score(e['H'], e['k1'], e['k2']) for e in fresh_lists]
    replayed = host(captured)
    assert_lists(replayed, wants, pinned['bounds'], 'replay')
    assert not np.array_equal(replayed['counts'], first['counts'])


# ------------------------------------------------------------------ boxes
@pytest.fixture(scope='module')
def pinned_boxes(gpu):
    boxes = ho.make_boxes(EXPECTED['seed'])
    assert [cvo.sha(b['H']) for b in boxes] == EXPECTED['box_H_sha256']
    params = np.stack([ho.param_block(b['H'], *b['sizes']) for b in boxes])
    return dict(boxes=boxes, host_params=params, params=torch.from_numpy(params).to(gpu))


def box_host(out):
    return {k: out[k].cpu().numpy() for k in ('overlap_box1', 'overlap_box2', 'overlap_valid', 'overlap_count')}


def assert_boxes(got, boxes, rows=None, tag=None):
    for n, b in enumerate(boxes):
        r, at = b['res'], n if rows is None else rows[n]
        where = (tag, b['kind'], b['sizes'])
        assert got['overlap_count'][at] == r['count'], (where, got['overlap_count'][at], r['count'])
        assert bool(got['overlap_valid'][at]) == r['valid'], where
        assert got['overlap_box1'][at].tolist() == r['box1'].tolist(), (where, got['overlap_box1'][at], r['box1'])
        assert got['overlap_box2'][at].tolist() == r['box2'].tolist(), (where, got['overlap_box2'][at], r['box2'])


def test_every_kind_and_size_in_one_call(gpu, pinned_boxes):
    import imagematching_oetr_amd as pkg
    boxes, params = pinned_boxes['boxes'], pinned_boxes['params']
    assert len(boxes) == 8 * 7
    out = pkg.overlap_boxes_from_homography(params, max_size1=(480, 640))
    assert out['overlap_box1'].dtype == torch.float32 and out['overlap_box1'].shape == (56, 4)
    assert out['overlap_valid'].dtype == torch.bool and out['overlap_count'].dtype == torch.int32
    assert out['count'] is out['overlap_count']
    got = box_host(out)
    assert_boxes(got, boxes, tag='one call')
    assert [dict(box1=[int(v) for v in got['overlap_box1'][n]], box2=[int(v) for v in got['overlap_box2'][n]],
                 valid=bool(got['overlap_valid'][n]), count=int(got['overlap_count'][n])) for n in range(56)] == EXPECTED['boxes']
    # the bound read back from the blocks, and H with sizes from the host: the same bits
    for other in (pkg.overlap_boxes_from_homography(params),
                  pkg.overlap_boxes_from_homography(np.stack([b['H'] for b in boxes]),
                                                    size1=np.array([b['sizes'][0] for b in boxes]),
                                                    size2=np.array([b['sizes'][1] for b in boxes]))):
        for k, v in box_host(other).items():
            assert np.array_equal(v, got[k]), k
    # two calls give equal bits; a workspace filled with 0xFF beforehand; out= reused with no allocation
    out['workspace'].fill_(0xFF)
    for k in ('overlap_box1', 'overlap_box2', 'overlap_count'):
        out[k].fill_(7)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    assert pkg.overlap_boxes_from_homography(params, max_size1=(480, 640), out=out) is out
    assert torch.cuda.memory_allocated(gpu) == before
    for k, v in box_host(out).items():
        assert np.array_equal(v, got[k]), k


def test_pairs_that_are_never_evaluated_leave_their_neighbours_alone(gpu, pinned_boxes):
    import imagematching_oetr_amd as pkg
    boxes = [b for b in pinned_boxes['boxes'] if b['sizes'] == ((65, 63), (31, 130))]          # the eight kinds
    params = np.stack([ho.param_block(b['H'], *b['sizes']) for b in boxes] * 2)
    bad = {1: (9, 62.5), 4: (11, 0.0), 6: (10, 66.0), 9: (12, np.nan), 11: (9, 8193.0), 13: (12, -3.0)}
    for row, (at, value) in bad.items():                                  # fractional W1, W2 = 0, H1 > max_h1, ...
        params[row, at] = value
    out = pkg.overlap_boxes_from_homography(torch.from_numpy(params).to(gpu), max_size1=(65, 63))
    got = box_host(out)
    for row in bad:
        assert got['overlap_count'][row] == -1 and not got['overlap_valid'][row], row
        assert not got['overlap_box1'][row].any() and not got['overlap_box2'][row].any(), row
    good = [r for r in range(16) if r not in bad]
    assert_boxes(got, [boxes[r % 8] for r in good], rows=good, tag='neighbours')
    # W1 > max_w1 as well: every pair of a call whose bound is too small for it
    small = box_host(pkg.overlap_boxes_from_homography(torch.from_numpy(params).to(gpu), max_size1=(65, 62)))
    assert (small['overlap_count'] == -1).all() and not small['overlap_valid'].any()


def test_boxes_call_is_captured_and_replayed_on_new_blocks(gpu, pinned_boxes):
    import imagematching_oetr_amd as pkg
    boxes = pinned_boxes['boxes']
    rows = [n for n, b in enumerate(boxes) if b['sizes'][0] == (64, 64)]
    params = pinned_boxes['params'][rows].clone()
    out = pkg.overlap_boxes_from_homography(params, max_size1=(64, 64))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pkg.overlap_boxes_from_homography(params, max_size1=(64, 64), out=out)
    params.copy_(params.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert_boxes(box_host(out), [boxes[n] for n in rows[::-1]], tag='replay')


# ------------------------------------------------------------------ the chain
def test_an_assembled_call_is_scored_through_its_offsets(gpu):
    """``assemble_matches``' ``k1``, ``k2``, ``offsets`` go in as they are: the pinned call of
    ``tests/match_assembly_expected.json``; the rows after the last list (NaN keypoints there) stay unscored."""
    import imagematching_oetr_amd as pkg
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    assembly = json.loads((REPO / 'tests' / 'match_assembly_expected.json').read_text())
    call = mao.make_call(assembly['seed'])
    assert mao.input_hashes(call) == assembly['inputs_sha256']
    want = mao.assemble(**call)
    records = torch.from_numpy(np.ascontiguousarray(call['info']).view(np.uint8).reshape(len(call['info']), -1).copy()).to(gpu)
    res = pkg.assemble_matches(crops=records, scales=t(call['scales']), kp0=t(call['kp0']), kp1=t(call['kp1']),
                               matches=t(call['matches'].astype(np.int32)), conf=t(call['conf']),
                               offsets0=t(call['off0']), offsets1=t(call['off1']))
    P = len(mao.PAIRS)
    Hs = np.stack([ho.make_homography(ho.KINDS[1 + p % 5], ((480, 640), (480, 640)), 40 + p) for p in range(P)])
    out = pkg.score_matches_homography(torch.from_numpy(Hs).to(gpu), res['k1'], res['k2'], offsets=res['offsets'])
    got, bounds = host(out), want['offsets']
    assert bounds.tolist() == assembly['offsets'] and got['dist_sq'].shape[0] > bounds[-1] > 0
    wants = [ho.score(Hs[p], want['k1'][bounds[p]:bounds[p + 1]], want['k2'][bounds[p]:bounds[p + 1]]) for p in range(P)]
    assert_lists(got, wants, bounds, 'assembled')
    assert np.isnan(got['dist_sq'][bounds[-1]:]).all()
    acc = pkg.homography_accuracy(out)
    assert acc['n_matches'].tolist() == np.diff(bounds).tolist()
    assert np.array_equal(acc['accuracy'], np.array([[w['counts'][1 + t] / w['counts'][0] if w['counts'][0] else 0.0
                                                      for t in range(15)] for w in wants]))


class _Stub:
    """A model that predicts prepared boxes, batch after batch, on the device of its one parameter."""

    def __init__(self, pred1, pred2, gpu):
        self.pred1, self.pred2, self.at = pred1.to(gpu), pred2.to(gpu), 0
        self.weight = torch.zeros(1, device=gpu)

    def parameters(self):
        return iter([self.weight])

    def forward_dummy(self, image1, image2):
        n = image1.shape[0]
        assert image1.device == self.weight.device and image1.shape[-1] == 3
        out = self.pred1[self.at:self.at + n], self.pred2[self.at:self.at + n]
        self.at += n
        return out


def test_evaluate_dummy_with_the_ground_truth_as_prediction_gives_recall_one(gpu, pinned_boxes):
    import imagematching_oetr_amd as pkg
    boxes = [b for b in pinned_boxes['boxes'] if b['sizes'] == ((64, 64), (64, 64)) and b['res']['valid']]
    assert len(boxes) >= 6 and all(b['res']['box1'][2] > b['res']['box1'][0] and b['res']['box2'][3] > b['res']['box2'][1]
                                   for b in boxes)
    pred1 = torch.tensor(np.stack([b['res']['box1'] for b in boxes]), dtype=torch.float32)
    pred2 = torch.tensor(np.stack([b['res']['box2'] for b in boxes]), dtype=torch.float32)
    Hs = torch.from_numpy(np.stack([b['H'] for b in boxes]))
    batches, at = [], 0
    for n in (2, len(boxes) - 2):
        batches.append({'image1': torch.zeros(n, 64, 64, 3), 'image2': torch.zeros(n, 64, 64, 3), 'homography': Hs[at:at + n]})
        at += n
    res = pkg.evaluate_dummy(_Stub(pred1, pred2, gpu), batches, gt='homography')
    assert res['recalls'].tolist() == [1.0] * 10 and res['n'] == 2 * len(boxes) and res['n_valid_pairs'] == len(boxes)
    assert res['mean_iou'] == 1.0
    with pytest.raises(KeyError, match='homography'):
        pkg.evaluate_dummy(_Stub(pred1, pred2, gpu), [{k: v for k, v in batches[0].items() if k != 'homography'}], gt='homography')


def table_homography(b1, b2):
    """A homography and picture sizes whose overlap boxes ARE the integer boxes ``b1`` / ``b2`` (x1, y1, x2, y2): a
    flip and a scale per axis, ``u2 = A - (u - x1) * s`` with ``A = a2 + 0.49`` so that ``x1`` lands on ``a2`` and
    ``x1 - 1`` beyond picture 2 (``W2 = a2 + 1``), ``s`` such that ``x2`` lands on ``a1``, and ``W1 = x2 + 1``."""
    rows = []
    for lo, hi, a_lo, a_hi in ((b1[0], b1[2], b2[0], b2[2]), (b1[1], b1[3], b2[1], b2[3])):
        A = a_hi + 0.49
        s = (A - a_lo + 0.25) / (hi - lo)
        rows.append((-s, A + lo * s))
    Hm = np.array([[rows[0][0], 0.0, rows[0][1]], [0.0, rows[1][0], rows[1][1]], [0.0, 0.0, 1.0]])
    return Hm, (int(b1[3]) + 1, int(b1[2]) + 1), (int(b2[3]) + 1, int(b2[2]) + 1)


@pytest.mark.parametrize('oiou', [False, True])
def test_evaluate_dummy_on_the_pinned_recall_table(gpu, oiou):
    """``covis_oracle.recall_table()``'s predictions against ground truth that the NEW entry computes from homographies
    made to have the table's ground-truth boxes: the recalls recorded in ``tests/covis_expected.json``."""
    import imagematching_oetr_amd as pkg
    gt, pred = cvo.recall_table()
    far = np.array([[1.0, 0, 900.0], [0, 1, 0], [0, 0, 1]])               # pairs 5-7: no co-visible pixel
    batches = []
    for p in range(gt.shape[1]):
        if gt[0, p].any():
            Hm, size1, size2 = table_homography(gt[0, p].astype(np.float64), gt[1, p].astype(np.float64))
        else:
            Hm, size1, size2 = far, (48, 64), (48, 64)
        res = ho.overlap_box(Hm, size1[1], size1[0], size2[1], size2[0])
        assert res['box1'].tolist() == gt[0, p].tolist() and res['box2'].tolist() == gt[1, p].tolist(), p
        batches.append({'image1': torch.zeros(1, *size1, 3, device=gpu), 'image2': torch.zeros(1, *size2, 3, device=gpu),
                        'homography': Hm[None]})
    model = _Stub(torch.from_numpy(pred[0]), torch.from_numpy(pred[1]), gpu)
    res = pkg.evaluate_dummy(model, batches, oiou=oiou, gt='homography')
    rec = COVIS['recalls']
    assert np.array_equal(res['recalls'], np.array(rec['oiou_recalls' if oiou else 'iou_recalls'])), res['recalls']
    assert res['n'] == 48 and res['n_valid_pairs'] == 21
