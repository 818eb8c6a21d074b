"""CPU-only checks of the homography specification (``tests/homography_oracle.py``) and of the host
side of ``imagematching_oetr_amd/homography.py``: the recipe regenerates the pinned inputs and the restatement
reproduces ``tests/homography_expected.json`` (written by ``tools/gen_golden_homography.py``, which checked it against
the reference's own ``h_evaluate``); the recorded margins hold; hand-made known answers; ``homography_accuracy``
against a transcription of the reference's accumulation; ``rescale_homography`` against composing by hand;
``evaluate_dummy``'s argument checks."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import imagematching_oetr_amd as pkg

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import covis_oracle as cvo  # noqa: E402
import homography_oracle as ho  # noqa: E402
import match_score_oracle as mso  # noqa: E402

EXPECTED = json.loads((REPO / 'tests' / 'homography_expected.json').read_text())


@pytest.fixture(scope='module')
def lists():
    return ho.make_lists(EXPECTED['seed'])


@pytest.fixture(scope='module')
def boxes():
    return ho.make_boxes(EXPECTED['seed'])


def test_recipe_regenerates_the_pinned_lists_and_the_oracle_reproduces_them(lists):
    assert EXPECTED['thresholds'] == list(ho.THRESHOLDS) == list(range(1, 16))
    assert EXPECTED['list_sizes'] == [list(s) for s in ho.LIST_SIZES]
    assert EXPECTED['list_kinds'] == list(ho.LIST_KINDS) + list(ho.DEGENERATE)
    assert EXPECTED['lengths'] == list(ho.LENGTHS) + [8, 64] == [len(e['k1']) for e in lists]
    assert set(ho.LIST_KINDS) == set(ho.KINDS)                           # every kind scores a list
    margin = np.inf
    for p, (e, rec) in enumerate(zip(lists, EXPECTED['lists'])):
        assert e['k1'].dtype == e['k2'].dtype == np.float32
        assert cvo.sha(e['H']) == EXPECTED['list_H_sha256'][p], (p, e['kind'])
        assert cvo.sha(np.concatenate([e['k1'], e['k2']])) == EXPECTED['kpts_sha256'][p], (p, e['kind'])
        res = ho.score(e['H'], e['k1'], e['k2'])
        assert ho.list_record(res) == rec, (p, e['kind'])
        assert res['counts'][0] == len(e['k1']) and (np.diff(res['counts'][1:]) >= 0).all()
        margin = min(margin, ho.threshold_margin(res['dist_sq']))
    assert margin == EXPECTED['threshold_margin'] >= mso.MIN_THRESHOLD_MARGIN
    # every threshold from 1 to 15 decides something on the long lists
    long = np.array(EXPECTED['lists'][8]['counts'])
    assert (np.diff(long[1:]) > 0).all() and 0 < long[1] and long[15] < long[0]
    # the degenerate lists: non-finite rows fail every threshold
    assert EXPECTED['lists'][10]['counts'] == [8] + [4] * 15 and EXPECTED['lists'][11]['counts'] == [64] + [0] * 15


def test_recipe_regenerates_the_pinned_boxes_and_the_oracle_reproduces_them(boxes):
    assert EXPECTED['box_kinds'] == list(ho.KINDS)
    assert EXPECTED['box_sizes'] == [[list(a), list(b)] for a, b in ho.BOX_SIZES]
    assert len(boxes) == len(ho.KINDS) * len(ho.BOX_SIZES) == len(EXPECTED['boxes'])
    for n, (b, rec) in enumerate(zip(boxes, EXPECTED['boxes'])):
        assert cvo.sha(b['H']) == EXPECTED['box_H_sha256'][n], (b['kind'], b['sizes'])
        assert ho.box_record(b['res']) == rec, (b['kind'], b['sizes'])
    # every kind and size gets through checked_homography within its cap (it raises otherwise), with the margin
    assert min(b['res']['margin'] for b in boxes) == EXPECTED['box_margin'] >= cvo.MIN_MARGIN == 1e-9
    by_kind = {k: [b['res'] for b in boxes if b['kind'] == k] for k in ho.KINDS}
    assert not any(r['valid'] for r in by_kind['disjoint']) and all(r['count'] == 0 for r in by_kind['disjoint'])
    assert all(r['valid'] for r in by_kind['identity'])
    # 'horizon': a2 changes sign inside every picture of more than one pixel, and pixels beyond the line WOULD land
    for b in boxes:
        if b['kind'] == 'horizon' and b['sizes'][0] != (1, 1):
            a2 = b['res']['a2']
            assert (a2 > 0).any() and (a2 < 0).any(), b['sizes']
            assert (b['res']['inside'] & (a2 <= 0)).any(), b['sizes']


def test_the_committed_file_was_checked_against_the_reference():
    assert EXPECTED['reference_checked'] is True
    assert 0 <= EXPECTED['reference_max_abs_diff_px'] <= 1e-9
    assert EXPECTED['reference_rows_compared'] == sum(EXPECTED['lengths']) - 4 - 64    # all but the non-finite rows


def test_known_answers_of_the_score():
    k1 = np.array([[0, 0], [10, 20], [7.5, -3.25], [100, 100]], np.float32)
    res = ho.score(np.eye(3), k1, k1 + np.array([3, 4], np.float32))
    assert res['dist_sq'].tolist() == [25.0] * 4
    assert res['counts'].tolist() == [4] + [0] * 4 + [4] * 11              # steps at thr 5: 25 <= 5 * 5
    empty = ho.score(np.eye(3), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    assert empty['counts'].tolist() == [0] * 16 and empty['dist_sq'].shape == (0,)
    # a2 == 0 exactly: a0 / a2 infinite, 0 / 0 NaN; both fail every threshold
    res = ho.score(ho.A2_ZERO_H, np.array([[2, 0], [2, 1]], np.float32), np.array([[2, 0], [0, 0]], np.float32))
    assert not np.isfinite(res['dist_sq']).any() and res['counts'].tolist() == [2] + [0] * 15
    # a NaN threshold fails its comparison, the others count
    res = ho.score(np.eye(3), k1, k1, thresholds=(1.0, np.nan, 2.0))
    assert res['counts'].tolist() == [4, 4, 0, 4]
    # the operation order: no FMA.  With x = 1 + 2^-23, h00 = 1 + 2^-30, h02 = -1 the exact product ends in 2^-53,
    # half an ulp, which rounding (to even) drops and a fused multiply-add would keep
    x = np.float32(1 + 2.0 ** -23)
    Hm = np.array([[1 + 2.0 ** -30, 0, -1.0], [0, 1, 0], [0, 0, 1]])
    res = ho.score(Hm, np.array([[x, 0]], np.float32), np.zeros((1, 2), np.float32))
    assert res['pu'][0] == 2.0 ** -23 + 2.0 ** -30 != 2.0 ** -23 + 2.0 ** -30 + 2.0 ** -53


def test_known_answers_of_the_boxes():
    for (h1, w1), (h2, w2) in ho.BOX_SIZES:
        res = ho.overlap_box(np.eye(3), w1, h1, w1, h1)
        assert res['count'] == h1 * w1 and res['valid']
        assert res['box1'].tolist() == res['box2'].tolist() == [0, 0, w1 - 1, h1 - 1]
    # a shift by (+2.25, -1.75) from a 5x7 picture (H1 = 5, W1 = 7) into a 7x5 one (H2 = 7, W2 = 5): u2 = u + 2.25
    # lands on i = u + 2, inside for u <= 2; v2 = v - 1.75 lands on j = v - 2, inside for v >= 2: 3 x 3 pixels
    shift = np.array([[1, 0, 2.25], [0, 1, -1.75], [0, 0, 1]])
    res = ho.overlap_box(shift, 7, 5, 5, 7)
    assert res['count'] == 9 and res['box1'].tolist() == [0, 2, 2, 4] and res['box2'].tolist() == [2, 0, 4, 2]
    assert res['margin'] == 0.25
    # half to even: u2 = u + 0.5 lands on the even neighbour (0.5 -> 0, 1.5 -> 2, 2.5 -> 2)
    half = np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1]])
    res = ho.overlap_box(half, 3, 1, 3, 1)
    assert res['count'] == 3 and res['box2'].tolist() == [0, 0, 2, 0] and res['margin'] == 0.0
    res = ho.overlap_box(half, 3, 1, 2, 1)                                 # u = 1, 2 land on 2: outside W2 = 2
    assert res['count'] == 1 and res['box1'].tolist() == [0, 0, 0, 0]
    gone = ho.overlap_box(np.array([[1, 0, 100.0], [0, 1, 0], [0, 0, 1]]), 7, 5, 5, 7)
    assert not gone['valid'] and gone['count'] == 0 and gone['box1'].tolist() == gone['box2'].tolist() == [0] * 4
    assert gone['margin'] == np.inf
    # a horizon by hand: a2 = 1 - u / 2.5 is positive for u = 0, 1, 2 only; a0 = a2 * 1, a1 = a2 * v puts every pixel
    # on (1, v) whatever the side, so exactly the a2 <= 0 columns are lost
    hor = np.array([[-0.4, 0, 1.0], [0, 0, 0], [-0.4, 0, 1.0]])
    res = ho.overlap_box(hor, 6, 4, 4, 4)
    assert res['count'] == 3 * 4 and res['box1'].tolist() == [0, 0, 2, 3] and res['box2'].tolist() == [1, 0, 1, 0]
    assert int((res['a2'] <= 0).sum()) == 3 * 4 and res['inside'].all()
    # NaN in H: nothing is kept
    bad = np.eye(3)
    bad[2, 2] = np.nan
    assert ho.overlap_box(bad, 4, 4, 4, 4)['count'] == 0


def test_homography_accuracy_is_the_reference_accumulation():
    counts = np.array([rec['counts'] for rec in EXPECTED['lists']], np.int32)
    names = ['i_ajuntament', 'v_abstract', 'v_bird', 'i_crownday', 'v_graffiti', 'i_fog', 'v_wall', 'i_ski',
             'v_yard', 'i_empty', 'v_degenerate', 'x_counts_as_viewpoint']
    res = pkg.homography_accuracy({'counts': torch.from_numpy(counts), 'thresholds': tuple(range(1, 16))}, seq_type=names)
    i_err, v_err = ho.reference_accumulation(counts.tolist(), names)
    assert res['i_err'] == i_err and res['v_err'] == v_err and list(res['i_err']) == list(range(1, 16))
    want = np.array([[c[1 + t] / c[0] if c[0] else 0.0 for t in range(15)] for c in counts.tolist()])
    assert np.array_equal(res['accuracy'], want) and res['accuracy'].shape == (12, 15)
    assert (res['accuracy'][[0, 9]] == 0).all()                            # the empty lists
    total = np.zeros(15)
    for row in want:
        total = total + row
    assert np.array_equal(res['sum'], total)
    assert res['n_matches'].tolist() == EXPECTED['lengths'] and res['thresholds'] == tuple(range(1, 16))
    # a bare array, no sequence types
    bare = pkg.homography_accuracy(counts)
    assert np.array_equal(bare['accuracy'], want) and 'i_err' not in bare and bare['thresholds'] == tuple(range(1, 16))
    none = pkg.homography_accuracy(np.zeros((0, 16), np.int32), seq_type=[])
    assert none['sum'].tolist() == [0.0] * 15 and none['i_err'][1] == 0.0
    with pytest.raises(ValueError):
        pkg.homography_accuracy(counts, seq_type=names[:3])


def test_rescale_homography_against_composing_by_hand():
    rng = np.random.default_rng(3)
    H = ho.make_homography('perspective', ((480, 640), (600, 800)), 1)
    s1, s2 = np.array([1.25, 1.5]), np.array([0.8, 2.0])                  # original / resized, (sx, sy)
    got = pkg.rescale_homography(H, s1, s2)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (3, 3)
    by_hand = np.array([[H[r, c] * (s1[c] if c < 2 else 1.0) / (s2[r] if r < 2 else 1.0) for c in range(3)]
                        for r in range(3)])
    assert np.array_equal(got, by_hand)
    assert np.allclose(got, np.diag([1 / s2[0], 1 / s2[1], 1]) @ H @ np.diag([s1[0], s1[1], 1]), rtol=1e-14, atol=0)
    # the property: a point p of resized image 1 is p * s1 in the original; its image under H, over s2, is got(p)
    p = rng.uniform(0, 400, (50, 2))
    a = ho.apply(H, p[:, 0] * s1[0], p[:, 1] * s1[1])
    b = ho.apply(got, p[:, 0], p[:, 1])
    assert np.allclose(a[0] / a[2] / s2[0], b[0] / b[2], rtol=1e-12) and np.allclose(a[1] / a[2] / s2[1], b[1] / b[2], rtol=1e-12)
    # batched, per-pair scales, and a tensor in gives a tensor out
    Hs = np.stack([H, np.eye(3)])
    both = pkg.rescale_homography(torch.from_numpy(Hs), torch.tensor([[1.25, 1.5], [2.0, 2.0]]), (0.8, 2.0))
    assert torch.is_tensor(both) and both.dtype == torch.float64 and both.shape == (2, 3, 3)
    assert np.array_equal(both[0].numpy(), got)
    assert both[1].tolist() == [[2.5, 0, 0], [0, 1, 0], [0, 0, 1]]


class _Stub:
    def forward_dummy(self, image1, image2):
        n = image1.shape[0]
        return torch.zeros(n, 4), torch.zeros(n, 4)


def test_evaluate_dummy_homography_argument_checks():
    batch = {'image1': torch.rand(2, 8, 8, 3), 'image2': torch.rand(2, 8, 8, 3)}
    with pytest.raises(KeyError, match='homography'):
        pkg.evaluate_dummy(_Stub(), [batch], gt='homography')
    with pytest.raises(ValueError, match='gt must be'):
        pkg.evaluate_dummy(_Stub(), [batch], gt='planar')
    assert pkg.evaluate_dummy(_Stub(), [], gt='homography')['n'] == 0
