"""CPU: the box -> crop oracle (``oracle/crop_oracle.py``) against
``tests/golden/crop.npz`` - produced by the reference's own ``Matching.forward`` overlap
branch, ``tensor_overlap_crop`` and ``patch_resize`` (``oracle/gen_golden.py::gen_crop``).
Gate, scaled boxes, ratios and output shapes are the reference's arithmetic and must match
exactly; the crop pixels match bit for bit because the golden run used this oracle's
bicubic in place of the absent ``cv2.resize`` (OpenCV's own numerics stay unpinned)."""
import numpy as np
import pytest
import torch

from oracle import crop_oracle as cro
from oracle import oetr_oracle as orc


def load_cases(golden_dir):
    g = np.load(golden_dir / 'crop.npz')
    for ci in range(int(g['n_cases'])):
        t = f'c{ci}_'
        gen = torch.Generator().manual_seed(int(g[t + 'seed']))
        ch = int(g[t + 'channels'])
        im0 = torch.rand(1, ch, *(int(v) for v in g[t + 'hw0']), generator=gen)
        im1 = torch.rand(1, ch, *(int(v) for v in g[t + 'hw1']), generator=gen)
        assert orc.checksum(im0) == list(g[t + 'in_fp'][0]) and orc.checksum(im1) == list(g[t + 'in_fp'][1])
        yield ci, {k[len(t):]: g[k] for k in g.files if k.startswith(t)}, im0, im1


def test_oracle_reproduces_the_reference_crop_step(golden_dir):
    n = 0
    for ci, c, im0, im1 in load_cases(golden_dir):
        out = cro.overlap_crop(im0, im1, torch.from_numpy(c['box0']), torch.from_numpy(c['box1']),
                               tuple(c['scales0']), tuple(c['scales1']),
                               keep_aspect=bool(c['keep_aspect']), size_divisor=int(c['size_divisor']),
                               pragueparks=bool(c['pragueparks']))
        assert out['valid'] == bool(c['valid']), ci
        assert np.array_equal(out['bbox0'].numpy().astype(np.float32), c['bbox0']), ci
        assert np.array_equal(out['bbox1'].numpy().astype(np.float32), c['bbox1']), ci
        assert np.array_equal(np.float32(out['ratio0']).astype(np.float64), c['ratio0']), ci
        assert np.array_equal(np.float32(out['ratio1']).astype(np.float64), c['ratio1']), ci
        assert tuple(out['crop0'].shape) == tuple(c['out_shape0']), ci
        assert tuple(out['crop1'].shape) == tuple(c['out_shape1']), ci
        assert orc.checksum(out['crop0']) == list(c['out_fp'][0]), ci
        assert orc.checksum(out['crop1']) == list(c['out_fp'][1]), ci
        if 'crop0' in c:
            assert np.array_equal(out['crop0'].numpy(), c['crop0'])
        n += 1
    assert n == 8


def test_bicubic_properties():
    """Size-independent properties of the restated OpenCV bicubic: identity at equal
    size, exact on constants, weights sum to 1, monotone on ramps, replicate border."""
    g = np.random.default_rng(0)
    img = g.random((13, 17, 3), dtype=np.float32)
    assert np.array_equal(cro.bicubic_resize(img, 17, 13), img)
    const = np.full((9, 11), 3.25, dtype=np.float32)
    assert np.allclose(cro.bicubic_resize(const, 23, 31), 3.25, atol=1e-6)
    for t in (0.0, 0.25, 0.5, 0.999):
        assert abs(float(cro.cubic_weights(t).sum()) - 1.0) < 1e-6
    # (a = -0.75 is not Catmull-Rom: linear ramps are reproduced only approximately)
    ramp = np.tile(np.arange(32, dtype=np.float32), (4, 1))
    up = cro.bicubic_resize(ramp, 64, 4)
    x = (np.arange(64) + 0.5) * 0.5 - 0.5
    assert np.abs(up[0, 4:-4] - x[4:-4]).max() < 0.1 and np.all(np.diff(up[0]) >= -1e-6)
    assert up[0, 0] == ramp[0, 0] or abs(up[0, 0] - ramp[0, 0]) < 0.2     # replicate border
    assert cro.bicubic_resize(img, 5, 4).shape == (4, 5, 3)


def test_gate_and_geometry_edge_cases():
    b = torch.tensor([10.0, 10.0, 50.0, 50.0])
    assert cro.scale_and_gate(b, b, (1, 1), (1, 1))[2] is True
    assert cro.scale_and_gate(torch.tensor([10.0, 10.0, 11.9, 50.0]), b, (1, 1), (1, 1))[2] is False
    assert cro.scale_and_gate(b, torch.tensor([10.0, 10.0, 10.0, 50.0]), (1, 1), (1, 1))[2] is False   # zero width
    assert cro.scale_and_gate(b, b, (1, 1), (1, 1), pragueparks=True)[2] is False       # ratio 1
    big = torch.tensor([0.0, 0.0, 130.0, 40.0])
    assert cro.scale_and_gate(big, b, (1, 1), (1, 1), pragueparks=True)[2] is True      # 130 // 40 = 3
    geo = cro.crop_geometry((100, 100), (50, 50), torch.tensor([90.0, 90.0, 120.0, 130.0]),
                            torch.tensor([0.0, 0.0, 50.0, 50.0]), True, 8)
    assert geo[0]['crop'] == (10, 10) and geo[0]['box'] == (90, 90, 120, 130)
    assert geo[0]['new'] == (100, 100) and geo[0]['out'] == (104, 104)
    assert geo[1]['ratio'] == (2.0, 2.0) and geo[1]['out'] == (104, 104)


# ---- the box domain (oracle/crop_oracle.py::in_domain) ----------------------------------------------------
# A literal table: written by hand from the rule and from patch_resize's arithmetic, not taken from the oracle.
# Images: 48 x 56 and 41 x 47 (h x w), keep_aspect, size_divisor 1, the plain gate; the larger image gives the
# target size (56 x 48).  Image 1's box is BOX1 with unit scales unless a row says otherwise: ints (3, 4, 40, 35),
# slice 37 x 31, 56 / 37 < 48 / 31 so the width is kept: new = (56, int(56 / 37 * 31) = 46).
NAN, INF = float('nan'), float('inf')
DOMAIN_HW = ((48, 56), (41, 47))
BOX1 = (3.0, 4.0, 40.0, 35.0)
SIDE1 = dict(box=(3, 4, 40, 35), crop=(37, 31), new=(56, 46))


def _row(name, box0, valid, side0=None, sc0=(1.0, 1.0), box1=BOX1, sc1=(1.0, 1.0)):
    return dict(name=name, box0=box0, box1=box1, sc0=sc0, sc1=sc1, valid=valid, side0=side0)


DOMAIN_TABLE = [
    # inside: slice 45 x 34, 56 / 45 < 48 / 34 -> new = (56, int(56 / 45 * 34) = 42)
    _row('base', (5.0, 6.0, 50.0, 40.0), 1, dict(box=(5, 6, 50, 40), crop=(45, 34), new=(56, 42))),
    # each of the four coordinates of image 0 alone at -5, and one of image 1
    _row('x1=-5', (-5.0, 6.0, 50.0, 40.0), -1),
    _row('y1=-5', (5.0, -5.0, 50.0, 40.0), -1),
    _row('x2=-5', (5.0, 6.0, -5.0, 40.0), -1),
    _row('y2=-5', (5.0, 6.0, 50.0, -5.0), -1),
    _row('image 1 y1=-5', (5.0, 6.0, 50.0, 40.0), -1, box1=(3.0, -5.0, 40.0, 35.0)),
    # the lower edge of the rule: -1.0 truncates to -1 (outside), -0.999 to 0 (inside: slice 50 x 34, new_h = int(1.12 * 34) = 38)
    _row('x1=-1.0', (-1.0, 6.0, 50.0, 40.0), -1),
    _row('y1=-1.0', (5.0, -1.0, 50.0, 40.0), -1),
    _row('x1=-0.999', (-0.999, 6.0, 50.0, 40.0), 1, dict(box=(0, 6, 50, 40), crop=(50, 34), new=(56, 38))),
    # the upper edge: the largest float32 below 2^31 is inside (the stop is clamped at the far edge: slice 51 x 34,
    # new_h = int(56 / 51 * 34) = 37); 2^31 itself and beyond are outside
    _row('x2=2147483520', (5.0, 6.0, 2147483520.0, 40.0), 1, dict(box=(5, 6, 2147483520, 40), crop=(51, 34), new=(56, 37))),
    _row('x2=2^31', (5.0, 6.0, 2147483648.0, 40.0), -1),
    _row('x2=3e9', (5.0, 6.0, 3e9, 40.0), -1),
    _row('x1=-3e9', (-3e9, 6.0, 50.0, 40.0), -1),
    _row('y2=nan', (5.0, 6.0, 50.0, NAN), -1),
    _row('x1=nan', (NAN, 6.0, 50.0, 40.0), -1),
    _row('x2=+inf', (5.0, 6.0, INF, 40.0), -1),
    _row('y1=-inf', (5.0, -INF, 50.0, 40.0), -1),
    _row('image 1 x2=+inf', (5.0, 6.0, 50.0, 40.0), -1, box1=(3.0, 4.0, INF, 35.0)),
    # negative only through the scale: -0.6 * 1.6 = -0.96 -> 0 (inside; 30 * 1.6 = 48 in float32: slice 48 x 34,
    # new_h = int(56 / 48 * 34) = 39); -0.6 * 2.0 = -1.2 (outside)
    _row('scale 1.6', (-0.6, 6.0, 30.0, 40.0), 1, dict(box=(0, 6, 48, 40), crop=(48, 34), new=(56, 39)), sc0=(1.6, 1.0)),
    _row('scale 2.0', (-0.6, 6.0, 30.0, 40.0), -1, sc0=(2.0, 1.0)),
    _row('scale 2.0 to -8', (-4.0, -4.0, 25.0, 20.0), -1, sc0=(2.0, 2.0)),
    # a negative coordinate that would also have failed the gate (half a pixel wide): -1, not 0
    _row('negative and thin', (-5.0, 6.0, -4.5, 40.0), -1),
    # inside the domain, as before: an inverted box fails the gate (pass-through); a box wholly past the far edge
    # passes it and leaves an empty slice (-1); a stop alone past the far edge is clamped (slice 51 x 34)
    _row('inverted', (50.0, 6.0, 5.0, 40.0), 0),
    _row('past the far edge', (60.0, 6.0, 90.0, 40.0), -1, dict(box=(60, 6, 90, 40), crop=(0, 34), new=(0, 0))),
    _row('stop past the far edge', (5.0, 6.0, 70.0, 40.0), 1, dict(box=(5, 6, 70, 40), crop=(51, 34), new=(56, 37))),
]


def domain_row_boxes(row):
    return torch.tensor(row['box0'], dtype=torch.float32), torch.tensor(row['box1'], dtype=torch.float32)


def test_box_domain_table():
    names = [r['name'] for r in DOMAIN_TABLE]
    assert len(set(names)) == len(names)
    im0, im1 = torch.rand(1, 1, *DOMAIN_HW[0]), torch.rand(1, 1, *DOMAIN_HW[1])
    for row in DOMAIN_TABLE:
        b0, b1 = domain_row_boxes(row)
        rec = cro.crop_record(*DOMAIN_HW, b0, b1, row['sc0'], row['sc1'], True, 1, False)
        assert rec['valid'] == row['valid'], (row['name'], rec)
        out = cro.overlap_crop(im0, im1, b0, b1, row['sc0'], row['sc1'], True, 1, False)
        assert out['valid'] == row['valid'] and type(out['valid']) is (int if row['valid'] < 0 else bool), row['name']
        if row['valid'] < 0:
            assert out['crop0'] is None and out['crop1'] is None, row['name']
            assert rec['new_w'] == rec['new_h'] == rec['out_w'] == rec['out_h'] == [0, 0], row['name']
        if row['valid'] == 0:
            assert rec['box'] == [[0, 0, 56, 48], [0, 0, 47, 41]] and rec['crop_w'] == rec['out_w'] == [56, 47], row['name']
            assert rec['crop_h'] == rec['out_h'] == [48, 41] and rec['ratio'] == [[1.0, 1.0]] * 2, row['name']
            assert out['crop0'] is im0 and out['crop1'] is im1
        if row['side0'] is not None:         # the integer fields of a record inside the domain
            new1 = SIDE1['new'] if row['valid'] == 1 else (0, 0)       # one empty side zeroes the sizes of both
            for i, want in ((0, row['side0']), (1, dict(SIDE1, new=new1))):
                got = dict(box=tuple(rec['box'][i]), crop=(rec['crop_w'][i], rec['crop_h'][i]), new=(rec['new_w'][i], rec['new_h'][i]))
                assert got == want, (row['name'], i, got)
                assert (rec['out_w'][i], rec['out_h'][i]) == want['new'], (row['name'], i)
        if row['valid'] == 1:
            assert tuple(out['crop0'].shape) == (1, 1, rec['out_h'][0], rec['out_w'][0]), row['name']
        if row['valid'] == -1 and row['side0'] is None:      # outside the domain: all integers and ratios zero, sbox as scaled
            assert rec['box'] == [[0] * 4] * 2 and rec['crop_w'] == rec['crop_h'] == [0, 0] and rec['ratio'] == [[0.0, 0.0]] * 2
            sb = cro.scale_boxes(b0, b1, row['sc0'], row['sc1'])
            assert np.array_equal(np.float32(rec['sbox']), torch.stack(sb).numpy(), equal_nan=True), row['name']
    assert {r['valid'] for r in DOMAIN_TABLE} == {1, 0, -1}


def test_in_domain_slice_and_size_come_from_one_rectangle():
    """Independent of the oracle's own clamping: for random NON-NEGATIVE integer boxes - starts and stops past
    the far edge, inverted and empty ones included - the size the oracle reports is the shape of Python's
    ``img[0, :, y1:y2, x1:x2]`` and the patch it resizes is that slice."""
    rng = np.random.default_rng(21)
    img = torch.rand(1, 2, 23, 31, generator=torch.Generator().manual_seed(21))
    other = (19, 40)
    n_past = n_empty = 0
    for _ in range(400):
        x1, x2 = (int(v) for v in rng.integers(0, 45, size=2))
        y1, y2 = (int(v) for v in rng.integers(0, 35, size=2))
        sb = torch.tensor([x1, y1, x2, y2], dtype=torch.float32)
        g = cro.crop_geometry(tuple(img.shape[2:]), other, sb, torch.tensor([1.0, 2.0, 30.0, 15.0]), True, 1)[0]
        want = img[0, :, y1:y2, x1:x2]
        assert g['box'] == (x1, y1, x2, y2)
        assert g['crop'] == (want.shape[2], want.shape[1]), (x1, y1, x2, y2, g)
        patch = cro.crop_patch(img, g['rect'])
        assert patch.shape == (want.shape[1], want.shape[2], 2)
        assert np.array_equal(patch, want.permute(1, 2, 0).numpy() * 255)
        n_past += x1 > 31 or y1 > 23 or x2 > 31 or y2 > 23
        n_empty += want.numel() == 0
    assert n_past > 100 and 50 < n_empty < 350


def test_fuzz_cases_are_unchanged_by_the_domain_rule():
    """``tests/crop_fuzz_expected.json`` holds what ``overlap_crop`` of the oracle gave for the 60 fuzz cases
    (``tests/test_gpu_crop_batch.py::fuzz_cases``) BEFORE the box domain was stated: gate, scaled boxes, ratios,
    shapes and pixel checksums.  (The oracle's own record, not the reference's output: it lies beside the other
    expected-result files, not among the regenerated fixtures of ``tests/golden/``.)  Every case lies inside the
    domain, and the oracle still gives exactly that."""
    import json
    from pathlib import Path
    from tests.test_gpu_crop_batch import fuzz_cases, image
    want = json.loads((Path(__file__).resolve().parent / 'crop_fuzz_expected.json').read_text())['cases']
    cases = fuzz_cases()
    assert len(want) == len(cases) == 60
    for ci, (c, w) in enumerate(zip(cases, want)):
        keep, div, pp = c['mode']
        assert cro.in_domain(*cro.scale_boxes(c['b0'], c['b1'], c['sc0'], c['sc1'])), ci
        ref = cro.overlap_crop(image(c['hw0']), image(c['hw1']), c['b0'], c['b1'], c['sc0'], c['sc1'], keep, div, pp)
        assert ref['valid'] is bool(w['valid']), ci
        for i, s in enumerate('01'):
            assert [float(v) for v in ref['bbox' + s].reshape(-1)] == w['bbox'][i], (ci, i)
            assert [float(v) for v in ref['ratio' + s]] == w['ratio'][i], (ci, i)
            assert list(ref['crop' + s].shape) == w['shape'][i] and orc.checksum(ref['crop' + s]) == w['checksum'][i], (ci, i)
    assert 0 < sum(w['valid'] for w in want) < 60


def test_bicubic_agrees_with_an_independent_implementation():
    """cv2 is not installed, so OpenCV's own output cannot pin :func:`bicubic_resize`; what
    can be checked is that the restatement agrees with an INDEPENDENT implementation of the
    same published algorithm - torch's ``F.interpolate(mode='bicubic',
    align_corners=False)``: cubic convolution with a = -0.75, pixel centres
    ``(d + 0.5) * scale - 0.5``, taps clamped to the border, no antialiasing.  The two
    differ only in fp32 rounding (torch evaluates all four tap polynomials, OpenCV gets the
    fourth as 1 - the others; separable passes in the other order): observed <= 7e-4 on
    the 0..255 scale the reference resizes on (3e-6 relative), up- and down-scaling."""
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    for h, w, nh, nw in ((13, 17, 31, 23), (40, 50, 20, 25), (33, 21, 64, 64), (64, 48, 17, 5), (7, 9, 7, 30)):
        img = (rng.random((h, w, 3)) * 255).astype(np.float32)
        ours = cro.bicubic_resize(img, nw, nh)
        ref = F.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None], size=(nh, nw), mode='bicubic',
                            align_corners=False)[0].permute(1, 2, 0).numpy()
        assert np.abs(ours - ref).max() <= 2e-3, (h, w, nh, nw, np.abs(ours - ref).max())
