"""forward_dummy's masks in every kernel form, against the oracle in fp64 (and fp32).

The masks select kernels of their own: the MASKED instantiations of the encoder (the exact-fp32 32-row
kernel, the 64-row and 32-row two-plane kernels), the decoder preparation of the last encoder launch,
the -1e9 fill of the heat-map logits (both tail forms), the `*_masked` seams.  Here every one of them runs
on mask patterns that line up with the kernels' tiling (oracle.make_mask_pattern: a whole 32- / 64-row
tile cleared, a lone token in the ragged last tile, one valid token per image, a side masked entirely,
fractional weights incl. 1.5 and 1e-6) on grids just below and above 32 and 64 tokens, under every
run-time form: precision x tile, tail form, decoder split, state pre-reduction.

The high-precision reference is orc.hot_path in float64; a stage passes when it is within TOL of the
fp32 oracle AND within max(FP32_CLASS x |torch fp32 - fp64|, floor) of fp64 (test_split_mode_is_fp32_class's
rule).  Forms of the same arithmetic are compared with each other as in test_gpu_parity.py.
Run with `-m gpu` on an MI355X."""
import itertools

import pytest
import torch

from oracle import oetr_oracle as orc
from tests.test_gpu_parity import FORM_TOL, FP32_CLASS, TOL, _write_margins, check_stages, margin, maxerr  # noqa: F401
from tests.test_gpu_precision import POLICY_TOL

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

W_SEED = 3
SIDES = ('1', '2')
# test_split_mode_is_fp32_class's floors (where torch's own fp32 drift is tiny)
FLOOR = dict(memory=2e-5, hs=1e-5, logits=2e-4, cxy=2e-3)

# id, pairs, grid 1, grid 2, patterns 1, patterns 2 (make_mask_pattern: per image, the last one repeats)
CASES = [
    ('1x1', 1, (1, 1), (1, 1), 'full', 'zero'),
    ('1x31_1x33', 2, (1, 31), (1, 33), 'last|weighted', 'tile32:1|first'),
    ('4x8_8x8', 2, (4, 8), (8, 8), 'tile32:0|one', 'weighted|tile64:0'),
    ('7x9_5x13', 3, (7, 9), (5, 13), 'weighted|tile32:1|last', 'one|first|tile64:1'),
    ('3x11_1x97', 2, (3, 11), (1, 97), 'empty', 'tile32:2|last'),
    ('20x20_40x40', 2, (20, 20), (40, 40), 'tile64:3|first', 'last|tile64:10'),
]
LARGE = [
    ('100x100_2x2', 1, (100, 100), (2, 2), 'weighted', 'last'),
    ('8x32x32', 8, (32, 32), (32, 32), 'weighted|tile64:5|one|tile32:7|first|last|full|zero',
     'tile32:3|weighted|last|one|zero|tile64:15|first|tile64:0'),
]
PRECISIONS = ['f32_split_f16@32', 'f32_split_f16@64', 'f32_split_qk16@32', 'f32_split_qk16@64', 'f32']
TAILS, SPLITS, PRERED = (0, 1, 2, 3), (0, 1, 4), (-1, 0, 1)


def _valid(combo):
    return not (combo[0] == 'f32' and combo[1] >= 2)


def covering_subset():
    """Settings (precision, tail, split, pre-reduction) in which every pair of values of two settings
    appears at least once (greedy, deterministic)."""
    combos = [c for c in itertools.product(PRECISIONS, TAILS, SPLITS, PRERED) if _valid(c)]
    pairs = lambda c: {(i, c[i], j, c[j]) for i, j in itertools.combinations(range(4), 2)}
    todo = set().union(*(pairs(c) for c in combos))
    rows = []
    while todo:
        best = max(combos, key=lambda c: len(pairs(c) & todo))
        rows.append(best)
        todo -= pairs(best)
    return rows


class Case:
    """Inputs, masks and the fp32 / fp64 oracle of one case (computed once)."""

    def __init__(self, cid, n, g1, g2, k1, k2, seed):
        self.id, self.n, self.g = cid, n, {'1': g1, '2': g2}
        self.w = orc.make_hot_weights(W_SEED, sharpen=True)
        self.f1, self.f2 = orc.make_features(500 + seed, n, *g1), orc.make_features(600 + seed, n, *g2)
        self.p1, self.p2 = orc.position_table(*g1), orc.position_table(*g2)
        self.m = {'1': orc.make_masks(700 + seed, n, *g1, kind=k1), '2': orc.make_masks(800 + seed, n, *g2, kind=k2)}
        self.img = {s: (self.g[s][0] * 32, self.g[s][1] * 32) for s in SIDES}
        self.ref = orc.hot_path(self.f1, self.f2, self.w, self.img['1'], self.img['2'], return_stages=True,
                                mask1=self.m['1'], mask2=self.m['2'])
        self.r64 = orc.hot_path(self.f1.double(), self.f2.double(), orc.cast_weights(self.w, torch.float64),
                                self.img['1'], self.img['2'], return_stages=True, mask1=self.m['1'], mask2=self.m['2'])
        self.drift = {k + s: float((self.ref[k + s].double() - self.r64[k + s]).abs().max())
                      for k in FLOOR for s in SIDES}

    def dev(self, gpu):
        return [t.to(gpu) for t in (self.f1, self.f2, self.p1, self.p2)]

    def forward(self, eng, gpu, **kw):
        return eng.forward(*self.dev(gpu), self.img['1'], self.img['2'], mask1=self.m['1'], mask2=self.m['2'], **kw)


@pytest.fixture(scope='module')
def cases():
    return {spec[0]: Case(*spec, seed=i) for i, spec in enumerate(CASES + LARGE)}


@pytest.fixture(scope='module')
def engines(gpu):
    from imagematching_oetr_amd import HotPathEngine
    cache = {}

    def get(precision):
        if precision not in cache:
            prec, _, tile = precision.partition('@')
            cache[precision] = HotPathEngine(orc.make_hot_weights(W_SEED, sharpen=True), device=gpu, precision=prec,
                                             enc_tile=int(tile) if tile else None)
        return cache[precision]
    return get


def fp64_rule(got, c, key, note, precision):
    """|HIP - fp64| <= max(FP32_CLASS x |torch fp32 - fp64|, floor); the observed ratio goes to the margins."""
    ref = c.r64[key]
    err = float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max())
    drift = c.drift[key]
    margin('masked_' + c.id, precision, 'err / torch-fp32-drift (ratio)', key, err / max(drift, 1e-12))
    margin('masked_' + c.id, precision, 'vs fp64 oracle', key, err)
    assert err <= max(FP32_CLASS * drift, FLOOR[key[:-1]]), f'{note} {key}: {err:.3e} vs fp64 (torch fp32 {drift:.3e})'


def check_special_images(got_cxy, c, s, note):
    """One valid token: the soft-argmax is that token's centre (every other weight is exp(-1e9 - max) = 0).
    No valid token: the uniform softmax, i.e. the centre of the grid."""
    hf, wf = c.g[s]
    stride = c.img[s][0] // hf
    m = c.m[s].flatten(1)
    for i in range(c.n):
        nz = torch.nonzero(m[i]).flatten()
        if nz.numel() == 1:
            y, x = divmod(int(nz[0]), wf)
            want = torch.tensor([(x + 0.5) * stride, (y + 0.5) * stride], dtype=torch.float64)
        elif nz.numel() == 0:
            want = torch.tensor([wf * stride / 2.0, hf * stride / 2.0], dtype=torch.float64)
        else:
            continue
        assert maxerr(c.r64['cxy' + s][i], want) <= 1e-9
        assert maxerr(got_cxy[i], want) <= 1e-3, f'{note} side {s} image {i}: cxy {got_cxy[i].tolist()} want {want.tolist()}'


def check_call(out, c, precision, note, eng):
    assert eng.query_flags() == 0, note
    for s in SIDES:
        dead = (c.m[s].flatten(1) == 0).to(out['logits' + s].device)
        assert (out['logits' + s][dead] == orc.MASK_FILL).all(), f'{note}: masked logits must hold -1e9'
        assert (out['logits' + s][~dead] > -1e8).all(), f'{note}: an unmasked logit was filled'
        check_special_images(out['cxy' + s], c, s, note)
    base = precision.partition('@')[0]
    if base == 'f32_split_qk16':
        for s in SIDES:
            for key, t in POLICY_TOL.items():
                e = margin('masked_' + c.id, precision, 'vs oracle', key + s, maxerr(out[key + s], c.ref[key + s]))
                assert e <= t, f'{note} {key}{s}: {e:.3e} > {t}'
            b_ref = c.ref['box' + s]
            area = (b_ref[:, 2] - b_ref[:, 0]) * (b_ref[:, 3] - b_ref[:, 1])
            iou = orc.bbox_iou_aligned(out['box' + s].cpu(), b_ref)
            assert (iou[area > 1] >= 1 - 1e-3).all(), f'{note} IoU {iou}'
        return
    check_stages(out, c.ref, note, 'masked_' + c.id, precision)
    for key in FLOOR:
        for s in SIDES:
            fp64_rule(out[key + s], c, key + s, note, precision)


def unmasked_logits_scale(out, c, s):
    live = (c.m[s].flatten(1) != 0).to(out['logits' + s].device)
    return 1.0 + (float(out['logits' + s][live].abs().max()) if live.any() else 0.0)


def check_forms(outs, c, precision):
    """Forms of the same arithmetic at one precision and tile: pre-reduction changes no bit; tail forms
    1 / 2 / 3 share the decoder at a fixed split (hs bit for bit) and differ in the conv's summation order;
    decoder split 1 against 4 to fp32 summation order.  (The automatic split, 0, depends on the tail form -
    beside the conv-P GEMMs or as a launch of its own, api.hip - so there tail forms agree to FORM_TOL.)"""
    keys = ('memory1', 'memory2', 'hs1', 'hs2', 'box1', 'box2')
    for (t, k, p), o in outs.items():
        for p2 in PRERED:
            if (t, k, p2) in outs and p2 != p:
                for key in keys:
                    assert torch.equal(o[key], outs[(t, k, p2)][key]), (precision, t, k, p, p2, key)
    for (t, k, p), o in outs.items():
        if t == 1:
            for t2 in (2, 3):
                if (t2, k, p) in outs:
                    other = outs[(t2, k, p)]
                    for s in SIDES:
                        if k == 0:
                            assert maxerr(o['hs' + s], other['hs' + s]) <= FORM_TOL['hs'], (precision, t2, p, s)
                            assert maxerr(o['box' + s], other['box' + s]) <= FORM_TOL['box'], (precision, t2, p, s)
                            continue
                        assert torch.equal(o['hs' + s], other['hs' + s]), (precision, t2, k, s)
                        e = maxerr(o['logits' + s], other['logits' + s])
                        assert e <= 1e-5 * unmasked_logits_scale(o, c, s), (precision, t2, k, s, e)
        if k == 1 and (t, 4, p) in outs:
            other = outs[(t, 4, p)]
            for s in SIDES:
                assert maxerr(o['hs' + s], other['hs' + s]) <= FORM_TOL['hs'], (precision, t, p, s)
                assert maxerr(o['box' + s], other['box' + s]) <= FORM_TOL['box'], (precision, t, p, s)


def run_settings(eng, c, gpu, precision, settings):
    outs = {}
    try:
        for tail, split, pre in settings:
            eng.set_tail_mode(tail)
            eng.set_decoder_split(split)
            eng.set_state_prereduce(pre)
            note = f'{c.id} {precision} tail {tail} split {split} prereduce {pre}'
            out = c.forward(eng, gpu, stages=True)
            check_call(out, c, precision, note, eng)
            outs[(tail, split, pre)] = out
    finally:
        eng.set_tail_mode(0)
        eng.set_decoder_split(0)
        eng.set_state_prereduce(-1)
    return outs


@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_masked_forms_full_cross_product(cid, cases, engines, gpu):
    c = cases[cid]
    for precision in PRECISIONS:
        eng = engines(precision)
        tails = TAILS if precision != 'f32' else (0, 1)
        outs = run_settings(eng, c, gpu, precision, list(itertools.product(tails, SPLITS, PRERED)))
        check_forms(outs, c, precision)
        if precision == 'f32':
            for t in (2, 3):
                with pytest.raises(Exception):
                    eng.set_tail_mode(t)      # the direct 64-row conv exists in the two-plane builds only


@pytest.mark.parametrize('cid', [c[0] for c in LARGE])
def test_masked_forms_covering_subset_at_large_grids(cid, cases, engines, gpu):
    c = cases[cid]
    rows = covering_subset()
    for precision in PRECISIONS:
        settings = [r[1:] for r in rows if r[0] == precision]
        outs = run_settings(engines(precision), c, gpu, precision, settings)
        check_forms(outs, c, precision)


def test_covering_subset_covers_every_pair():
    rows = covering_subset()
    valid = [c for c in itertools.product(PRECISIONS, TAILS, SPLITS, PRERED) if _valid(c)]
    for i, j in itertools.combinations(range(4), 2):
        assert {(r[i], r[j]) for r in rows} == {(c[i], c[j]) for c in valid}, (i, j)


@pytest.mark.parametrize('cid', ['7x9_5x13', '3x11_1x97'])
def test_masked_seams_vs_fp64(cid, cases, engines, gpu):
    """oetr_feature_correlation_masked at tile 32 / 64 with the pre-reduction off and on, and
    oetr_center_estimation_masked (k_heat_conv, not the fused tail) on its outputs."""
    c = cases[cid]
    for precision in ('f32_split_f16@32', 'f32_split_f16@64', 'f32'):
        eng = engines(precision)
        for pre in (0, 1):
            eng.set_state_prereduce(pre)
            try:
                hs1, hs2, mem1, mem2 = eng.feature_correlation(*c.dev(gpu), mask1=c.m['1'], mask2=c.m['2'])
            finally:
                eng.set_state_prereduce(-1)
            assert eng.query_flags() == 0
            note = f'seam {c.id} {precision} prereduce {pre}'
            for key, got in (('memory1', mem1), ('memory2', mem2), ('hs1', hs1), ('hs2', hs2)):
                assert maxerr(got, c.ref[key]) <= TOL[key[:-1]], (note, key)
                fp64_rule(got, c, key, note, precision)
            (h1, w1), (h2, w2) = c.g['1'], c.g['2']
            c1, c2 = eng.center_estimation(hs1, hs2, mem1, mem2, h1, w1, h2, w2, c.img['1'][0], c.img['2'][0],
                                           mask1=c.m['1'], mask2=c.m['2'])
            for s, got in (('1', c1), ('2', c2)):
                assert maxerr(got, c.ref['cxy' + s]) <= TOL['cxy'], (note, s)
                fp64_rule(got, c, 'cxy' + s, note, precision)
                check_special_images(got, c, s, note)


def _module(gpu):
    import imagematching_oetr_amd as pkg
    torch.manual_seed(0)
    model = pkg.OETR(pkg.get_cfg_defaults().OETR).eval()
    sd = model.state_dict()
    w = orc.make_hot_weights(5, sharpen=True)
    sd.update(w)
    model.load_state_dict(sd, strict=True)
    return pkg, model.to(gpu), w


def _exact(pkg, w, gpu):
    exact = pkg.HotPathEngine(w, device=gpu, precision='f32')
    exact.set_decoder_split(1)     # as the module's re-run route (waits for nobody)
    return exact


@pytest.mark.parametrize('defer', [True, False])
def test_module_reruns_an_overflowing_masked_batch_in_exact_fp32(gpu, defer):
    """A masked batch one of whose images trips the f16 range guard is answered with the exact-fp32
    engine's MASKED boxes (the re-run carries the masks), and those are fp32-class against fp64."""
    pkg, model, w = _module(gpu)
    model.hip_defer_check = defer
    f1, f2 = orc.make_features(95, 2, 8, 10), orc.make_features(96, 2, 10, 8)
    f1[1] *= 4.0e5                                   # image 1: a GEMM operand beyond the f16 range
    m1, m2 = orc.make_masks(97, 2, 8, 10, 'tile32:1|weighted'), orc.make_masks(98, 2, 10, 8, 'weighted|tile32:2')
    im1, im2 = (256, 320), (320, 256)
    dev = [t.to(gpu) for t in (f1, f2, orc.position_table(8, 10), orc.position_table(10, 8))]
    b1, b2 = model.boxes_from_features(*dev, im1, im2, m1.to(gpu), m2.to(gpu))
    if defer:
        assert model._pending is not None
    model.hip_flush()
    e1, e2 = _exact(pkg, w, gpu).forward(*dev, im1, im2, mask1=m1, mask2=m2)
    assert torch.equal(b1, e1) and torch.equal(b2, e2) and torch.isfinite(b1).all()
    raw = model.engine().forward(*dev, im1, im2, mask1=m1, mask2=m2)
    assert model.engine().query_flags() & pkg.FLAG_F16_RANGE      # (the default build did trip)
    del raw
    r32 = orc.hot_path(f1, f2, w, im1, im2, mask1=m1, mask2=m2)
    r64 = orc.hot_path(f1.double(), f2.double(), orc.cast_weights(w, torch.float64), im1, im2, mask1=m1, mask2=m2)
    for got, a, b, s in ((b1, r32[0], r64[0], '1'), (b2, r32[1], r64[1], '2')):
        drift = float((a.double() - b).abs().max())
        err = float((got.cpu().double() - b).abs().max())
        margin('masked_overflow_8x10_10x8', 'f32', 'vs fp64 oracle', 'box' + s, err)
        assert err <= max(FP32_CLASS * drift, FLOOR['cxy']), (s, err, drift)


def test_throughput_mode_with_masks_is_the_serial_result_bit_for_bit(gpu):
    """test_throughput_mode_is_the_serial_result_bit_for_bit with masks: hip_streams = 3 (64-row encoder
    workgroups, direct tail, side streams) at queue depth 1 and 2; one batch overflow-injected.  After
    hip_flush() every batch equals the one-batch-at-a-time result bit for bit; the tripped batch equals
    the exact-fp32 engine's masked boxes."""
    pkg, model, w = _module(gpu)
    shapes = [(3, 13, 13, 'weighted|tile64:1|last', 'tile32:2|one|first'),
              (8, 20, 20, 'tile64:2|weighted|one|full', 'last|tile32:5|weighted|zero'),
              (2, 10, 20, 'one|weighted', 'tile64:4|tile32:0')]
    batches = []
    for i in range(12):
        n, h1, h2, k1, k2 = shapes[i % 3]
        f1, f2 = orc.make_features(100 + i, n, h1, h1), orc.make_features(200 + i, n, h2, h2)
        if i == 4:
            f1[0] *= 4.0e5                       # a GEMM operand beyond the f16 range
        m1, m2 = orc.make_masks(300 + i, n, h1, h1, k1), orc.make_masks(400 + i, n, h2, h2, k2)
        batches.append([t.to(gpu) for t in (f1, f2, orc.position_table(h1, h1), orc.position_table(h2, h2))]
                       + [(h1 * 32, h1 * 32), (h2 * 32, h2 * 32), m1.to(gpu), m2.to(gpu)])
    model.hip_streams, model.hip_throughput = 1, True
    serial = []
    for b in batches:
        out = model.boxes_from_features(*b)
        model.hip_flush()
        serial.append([t.clone() for t in out])
    e = _exact(pkg, w, gpu).forward(*batches[4][:6], mask1=batches[4][6], mask2=batches[4][7])
    assert torch.equal(serial[4][0], e[0]) and torch.equal(serial[4][1], e[1])
    model.hip_streams, model.hip_throughput = 3, None
    for depth in (1, 2):
        model.hip_queue_depth = depth
        outs = [model.boxes_from_features(*b) for b in batches]
        model.hip_flush()
        assert len(model._inflight) == 0
        torch.cuda.synchronize()
        for i, (o, r) in enumerate(zip(outs, serial)):
            assert torch.equal(o[0], r[0]) and torch.equal(o[1], r[1]), (depth, i)
    assert model.engine().query_flags() == 0
