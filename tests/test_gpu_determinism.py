"""A forward is a pure function of its inputs: repeated forwards return bit-identical boxes,
whatever ran before them.

Regression test for the timing-dependent linear-attention states of round 3 (DESIGN 3.2,
csrc/encoder.hip: OETR_SPLIT_STATE, csrc/common.h: mma16_split3 and the OETR_SOAK_AMP amplifiers).  What
exposed them - and what this test therefore does - is INTERLEAVING shapes: a big batch between
two forwards of a small one leaves the weights cold in L2, the waves of a workgroup drift apart
behind their weight loads, and the ragged last tile of an image (a workgroup with short GEMM
steps) is where one head's state then came out wrong: 2-800 of 25 000 forwards depending on the
mode; a loop over ONE shape showed nothing.  tools/determinism_hunt.py is the long form
(buffer-level localisation, time budget, library variants).
"""
import pytest
import torch

import imagematching_oetr_amd as pkg

pytestmark = pytest.mark.gpu

# (pairs, h1, w1, h2, w2): ragged last tiles of 16, 36 / 56 and 49 rows, an exact fit, a big batch
SHAPES = [(2, 20, 20, 20, 20), (8, 20, 20, 20, 20), (2, 10, 10, 6, 20), (3, 25, 25, 25, 25), (1, 32, 32, 32, 32)]


@pytest.fixture(scope='module')
def model():
    torch.manual_seed(0)
    return pkg.OETR(pkg.get_cfg_defaults().OETR).eval()


@pytest.mark.parametrize('precision,tile,rounds,attention,prereduce',
                         [('f32_split_f16', 64, 400, 'linear', 0), ('f32_split_qk16', 64, 300, 'linear', 0),
                          ('f16', 64, 400, 'linear', 0), ('bf16', 64, 150, 'linear', 0),
                          ('f32_split_f16', 32, 300, 'linear', 0), ('f32_split_qk16', 32, 200, 'linear', 0),
                          ('f16', 32, 150, 'linear', 0), ('f32', 32, 40, 'linear', 0),
                          # the state pre-reduction launch (oetr_set_state_prereduce) forced on
                          ('f32_split_f16', 64, 200, 'linear', 1), ('f32_split_qk16', 64, 150, 'linear', 1),
                          ('f32_split_f16', 32, 150, 'linear', 1),
                          ('f32_split_f16', 32, 100, 'full', 0),     # (the all-pairs mode's MFMA triples are fenced too)
                          ('f32_split_f16', 64, 100, 'full', 0),     # (tile request ignored by the all-pairs mode: 32 rows)
                          ('f32', 32, 20, 'full', 0)])
def test_forward_is_a_function_of_its_inputs(model, precision, tile, rounds, attention, prereduce):
    _interleaved(model, precision, tile, rounds, attention, prereduce, 0)


@pytest.mark.parametrize('split', [1, 4])
def test_forward_is_a_function_of_its_inputs_decoder_split(model, split):
    """The decoder chain pinned to one workgroup per image (rounds 1-3) and to four (round 4: in-launch
    all-reduces as tagged granules - every workgroup adds the four partials in the same order); the
    automatic rule, which the cases above run, picks four for these batch sizes."""
    _interleaved(model, 'f32_split_f16', 64, 150, 'linear', 0, split)


@pytest.mark.parametrize('precision,tile,rounds', [('f32_split_f16', 64, 200), ('f32_split_f16', 32, 150), ('f32', 32, 30)])
def test_masked_forward_is_a_function_of_its_inputs(model, precision, tile, rounds):
    """The MASKED instantiations of the encoder kernels (forward_dummy's masks) are kernels
    of their own: same interleaving, masks with holes on every shape."""
    _interleaved(model, precision, tile, rounds, 'linear', 0, 0, masked=True)


def _interleaved(model, precision, tile, rounds, attention, prereduce, split, masked=False):
    dev = torch.device('cuda', 0)
    eng = pkg.HotPathEngine(model.hot_path_state(), device=dev, precision=precision, enc_tile=tile,
                            attention=attention)
    if prereduce:
        eng.set_state_prereduce(prereduce)
    if split:
        eng.set_decoder_split(split)
    gen = torch.Generator().manual_seed(1)
    cases = []
    for n, h1, w1, h2, w2 in SHAPES:
        f1 = (torch.rand(n, 256, h1, w1, generator=gen) - 0.5).to(dev)
        f2 = (torch.rand(n, 256, h2, w2, generator=gen) - 0.5).to(dev)
        p1 = model.pos_encoding(f1.cpu()).contiguous().to(dev)
        p2 = model.pos_encoding(f2.cpu()).contiguous().to(dev)
        cases.append((f1, f2, p1, p2, (h1 * 32, w1 * 32), (h2 * 32, w2 * 32)))
    kws = [{} for _ in cases]
    if masked:
        from oracle import oetr_oracle as orc
        kws = [dict(mask1=orc.make_masks(50 + i, n, h1, w1, 'holes').to(dev), mask2=orc.make_masks(60 + i, n, h2, w2, 'holes').to(dev))
               for i, (n, h1, w1, h2, w2) in enumerate(SHAPES)]
    cases_kw = list(zip(cases, kws))
    refs = [eng.forward(*c, stages=True, **kw) for c, kw in cases_kw]
    keys = ('memory1', 'memory2', 'hs1', 'hs2', 'box1', 'box2')
    refs = [{k: r[k].clone() for k in keys} for r in refs]
    differing, runs = [], 0
    for rnd in range(rounds):
        for ci, (c, kw) in enumerate(cases_kw):
            if runs % 3 == 0:   # disturb the workspace: a shorter encoder run of the same shape
                eng.forward(*c, stages=True, enc_layers=1 + runs % 5, **kw)
            out = eng.forward(*c, stages=True, **kw)
            runs += 1
            bad = [k for k in keys if not torch.equal(out[k], refs[ci][k])]
            if bad:
                differing.append((rnd, SHAPES[ci], bad, float((out['box1'] - refs[ci]['box1']).abs().max())))
    assert not differing, f'{len(differing)} of {runs} forwards differ from the first of their shape: {differing[:5]}'
    assert eng.query_flags() == 0


def test_amplified_soak_build_is_deterministic(model):
    """The tripwire of the split-f16 linear-attention state (csrc/encoder.hip: OETR_SPLIT_STATE - shipped on
    evidence, its round-2 failure mode never named): ``liboetr_hip_soak.so`` is the library
    with BOTH amplifiers of round 4's hazard study compiled into the encoder kernels (``-DOETR_SOAK_AMP=3``:
    ``s_waitcnt vmcnt(0)`` before every GEMM step - the waves of a workgroup drift apart - and ``s_setprio 3``
    around the state).  Under them the two-path forms of that state failed 14 .. 8 002 of 37 000 forwards;
    the shipped one-path form must show 0 - interleaved shapes, both tile sizes, 20 s in every GPU run."""
    import time
    from pathlib import Path
    from imagematching_oetr_amd import hip_engine
    soak = Path(hip_engine.LIB_PATH).with_name('liboetr_hip_soak.so')
    assert soak.exists(), f'{soak} not built (make -C imagematching_oetr_amd/csrc)'
    shipped = hip_engine.load_library()
    dev = torch.device('cuda', 0)
    try:
        hip_engine._lib = hip_engine.load_library(str(soak))
        assert hip_engine._lib is not shipped
        total = 0
        for tile, budget in ((64, 10.0), (32, 10.0)):
            eng = pkg.HotPathEngine(model.hot_path_state(), device=dev, precision='f32_split_f16', enc_tile=tile)
            assert eng.lib is hip_engine._lib
            gen = torch.Generator().manual_seed(1)
            cases = []
            for n, h1, w1, h2, w2 in SHAPES:
                f1 = (torch.rand(n, 256, h1, w1, generator=gen) - 0.5).to(dev)
                f2 = (torch.rand(n, 256, h2, w2, generator=gen) - 0.5).to(dev)
                p1 = model.pos_encoding(f1.cpu()).contiguous().to(dev)
                p2 = model.pos_encoding(f2.cpu()).contiguous().to(dev)
                cases.append((f1, f2, p1, p2, (h1 * 32, w1 * 32), (h2 * 32, w2 * 32)))
            keys = ('memory1', 'memory2', 'hs1', 'hs2', 'box1', 'box2')
            refs = [{k: v.clone() for k, v in eng.forward(*c, stages=True).items() if k in keys} for c in cases]
            differing, runs, t0 = [], 0, time.time()
            while time.time() - t0 < budget:
                for ci, c in enumerate(cases):
                    if runs % 3 == 0:
                        eng.forward(*c, stages=True, enc_layers=1 + runs % 5)
                    out = eng.forward(*c, stages=True)
                    runs += 1
                    bad = [k for k in keys if not torch.equal(out[k], refs[ci][k])]
                    if bad:
                        differing.append((tile, runs, SHAPES[ci], bad))
            assert not differing, (f'{len(differing)} of {runs} forwards of the AMPLIFIED build differ from the first of '
                                   f'their shape: {differing[:5]} - set OETR_SPLIT_STATE 0 (csrc/encoder.hip)')
            assert runs >= 500, runs        # (the loop really ran: ~200 forwards per second)
            total += runs
            del eng
    finally:
        hip_engine._lib = shipped


def test_neck_is_a_function_of_its_inputs():
    """The same for the HIP neck: three map sizes interleaved."""
    from oracle import oetr_oracle as orc
    dev = torch.device('cuda', 0)
    neck = pkg.NeckEngine(orc.make_neck_weights(8), device=dev)
    maps = [orc.make_backbone_features(72, 1, 6, 10).to(dev), orc.make_backbone_features(73, 8, 40, 40).to(dev),
            orc.make_backbone_features(74, 3, 26, 34).to(dev)]
    refs = [neck.forward(m).clone() for m in maps]
    differing = []
    for rnd in range(60):
        for i, m in enumerate(maps):
            if not torch.equal(neck.forward(m), refs[i]):
                differing.append((rnd, i))
    assert not differing, f'{len(differing)} of 180 neck forwards differ: {differing[:5]}'
