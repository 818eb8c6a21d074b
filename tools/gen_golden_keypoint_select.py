#!/usr/bin/env python
"""Write tests/keypoint_select_expected.json: the results of the keypoint-selection specification
(tests/keypoint_select_oracle.py) on the pinned calls of tests/keypoint_select_cases.py, and the margin
measured against a torch restatement on the CPU.

The inputs are a RECIPE (seeds, shapes) regenerated bit for bit; per call the file records the counters, the kept
raster indices in output order, the scores' bit patterns and a digest of the descriptors' bytes.

The torch restatement (:func:`torch_head`) is SuperPoint's published post-processing written with torch's own
operators: ``F.max_pool2d`` for ``simple_nms``, ``nonzero``, ``torch.topk``, ``F.grid_sample(align_corners=True)``,
``F.normalize``.  On the pinned maps (pairwise distinct scores) its keypoints, scores, counts and order must EQUAL the
specification's; its descriptors differ by rounding, because torch's CPU kernels choose their own contraction and
vector order.  The largest absolute difference over all pinned calls is recorded as ``torch_descriptor_margin``;
``tests/test_keypoint_select_cpu.py`` gates at four times that value.  ``--margin X`` writes a given margin instead of
measuring one (what the regeneration test does with the recorded value).

Usage:  python tools/gen_golden_keypoint_select.py [--out tests/keypoint_select_expected.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.dont_write_bytecode = True
sys.path.insert(0, str(REPO / 'tests'))

import keypoint_select_cases as ksc  # noqa: E402
import keypoint_select_oracle as kso  # noqa: E402


def torch_head(S, F, nms_radius, threshold, remove_borders, max_keypoints, cell):
    """``(keypoints [K,2] float32 (x, y), scores [K], descriptors [K,D], candidates)`` with torch on the CPU."""
    import torch
    import torch.nn.functional as nnf
    scores, desc = torch.as_tensor(S)[None], torch.as_tensor(F)[None]

    def max_pool(x):
        return nnf.max_pool2d(x, kernel_size=nms_radius * 2 + 1, stride=1, padding=nms_radius)

    zeros = torch.zeros_like(scores)
    max_mask = scores == max_pool(scores)
    for _ in range(2):
        supp_mask = max_pool(max_mask.float()) > 0
        supp_scores = torch.where(supp_mask, zeros, scores)
        new_max_mask = supp_scores == max_pool(supp_scores)
        max_mask = max_mask | (new_max_mask & (~supp_mask))
    nms = torch.where(max_mask, scores, zeros)[0]
    kp = torch.nonzero(nms > threshold)                             # (y, x), raster order
    sc = nms[kp[:, 0], kp[:, 1]]
    H, W = nms.shape
    b = remove_borders
    keep = (kp[:, 0] >= b) & (kp[:, 0] < H - b) & (kp[:, 1] >= b) & (kp[:, 1] < W - b)
    kp, sc = kp[keep], sc[keep]
    candidates = len(sc)
    if max_keypoints < len(sc):
        sc, order = torch.topk(sc, max_keypoints, dim=0)
        kp = kp[order]
    kp = torch.flip(kp, [1]).float()                                # (x, y)
    _, _, h, w = desc.shape
    g = kp[None] - cell / 2 + 0.5
    g = g / torch.tensor([(w * cell - cell / 2 - 0.5), (h * cell - cell / 2 - 0.5)]).to(g)[None]
    g = g * 2 - 1
    d = nnf.grid_sample(desc, g.view(1, 1, -1, 2), mode='bilinear', align_corners=True)
    d = nnf.normalize(d.reshape(1, desc.shape[1], -1), p=2, dim=1)
    return kp.numpy(), sc.numpy(), d[0].t().contiguous().numpy(), candidates


def torch_margin():
    """The largest absolute descriptor difference between the specification and :func:`torch_head` over the pinned
    calls; everything else must be equal."""
    worst = 0.0
    for case in ksc.PINNED:
        S, F = ksc.inputs(case)
        p = ksc.parameters(case)
        spec = kso.select_image(S, F, **p)
        kp, sc, d, cand = torch_head(S, F, **p)
        assert cand == spec['counts'][0] and len(sc) == spec['counts'][1], case[0]
        assert np.array_equal(kp, spec['keypoints']), case[0]
        assert np.array_equal(sc.view(np.uint32), spec['scores'].view(np.uint32)), case[0]
        if d.size:
            worst = max(worst, float(np.abs(d.astype(np.float64) - spec['descriptors']).max()))
    return worst


def build(margin=None):
    return dict(specification='tests/keypoint_select_oracle.py', calls=[ksc.record(case) for case in ksc.PINNED],
                torch_descriptor_margin=torch_margin() if margin is None else float(margin))


def dumps(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + '\n'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=str(REPO / 'tests' / 'keypoint_select_expected.json'))
    ap.add_argument('--margin', type=float, default=None)
    args = ap.parse_args()
    doc = build(args.margin)
    Path(args.out).write_text(dumps(doc))
    print(f"{args.out}: {len(doc['calls'])} calls, torch descriptor margin {doc['torch_descriptor_margin']:.3e}")


if __name__ == '__main__':
    main()
