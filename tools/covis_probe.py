"""What the co-visibility boxes cost (include/oetr_covis.h, imagematching_oetr_amd/csrc/covis.hip), in one run:

For 8 and 32 pairs of 640 x 640 maps and 8 pairs of 1024 x 1024, with and without masks,
1. the time of one ``oetr_covis_boxes`` call (its clearing kernels, k_covis_warp, k_covis_finish),
2. the time of a ``Tensor.copy_`` that moves the call's ALGORITHMIC bytes - depth1 and depth2 read once and, with
   masks, both masks cleared and written once; the copy reads half of that many bytes and writes the other half -
   the yardstick: the same bytes moved with no arithmetic,
3. the float64 numpy restatement of the same pairs on the host (tests/covis_oracle.py), which the device results
   are also checked against.
Device variants are captured into a HIP graph of CALLS back-to-back calls (the host's enqueue cost is not part of
the number) and replayed between device events; the variants alternate over ROUNDS after a warm-up replay.

    python tools/covis_probe.py [--out profiles/covis_probe.json]

One JSON record.  The call is EXPECTED to take at most 3x the copy (1x for the bytes, up to 2x for about a hundred
float64 operations and nine float64 divisions per pixel, which the copy does not have); that is recorded per cell
(``within_3x_of_copy``) and overall (``expectation_met``), not gated."""
import argparse
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402
import covis_oracle as cvo  # noqa: E402
from imagematching_oetr_amd.covis import covis_boxes  # noqa: E402

CALLS, ROUNDS = 50, 9
DISTINCT = 8                      # distinct scenes per size; larger batches repeat them
KINDS = ('plane', 'plane', 'trunc', 'plane', 'no_overlap', 'plane', 'behind', 'plane')
SHAPES = ((8, 640), (32, 640), (8, 1024))


def scenes_of(size):
    arrays, expected = cvo.scene_batch(KINDS, size, size, seed=900 + size)
    host_ms = []
    for p in range(DISTINCT):
        scene = {k: v[p] for k, v in arrays.items()}
        t = time.perf_counter()
        cvo.restate(scene)
        host_ms.append((time.perf_counter() - t) * 1e3)
    params = np.stack([cvo.param_block({k: v[p] for k, v in arrays.items()}) for p in range(DISTINCT)])
    return arrays, expected, params, host_ms


def cell(dev, n, size, masks, arrays, expected, params):
    rep = n // DISTINCT
    d1 = torch.from_numpy(arrays['depth1']).repeat(rep, 1, 1).to(dev).contiguous()
    d2 = torch.from_numpy(arrays['depth2']).repeat(rep, 1, 1).to(dev).contiguous()
    prm = torch.from_numpy(params).repeat(rep, 1).to(dev).contiguous()
    out = covis_boxes(d1, d2, prm, masks=masks)
    torch.cuda.synchronize()
    for p in range(n):                       # the measured call computes the right thing
        e = expected[p % DISTINCT]
        assert np.array_equal(out['overlap_box1'][p].cpu().numpy(), e['box1'].astype(np.float32)), p
        assert np.array_equal(out['overlap_box2'][p].cpu().numpy(), e['box2'].astype(np.float32)), p
        assert int(out['overlap_count'][p]) == e['count'], p
        if masks:
            assert np.array_equal(out['overlap_mask1'][p].cpu().numpy(), e['mask1']), p
            assert np.array_equal(out['overlap_mask2'][p].cpu().numpy(), e['mask2']), p
    depth_bytes = 2 * n * size * size * 4
    mask_bytes = 2 * 2 * n * size * size if masks else 0          # two masks, each cleared and written
    moved = depth_bytes + mask_bytes
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    graphs = {'covis': graph_of(lambda: covis_boxes(d1, d2, prm, masks=masks, out=out), CALLS),
              'copy': graph_of(lambda: dst.copy_(src), CALLS)}
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / CALLS)
    rec = {'pairs': n, 'map': [size, size], 'masks': masks, 'algorithmic_bytes': moved,
           'inliers_per_call': int(sum(expected[p % DISTINCT]['count'] for p in range(n)))}
    for k in us:
        rec[k + '_us'] = stats(us[k])
        rec[k + '_TBps'] = moved / (rec[k + '_us']['median'] * 1e-6) / 1e12
    rec['spread_us'] = max(rec[k + '_us']['max'] - rec[k + '_us']['min'] for k in us)
    rec['ratio_to_copy'] = rec['covis_us']['median'] / rec['copy_us']['median']
    rec['within_3x_of_copy'] = rec['ratio_to_copy'] <= 3.0
    rec['ns_per_pixel'] = rec['covis_us']['median'] * 1e3 / (n * size * size)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'covis_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('covis_probe.py measures on the GPU: none visible')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda', 0)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/covis_probe.py', 'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__,
           'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/covis_probe.py', 'imagematching_oetr_amd/csrc/covis.hip')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'cells': [], 'host_numpy_ms_per_pair': {}}
    made = {}
    for n, size in SHAPES:
        if size not in made:
            made[size] = scenes_of(size)
            rec['host_numpy_ms_per_pair'][str(size)] = stats(made[size][3])
        arrays, expected, params, host_ms = made[size]
        for masks in (False, True):
            c = cell(dev, n, size, masks, arrays, expected, params)
            c['host_numpy_ms_per_call'] = statistics.median(host_ms) * n
            c['host_over_device'] = c['host_numpy_ms_per_call'] * 1e3 / c['covis_us']['median']
            rec['cells'].append(c)
            print(json.dumps(c), flush=True)
    rec['max_ratio_to_copy'] = max(c['ratio_to_copy'] for c in rec['cells'])
    rec['expectation_met'] = all(c['within_3x_of_copy'] for c in rec['cells'])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps({k: rec[k] for k in ('max_ratio_to_copy', 'expectation_met')}))


if __name__ == '__main__':
    main()
