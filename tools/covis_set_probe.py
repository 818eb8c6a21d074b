"""What ground-truth boxes BY INDEX over a depth-map set cost (include/oetr_covis_set.h, csrc/covis.hip), in one run.

Cells: 64 maps of 640 x 640 with 16 pairs per image (1024 pairs), the same set with 4 pairs per image (256 pairs),
and a mixed set of 480 x 640, 640 x 480 and 640 x 640 maps with 16 pairs per image.  Per cell
  indexed         one ``oetr_covis_boxes_indexed`` call on the set in place (parameter blocks precomputed, as for (a)),
  indexed_gather  ``overlap_boxes_indexed``: the same plus the gather of the parameter blocks from the camera records,
and, in the equal-size cells, the two yardsticks from this tree in the same run:
  (a) stacked     ``oetr_covis_boxes`` on PRE-STACKED maps [P,H,W] per side (the maps of every pair materialised),
  (b) select      ``index_select`` of both sides from the stacked set + (a): the only route without the set entry.
The indexed results are checked bit for bit against (a)'s and a few pairs against the float64 restatement.  Device
variants are captured into a HIP graph of CALLS back-to-back calls and replayed between device events; the variants
alternate over ROUNDS after a warm-up replay; medians.  CALLS is 10 where tools/covis_probe.py has 50: a call of the
1024-pair cell works through 419 M pixels (milliseconds, not tens of microseconds, so ten calls already make a replay
far longer than its launch), and route (b) allocates 3.4 GB of gathered maps per captured call.  The bytes of device
memory each route holds are recorded.

    python tools/covis_set_probe.py [--out profiles/covis_set_probe.json]
                                    [--parent-probe P1.json ... --this-probe T1.json ...]

EXPECTED (recorded per cell and overall as met / missed, not gated): the indexed call is not slower than (b) in any
equal-size cell, and it is within the run's round-to-round spread of (a) - the arithmetic is the same float64 code
and the table loads are per workgroup.

``--parent-probe`` / ``--this-probe``: records of ``tools/covis_probe.py`` run alternately in a checkout of the parent
commit and in this tree in one session; the existing entry's three cells (without masks) are folded into the record
with both medians - EXPECTED to move by at most the larger of 3 % and that probe's spread between rounds."""
import argparse
import hashlib
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402
import covis_set_oracle as cso  # noqa: E402
from imagematching_oetr_amd import DepthSet, overlap_boxes_indexed  # noqa: E402
from imagematching_oetr_amd.covis import covis_boxes  # noqa: E402
from imagematching_oetr_amd.covis_set import covis_boxes_indexed, pair_params  # noqa: E402

CALLS, ROUNDS = 10, 9
N_MAPS = 64
CELLS = (('640x640 x64, 16 pairs per image', ((640, 640),), 16),
         ('640x640 x64, 4 pairs per image', ((640, 640),), 4),
         ('480x640 / 640x480 / 640x640 x64, 16 pairs per image', ((480, 640), (640, 480), (640, 640)), 16))
KEYS = ('overlap_box1', 'overlap_box2', 'overlap_valid', 'overlap_count')


def nbytes(*tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors))


def cell(dev, name, shapes, per_image):
    sizes = tuple(shapes[k % len(shapes)] for k in range(N_MAPS))
    views = cso.make_set(sizes, seed=640)
    ds = DepthSet(dev)
    for v in views:
        ds.add(torch.from_numpy(v['depth']), v['intrinsics'], v['pose'], v['bbox'], v['ratio'])
    pairs = [(i, (i + 1 + k) % N_MAPS) for i in range(N_MAPS) for k in range(per_image)]
    index = torch.tensor(pairs, dtype=torch.int32, device=dev)
    idx1, idx2 = index[:, 0].contiguous(), index[:, 1].contiguous()
    params = pair_params(ds, idx1, idx2)
    table, cameras = ds._commit()
    out = covis_boxes_indexed(table, len(ds), ds.max_pixels, idx1, idx2, params)
    torch.cuda.synchronize()
    count = out['overlap_count'].cpu().numpy()
    checked = 0
    for p in range(0, len(pairs), max(1, len(pairs) // 6)):      # a few pairs against the float64 restatement
        e = cso.restate_pair(views, *pairs[p], T=params[p, :16].cpu().numpy().reshape(4, 4))
        assert np.array_equal(out['overlap_box1'][p].cpu().numpy(), e['box1'].astype(np.float32)), p
        assert np.array_equal(out['overlap_box2'][p].cpu().numpy(), e['box2'].astype(np.float32)), p
        assert int(count[p]) == e['count'], p
        checked += 1
    source_pixels = int(sum(sizes[i][0] * sizes[i][1] for i, _ in pairs))
    set_bytes = ds.map_bytes + nbytes(table, cameras)
    call_bytes = nbytes(idx1, idx2, params, out['workspace'], *(out[k] for k in KEYS))
    rec = {'cell': name, 'maps': N_MAPS, 'pairs': len(pairs), 'source_pixels_per_call': source_pixels,
           'valid_pairs': int((count > 0).sum()), 'inliers_per_call': int(count.clip(min=0).sum()),
           'pairs_restated_on_the_host': checked,
           'device_bytes': {'indexed': set_bytes + call_bytes}}
    out_g = overlap_boxes_indexed(ds, index)
    graphs = {'indexed': graph_of(lambda: covis_boxes_indexed(table, len(ds), ds.max_pixels, idx1, idx2, params, out=out), CALLS),
              'indexed_gather': graph_of(lambda: overlap_boxes_indexed(ds, index, out=out_g), CALLS)}
    if len(shapes) == 1:
        stacked = torch.stack(ds._maps)
        d1, d2 = stacked.index_select(0, idx1.long()), stacked.index_select(0, idx2.long())
        out_a = covis_boxes(d1, d2, params)
        torch.cuda.synchronize()
        for k in KEYS:                                           # the set entry computes what the stacked entry computes
            assert torch.equal(out[k], out_a[k]), k
        out_b = {k: v.clone() for k, v in out_a.items()}
        graphs['stacked'] = graph_of(lambda: covis_boxes(d1, d2, params, out=out_a), CALLS)
        graphs['select'] = graph_of(lambda: covis_boxes(stacked.index_select(0, idx1.long()),
                                                        stacked.index_select(0, idx2.long()), params, out=out_b), CALLS)
        pair_maps = nbytes(d1, d2)
        rec['device_bytes']['stacked'] = pair_maps + call_bytes - nbytes(idx1, idx2)
        rec['device_bytes']['select'] = nbytes(stacked) + pair_maps + call_bytes
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / CALLS)
    for k in us:
        rec[k + '_us'] = stats(us[k])
    rec['spread_us'] = max(rec[k + '_us']['max'] - rec[k + '_us']['min'] for k in us)
    rec['indexed_Gpixels_per_s'] = source_pixels / (rec['indexed_us']['median'] * 1e-6) / 1e9
    rec['ns_per_pixel'] = rec['indexed_us']['median'] * 1e3 / source_pixels
    if 'stacked' in us:
        rec['indexed_over_stacked'] = rec['indexed_us']['median'] / rec['stacked_us']['median']
        rec['indexed_over_select'] = rec['indexed_us']['median'] / rec['select_us']['median']
        rec['not_slower_than_select'] = rec['indexed_us']['median'] <= rec['select_us']['median']
        ab_spread = max(rec[k + '_us']['max'] - rec[k + '_us']['min'] for k in ('indexed', 'stacked'))
        rec['within_spread_of_stacked'] = abs(rec['indexed_us']['median'] - rec['stacked_us']['median']) <= ab_spread
        rec['spread_indexed_stacked_us'] = ab_spread
    return rec


def existing_entry(parent_files, this_files):
    """``tools/covis_probe.py`` records of the parent commit and of this tree -> per cell (no masks) both medians of the
    runs' medians, the change, and the bound: the larger of 3 % and the spread between rounds (largest in any run)."""
    load = lambda files: [json.loads(Path(f).read_text()) for f in files]
    parent, this = load(parent_files), load(this_files)
    cells = []
    for k, c in enumerate(parent[0]['cells']):
        if c['masks']:
            continue
        p = [r['cells'][k]['covis_us']['median'] for r in parent]
        t = [r['cells'][k]['covis_us']['median'] for r in this]
        spread = max(r['cells'][k]['covis_us']['max'] - r['cells'][k]['covis_us']['min'] for r in parent + this)
        pm, tm = statistics.median(p), statistics.median(t)
        bound = max(0.03 * pm, spread)
        cells.append({'pairs': c['pairs'], 'map': c['map'], 'parent_us': pm, 'this_us': tm, 'parent_runs_us': p,
                      'this_runs_us': t, 'change': tm / pm - 1.0, 'spread_between_rounds_us': spread,
                      'bound_us': bound, 'within_bound': abs(tm - pm) <= bound})
    return {'tool': 'tools/covis_probe.py, run alternately in a checkout of the parent commit and in this tree',
            'runs_each': [len(parent), len(this)], 'cells': cells,
            'expectation_met': all(c['within_bound'] for c in cells)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'covis_set_probe.json'))
    ap.add_argument('--parent-probe', nargs='*', default=[])
    ap.add_argument('--this-probe', nargs='*', default=[])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('covis_set_probe.py measures on the GPU: none visible')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda', 0)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/covis_set_probe.py', 'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__,
           'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/covis_set_probe.py', 'imagematching_oetr_amd/csrc/covis.hip')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'cells': []}
    for name, shapes, per_image in CELLS:
        c = cell(dev, name, shapes, per_image)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    equal = [c for c in rec['cells'] if 'stacked_us' in c]
    rec['expectations'] = {'not_slower_than_select_in_every_equal_size_cell': all(c['not_slower_than_select'] for c in equal),
                           'within_spread_of_stacked_in_every_equal_size_cell': all(c['within_spread_of_stacked'] for c in equal)}
    if args.parent_probe and args.this_probe:
        rec['existing_entry_vs_parent'] = existing_entry(args.parent_probe, args.this_probe)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps({k: rec[k] for k in ('expectations', 'existing_entry_vs_parent') if k in rec}))


if __name__ == '__main__':
    main()
