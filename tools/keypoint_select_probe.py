"""What selecting keypoints from dense maps costs on the device (include/oetr_keypoint_select.h,
csrc/keypoint_select.hip), in one run.

Cells: 64 and 256 maps of 480 x 640 with descriptor maps of D = 256 at one eighth (60 x 80), and 64 maps of mixed sizes
(480 x 640, 360 x 480, 240 x 320, 600 x 800 in turn); max_keypoints 2048, nms_radius 4, threshold 0.005, border 4.
Scores are uniform random numbers, so nearly every map has more candidates than max_keypoints.  Per cell
  selected      one ``oetr_keypoint_select`` call through ``select_keypoints`` on a prepared table, captured into a HIP
                graph of CALLS back-to-back calls and replayed between device events; the descriptor maps are NCHW, what
                a torch network delivers unless asked otherwise;
  channels-last the same call on the same maps stored channels-last (``[h,w,D]`` storage behind a ``[D,h,w]`` view - no
                copy inside the call either way): the four taps of a keypoint are then 64 adjacent floats per load
                instead of 64 cache lines; the two results must have the same bits;
  (a) copy      ``copy_`` of the call's ALGORITHMIC bytes - every score map and every descriptor map read once, every
                output row written once - captured and replayed the same way;
  (b) torch     the same head written in torch on the device, image by image as a caller has to run it today: five
                ``max_pool2d``, ``nonzero``, ``topk``, ``grid_sample``, ``normalize``.  Timed EAGERLY between device events
                (``nonzero`` reads back and cannot be captured) on TORCH_MAPS maps and scaled to the cell's maps;
  agreement     whether (b) and the call keep the same number of keypoints on those maps (recorded, not asserted -
                tests/test_gpu_keypoint_select.py holds the call to its specification bit for bit).
All variants alternate over ROUNDS after a warm-up; medians.

    python tools/keypoint_select_probe.py [--out profiles/keypoint_select_probe.json] [--dry-run] [--scale S]

``--dry-run`` does everything up to the first device call - input generation (on the CPU, two maps a cell), route (b)
on CPU tensors, the byte counts, the JSON skeleton (printed, not written) - and needs no GPU.  ``--scale`` divides the
map counts for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as met / missed, not gated): less device time than (b), and within three times
(a).  DESIGN 9.3n holds the estimate made before the first measurement."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as nnf  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402

CALLS, ROUNDS = 10, 9
D, K, RADIUS, THRESHOLD, BORDER, CELL = 256, 2048, 4, 0.005, 4, 8
UNIFORM, MIXED = ((480, 640),), ((480, 640), (360, 480), (240, 320), (600, 800))
CELLS = (('64 maps of 480 x 640', 64, UNIFORM), ('256 maps of 480 x 640', 256, UNIFORM), ('64 maps of mixed sizes', 64, MIXED))
TORCH_MAPS = 8


def make_maps(n, sizes, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    scores = [torch.rand(*sizes[i % len(sizes)], device=dev, generator=g) for i in range(n)]
    descriptors = [torch.randn(D, s.shape[0] // CELL, s.shape[1] // CELL, device=dev, generator=g) for s in scores]
    return scores, descriptors


def torch_head(scores, desc):
    """Route (b) for one image: SuperPoint's post-processing as a caller writes it in torch."""
    s = scores[None]
    pool = lambda x: nnf.max_pool2d(x, kernel_size=2 * RADIUS + 1, stride=1, padding=RADIUS)
    zeros = torch.zeros_like(s)
    mask = s == pool(s)
    for _ in range(2):
        supp = pool(mask.float()) > 0
        supp_scores = torch.where(supp, zeros, s)
        mask = mask | ((supp_scores == pool(supp_scores)) & ~supp)
    nms = torch.where(mask, s, zeros)[0]
    kp = torch.nonzero(nms > THRESHOLD)
    sc = nms[kp[:, 0], kp[:, 1]]
    H, W = nms.shape
    keep = (kp[:, 0] >= BORDER) & (kp[:, 0] < H - BORDER) & (kp[:, 1] >= BORDER) & (kp[:, 1] < W - BORDER)
    kp, sc = kp[keep], sc[keep]
    if K < len(sc):
        sc, order = torch.topk(sc, K, dim=0)
        kp = kp[order]
    kp = torch.flip(kp, [1]).float()
    h, w = desc.shape[1:]
    g = kp[None] - CELL / 2 + 0.5
    g = g / torch.tensor([(w * CELL - CELL / 2 - 0.5), (h * CELL - CELL / 2 - 0.5)]).to(g)[None]
    d = nnf.grid_sample(desc[None], (g * 2 - 1).view(1, 1, -1, 2), mode='bilinear', align_corners=True)
    return kp, sc, nnf.normalize(d.reshape(1, desc.shape[0], -1), p=2, dim=1)


def cell(dev, name, n, sizes, dry_run):
    where = torch.device('cpu') if dry_run else dev
    scores, descriptors = make_maps(2 if dry_run else n, sizes, where, seed=n + len(sizes))
    shapes = [sizes[i % len(sizes)] for i in range(n)]
    pixels = sum(H * W for H, W in shapes)
    bytes_in = 4 * pixels + 4 * D * sum((H // CELL) * (W // CELL) for H, W in shapes)
    bytes_out = n * K * (8 + 4 + 4 * D) + 4 * (n + 1) + 8 * n
    rec = {'cell': name, 'maps': n, 'D': D, 'max_keypoints': K, 'nms_radius': RADIUS, 'pixels': pixels,
           'algorithmic_bytes': bytes_in + bytes_out}
    m = min(TORCH_MAPS, len(scores))
    theirs = [torch_head(scores[i], descriptors[i]) for i in range(m)]
    rec['torch_maps_timed'] = m
    rec['torch_kept'] = [int(len(t[1])) for t in theirs]
    if dry_run:
        return rec
    from imagematching_oetr_amd import keypoint_counts, keypoint_map_table, select_keypoints
    table = keypoint_map_table(scores, descriptors)
    kw = dict(nms_radius=RADIUS, threshold=THRESHOLD, remove_borders=BORDER, max_keypoints=K, cell=CELL)
    out = select_keypoints(table, **kw)
    counts = keypoint_counts(out)
    rec['candidates_mean'] = float(counts[:, 0].mean())
    rec['kept_mean'] = float(counts[:, 1].mean())
    rec['torch_keeps_the_same_number'] = counts[:m, 1].tolist() == rec['torch_kept']
    rec['workspace_bytes'] = int(out['workspace'].numel())
    graph = graph_of(lambda: select_keypoints(table, **kw, out=out), CALLS)
    table_last = keypoint_map_table(scores, [d.permute(1, 2, 0).contiguous().permute(2, 0, 1) for d in descriptors])
    out_last = select_keypoints(table_last, **kw)
    rec['channels_last_gives_the_same_bits'] = all(
        torch.equal(out[key].view(torch.int32), out_last[key].view(torch.int32))
        for key in ('keypoints', 'scores', 'descriptors', 'offsets', 'counts'))
    graph_last = graph_of(lambda: select_keypoints(table_last, **kw, out=out_last), CALLS)
    src = torch.empty(rec['algorithmic_bytes'], dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy = graph_of(lambda: dst.copy_(src), CALLS)
    run_torch = lambda: [torch_head(scores[i], descriptors[i]) for i in range(m)]
    run_torch()                                                      # warm-up
    ms = {'selected': [], 'selected_channels_last': [], 'copy': [], 'torch': []}
    for _ in range(ROUNDS):
        ms['selected'].append(timed(graph.replay) / CALLS)
        ms['selected_channels_last'].append(timed(graph_last.replay) / CALLS)
        ms['copy'].append(timed(copy.replay) / CALLS)
        ms['torch'].append(timed(run_torch) * n / m)
    for k in ms:
        rec[k + '_ms'] = stats(ms[k])
    med = lambda k: rec[k + '_ms']['median']
    rec['algorithmic_gb_per_s'] = rec['algorithmic_bytes'] / (med('selected') * 1e-3) / 1e9
    rec['selected_over_copy'] = med('selected') / med('copy')
    rec['torch_over_selected'] = med('torch') / med('selected')
    rec['less_device_time_than_torch'] = med('selected') < med('torch')
    rec['within_three_times_the_copy'] = med('selected') <= 3 * med('copy')
    rec['channels_last_over_copy'] = med('selected_channels_last') / med('copy')
    rec['channels_last_within_three_times_the_copy'] = med('selected_channels_last') <= 3 * med('copy')
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'keypoint_select_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--scale', type=int, default=1)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('keypoint_select_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/keypoint_select_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__,
           'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/keypoint_select_probe.py', 'imagematching_oetr_amd/csrc/keypoint_select.hip',
                                             'imagematching_oetr_amd/csrc/keypoint_select_math.h',
                                             'tests/keypoint_select_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'scale': args.scale, 'cells': []}
    dev = None
    if not args.dry_run:
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
    for name, n, sizes in CELLS:
        c = cell(dev, name, max(1, n // args.scale), sizes, args.dry_run)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    if args.dry_run:
        print(json.dumps(rec, indent=1))
        print('dry run: stopped before the first device call; nothing written')
        return
    rec['expectations'] = {
        'less_device_time_than_torch_in_every_cell': all(c['less_device_time_than_torch'] for c in rec['cells']),
        'within_three_times_the_copy_in_every_cell': all(c['within_three_times_the_copy'] for c in rec['cells']),
        'channels_last_within_three_times_the_copy_in_every_cell': all(c['channels_last_within_three_times_the_copy']
                                                                       for c in rec['cells'])}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
