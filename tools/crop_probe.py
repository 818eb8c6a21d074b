"""What the box -> crop step costs per pair, batched against per pair (include/oetr_crop_batch.h,
imagematching_oetr_amd/csrc/crop_batch.hip against csrc/crop.hip), in one run:

For 8 and 32 pairs of grey 1 x 480 x 640 and colour 3 x 480 x 640 matcher images, size_divisor 1 and 8, boxes
drawn so that every gate passes,
(a) DEVICE time of one ``oetr_overlap_crop_batch`` call against n ``oetr_overlap_crop`` calls - the per-pair route
    is the yardstick, measured in the same run: this tree's per-pair entry (the same pinned arithmetic, three
    launches per pair).  Both are captured into a HIP graph of CALLS back-to-back
    repetitions (the host's enqueue cost is not part of the number) and replayed REPLAYS times between device
    events; the two variants alternate over ROUNDS after a warm-up replay;
(b) eager HOST wall time per pair, device work included (a synchronise closes the window): ITERS calls of
    ``overlap_crop_batch(out=...)`` against ITERS loops of ``overlap_crop`` over the n pairs, alternated likewise.
The batched results are first checked against the per-pair ones, bit for bit.

    python tools/crop_probe.py [--out profiles/crop_probe.json]

One JSON record.  The batched call is EXPECTED to be no slower than the per-pair route in any cell on either
measure; that is recorded per cell and overall (``expectation_met``), not gated."""
import argparse
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import torch  # noqa: E402
from probe_common import graph_of, stats, timed, wall  # noqa: E402
import imagematching_oetr_amd as pkg  # noqa: E402
from imagematching_oetr_amd.hip_engine import _CropInfo, _check, _stream  # noqa: E402

CALLS, REPLAYS, ROUNDS, ITERS = 10, 40, 9, 20      # a device window is 400 calls: 10 ms in the smallest cell
H, W, FRAME = 480, 640, 640
SCALES = (W / FRAME, H / FRAME)          # overlap_scales of a 640 x 480 matcher image under a 640 x 640 OETR frame
CELLS = [(n, c, d) for n in (8, 32) for c in (1, 3) for d in (1, 8)]


def boxes(n, gen):
    """[n,4] boxes in the OETR frame, every side at least 120 px there (>= 90 px in the image): all gates pass."""
    xy = torch.rand(n, 2, generator=gen) * (FRAME * 0.45)
    wh = 120.0 + torch.rand(n, 2, generator=gen) * (FRAME * 0.5 - 120.0)
    return torch.cat([xy, xy + wh], dim=1)


def cell(dev, n, channels, divisor):
    gen = torch.Generator().manual_seed(1000 * n + 10 * channels + divisor)
    ims0 = [torch.rand(1, channels, H, W, generator=gen).to(dev) for _ in range(n)]
    ims1 = [torch.rand(1, channels, H, W, generator=gen).to(dev) for _ in range(n)]
    b0, b1 = boxes(n, gen).to(dev), boxes(n, gen).to(dev)
    table = pkg.crop_pair_table(ims0, ims1, [SCALES] * n, [SCALES] * n)
    held = pkg.overlap_crop_batch(table, b0, b1, True, divisor)
    assert held.valid == [1] * n, held.valid
    per_pair = lambda: [pkg.overlap_crop(ims0[k], ims1[k], b0[k], b1[k], SCALES, SCALES, True, divisor) for k in range(n)]

    def per_pair_loop():                     # results dropped one by one, as a consumer would
        for k in range(n):
            pkg.overlap_crop(ims0[k], ims1[k], b0[k], b1[k], SCALES, SCALES, True, divisor)
    for k, one in enumerate(per_pair()):     # the measured call computes the per-pair result
        for i in (0, 1):
            assert torch.equal(held.crop(k, i), one.crop(i)), (k, i)
    # (a) the per-pair entry on buffers of its own, as the batched call has them: no allocation inside the graphs
    lib = pkg.load_library()
    cap = int(lib.oetr_overlap_crop_capacity(channels, H, W, H, W, divisor, None, None))
    tmp, out = torch.empty(n, 2, cap, device=dev), torch.empty(n, 2, cap, device=dev)
    info = torch.zeros(n, (C.sizeof(_CropInfo) + 7) // 8, dtype=torch.float64, device=dev)
    sc = (C.c_float * 2)(*SCALES)

    def per_pair_entry():
        for k in range(n):
            _check(lib, lib.oetr_overlap_crop(
                ims0[k].data_ptr(), ims1[k].data_ptr(), channels, H, W, H, W, b0[k].data_ptr(), b1[k].data_ptr(), sc, sc,
                1, divisor, 0, tmp[k].data_ptr(), out[k, 0].data_ptr(), out[k, 1].data_ptr(), cap, info[k].data_ptr(),
                _stream(dev)), 'oetr_overlap_crop')
    graphs = {'batched': graph_of(lambda: pkg.overlap_crop_batch(table, b0, b1, True, divisor, out=held), CALLS),
              'per_pair': graph_of(per_pair_entry, CALLS)}
    for k in range(n):                       # the yardstick ran on the same pairs
        assert torch.equal(out[k, 0, :held.crop(k, 0).numel()], held.crop(k, 0).reshape(-1)), k
    eager = {'batched': lambda: [pkg.overlap_crop_batch(table, b0, b1, True, divisor, out=held) for _ in range(ITERS)],
             'per_pair': lambda: [per_pair_loop() for _ in range(ITERS)]}
    for fn in eager.values():
        fn()                                 # warm-up: the allocator's blocks
    dev_us, host_us = {k: [] for k in graphs}, {k: [] for k in eager}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            dev_us[k].append(timed(lambda: [g.replay() for _ in range(REPLAYS)]) * 1e3 / (CALLS * REPLAYS))
        for k, fn in eager.items():
            host_us[k].append(wall(fn) * 1e3 / (ITERS * n))
    geo = held.geometry()
    rec = {'pairs': n, 'channels': channels, 'image': [H, W], 'size_divisor': divisor,
           'output_pixels_per_call': int(sum(int(g.out_w[i]) * int(g.out_h[i]) for g in geo for i in (0, 1))) * channels,
           'launches': {'batched': 2 if divisor == 1 else 3, 'per_pair': 3 * n}}
    for k in graphs:
        rec[f'device_us_per_call_{k}'] = stats(dev_us[k])
        rec[f'host_us_per_pair_{k}'] = stats(host_us[k])
    rec['device_us_per_pair'] = {k: rec[f'device_us_per_call_{k}']['median'] / n for k in graphs}
    rec['device_per_pair_over_batched'] = rec['device_us_per_call_per_pair']['median'] / rec['device_us_per_call_batched']['median']
    rec['host_per_pair_over_batched'] = rec['host_us_per_pair_per_pair']['median'] / rec['host_us_per_pair_batched']['median']
    rec['device_not_slower'] = rec['device_per_pair_over_batched'] >= 1.0
    rec['host_not_slower'] = rec['host_per_pair_over_batched'] >= 1.0
    rec['expectation_met'] = rec['device_not_slower'] and rec['host_not_slower']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'crop_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('crop_probe.py measures on the GPU: none visible')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda', 0)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    csrc = 'imagematching_oetr_amd/csrc/'
    rec = {'tool': 'tools/crop_probe.py', 'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/crop_probe.py', csrc + 'crop_batch.hip', csrc + 'crop.hip', csrc + 'crop_sample.h')},
           'calls_per_graph': CALLS, 'replays_per_window': REPLAYS, 'rounds': ROUNDS, 'eager_iterations': ITERS, 'cells': []}
    for n, channels, divisor in CELLS:
        c = cell(dev, n, channels, divisor)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    rec['min_device_per_pair_over_batched'] = min(c['device_per_pair_over_batched'] for c in rec['cells'])
    rec['min_host_per_pair_over_batched'] = min(c['host_per_pair_over_batched'] for c in rec['cells'])
    rec['expectation_met'] = all(c['expectation_met'] for c in rec['cells'])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps({k: rec[k] for k in ('min_device_per_pair_over_batched', 'min_host_per_pair_over_batched', 'expectation_met')}))


if __name__ == '__main__':
    main()
