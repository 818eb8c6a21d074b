"""What assembling matcher output into origin-frame match lists costs on the device (include/oetr_match_assembly.h,
csrc/match_assembly.hip), in one run.

Cells: 1024 pairs (64 maps' worth at 16 pairs per image, as in tools/match_score_probe.py) and 256 pairs (4 per image),
2048 keypoints per side and pair, half of the rows of side 0 matched, int32 matches, with confidences.  Per cell
  assembled     one ``oetr_assemble_matches`` call through ``assemble_matches`` on device tensors (the joined form),
and three yardsticks, taken in the same run:
  (a) copy      a ``Tensor.copy_`` that moves the call's ALGORITHMIC bytes - per keypoint row of side 0: 8 B keypoint,
                4 B match, 4 B confidence read, 16 B origin and 28 B of list row written; per row of side 1: 8 B read,
                16 B written; the copy reads half of that many bytes and writes the other half;
  (b) host      what a caller does without the call: the geometry read, then per pair the keypoints and matches read
                back, ``keypoints_to_origin`` on both sides, ``nonzero`` / indexing, the float32 rounding - and at the
                end the concatenation and the upload.  Host wall time, on HOST_PAIRS pairs, per pair;
  (c) torch     a restatement in torch on the device, vectorised over the pairs, with ``nonzero`` (which synchronises,
                so it cannot be captured): timed EAGERLY between device events - device time plus its forced
                synchronisations - next to the call timed the same way (``assembled_eager``).
The first pairs are first checked bit for bit against the numpy specification.  ``assembled`` and ``copy`` are captured
into a HIP graph of CALLS back-to-back calls and replayed between device events; all variants alternate over ROUNDS
after a warm-up; medians.

    python tools/match_assembly_probe.py [--out profiles/match_assembly_probe.json] [--dry-run] [--keypoints K] [--scale S]

``--dry-run`` does everything up to the first device call - input generation, the host route (b) on CPU tensors, the
JSON skeleton (printed, not written) - and needs no GPU.  ``--keypoints`` / ``--scale`` (divides the pair counts)
shrink the workload for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as met / missed, not gated): less device time than (c), less wall time than
(b) for the same pairs, and within 3x of (a)."""
import argparse
import ctypes as C
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
import match_assembly_oracle as mao  # noqa: E402

CALLS, ROUNDS = 10, 9
CELLS = (('16 pairs per image', 1024), ('4 pairs per image', 256))
BYTES_PER_ROW0 = {'kp0': 8, 'matches': 4, 'conf': 4, 'origin0': 16, 'index0': 4, 'index1': 4, 'k1': 8, 'k2': 8, 'mconf': 4}
BYTES_PER_ROW1 = {'kp1': 8, 'origin1': 16}
HOST_PAIRS = 32                     # pairs route (b) is timed on
CHECKED_PAIRS = 8                   # pairs checked against the specification


def make_inputs(P, K, seed):
    """One cell's call on the host, in the layout of ``mao.make_call``."""
    rng = np.random.default_rng(seed)
    info = np.zeros(P, mao.INFO_DTYPE)
    info['valid'] = 1
    info['ratio'] = rng.uniform(0.35, 2.8, size=(P, 2, 2))
    info['sbox'][:, :, :2] = rng.uniform(1.0, 200.0, size=(P, 2, 2)).astype(np.float32)
    scales = np.array(mao.SCALES)[rng.integers(0, len(mao.SCALES), size=(P, 2))]
    kp0 = rng.uniform(0.0, 640.0, size=(P * K, 2)).astype(np.float32)
    kp1 = rng.uniform(0.0, 640.0, size=(P * K, 2)).astype(np.float32)
    matches = np.where(rng.random(P * K) < 0.5, rng.integers(0, K, size=P * K), -1).astype(np.int32)
    off = (np.arange(P + 1, dtype=np.int64) * K).astype(np.int32)
    return dict(info=info, scales=scales, kp0=kp0, kp1=kp1, off0=off, off1=off.copy(), matches=matches,
                conf=rng.random(P * K).astype(np.float32))


def host_route(t, pairs, K, dev):
    """Route (b) on ``pairs``: ``t`` holds the call's tensors where the matcher left them (on ``dev``; CPU tensors in a
    dry run).  Returns (k1, k2, mconf, lengths) as uploaded, and the milliseconds per pair."""
    from imagematching_oetr_amd import keypoints_to_origin
    from imagematching_oetr_amd.hip_engine import _CropInfo
    t0 = time.perf_counter()
    raw = t['crops'].cpu().numpy().tobytes()                           # the geometry read: all records at once
    geo = (_CropInfo * (len(raw) // C.sizeof(_CropInfo))).from_buffer_copy(raw)
    scales = t['scales'].cpu().numpy()
    k1, k2, mconf, lengths = [], [], [], []
    for p in pairs:
        rows = slice(p * K, (p + 1) * K)
        kp0, kp1 = t['kp0'][rows].cpu().numpy(), t['kp1'][rows].cpu().numpy()
        matches, conf = t['matches'][rows].cpu().numpy(), t['conf'][rows].cpu().numpy()
        g = geo[p]
        o = [keypoints_to_origin(kp, torch.tensor([[g.ratio[i][0], g.ratio[i][1]]]),
                                 torch.tensor(list(g.sbox[i]), dtype=torch.float32), tuple(scales[p, i]))
             for i, kp in enumerate((kp0, kp1))]
        valid = matches > -1
        index0, index1 = np.nonzero(valid)[0], matches[valid]
        k1.append(o[0][index0].astype(np.float32))
        k2.append(o[1][index1].astype(np.float32))
        mconf.append(conf[valid])
        lengths.append(len(index0))
    up = [torch.from_numpy(np.concatenate(x)).to(dev) for x in (k1, k2, mconf)]
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return up, lengths, (time.perf_counter() - t0) * 1e3 / len(pairs)


def torch_route(t, P, K):
    """Route (c): the call restated in torch on the device, vectorised over equally long pairs."""
    info = t['crops']
    ratio = info[:, 11:15].reshape(P, 2, 2).float()                    # oetr_crop_info.ratio: bytes 88..119
    sbox = info.view(torch.float32)[:, 30:38].reshape(P, 2, 4)[:, :, :2]   # .sbox: bytes 120..151
    pair = torch.arange(P, device=info.device).repeat_interleave(K)
    origin = [((kp / ratio[pair, i]) + sbox[pair, i]).double() * t['scales'][pair, i]
              for i, kp in enumerate((t['kp0'], t['kp1']))]
    m = t['matches']
    valid = (m > -1) & (m < K)
    index = torch.nonzero(valid)[:, 0]                                 # synchronises
    index1 = m[index]
    lengths = valid.view(P, K).sum(1)
    offsets = torch.cat([lengths.new_zeros(1), lengths.cumsum(0)]).int()
    return dict(origin0=origin[0], origin1=origin[1], index0=(index % K).int(), index1=index1,
                k1=origin[0][index].float(), k2=origin[1][pair[index] * K + index1].float(), mconf=t['conf'][index],
                offsets=offsets)


def cell(dev, name, P, K, dry_run):
    call = make_inputs(P, K, seed=2048 + P)
    N = P * K
    moved = {k: v * N for k, v in {**BYTES_PER_ROW0, **BYTES_PER_ROW1}.items()}
    rec = {'cell': f'{P} pairs x {K} keypoints per side, {name}', 'pairs': P, 'keypoints_per_side': K, 'rows': N,
           'matched_share': float((call['matches'] > -1).mean()), 'algorithmic_bytes': moved,
           'algorithmic_bytes_total': sum(moved.values())}
    host_pairs = list(range(0, P, max(1, P // HOST_PAIRS)))[:HOST_PAIRS]
    where = torch.device('cpu') if dry_run else dev
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(where)
    t = dict(crops=as_t(call['info'].view(np.float64).reshape(P, -1)), scales=as_t(call['scales']), kp0=as_t(call['kp0']),
             kp1=as_t(call['kp1']), matches=as_t(call['matches']), conf=as_t(call['conf']), offsets0=as_t(call['off0']),
             offsets1=as_t(call['off1']))
    host_ms = []
    for _ in range(1 if dry_run else 3):
        up, lengths, ms = host_route(t, host_pairs, K, where)
        host_ms.append(ms)
    rec['host_pairs_timed'] = len(host_pairs)
    rec['host_ms_per_pair'] = stats(host_ms)
    rec['host_ms_for_all_pairs'] = statistics.median(host_ms) * P
    if dry_run:
        return rec
    from imagematching_oetr_amd import assemble_matches
    out = assemble_matches(**t)
    torch.cuda.synchronize()
    # bit for bit against the specification on the first pairs, and against route (b) on its pairs
    n = CHECKED_PAIRS
    sub = dict(info=call['info'][:n], scales=call['scales'][:n], kp0=call['kp0'][:n * K], kp1=call['kp1'][:n * K],
               off0=call['off0'][:n + 1], off1=call['off1'][:n + 1], matches=call['matches'][:n * K], conf=call['conf'][:n * K])
    want = mao.assemble(**sub)
    total = int(want['offsets'][-1])
    offsets = out['offsets'].cpu().numpy()
    assert offsets[:n + 1].tolist() == want['offsets'].tolist() and out['counts'][:n].cpu().numpy().tolist() == want['counts'].tolist()
    for k in ('origin0', 'origin1'):
        assert mao.equal_bits(out[k][:n * K].cpu().numpy(), want[k]), k
    for k in ('index0', 'index1', 'k1', 'k2', 'mconf'):
        assert mao.equal_bits(out[k][:total].cpu().numpy(), want[k][:total]), k
    for p, rows in zip(host_pairs, np.split(up[0].cpu().numpy(), np.cumsum(lengths)[:-1])):
        assert mao.equal_bits(out['k1'][int(offsets[p]):int(offsets[p + 1])].cpu().numpy(), rows), p
    rec['matches_kept'] = int(offsets[-1])
    rec['few'] = int(out['n_few'].item())
    theirs = torch_route(t, P, K)
    rec['torch_route_equals_the_call'] = bool(all(
        mao.equal_bits(theirs[k].cpu().numpy(), out[k][:len(theirs[k])].cpu().numpy()) for k in theirs))
    total_bytes = rec['algorithmic_bytes_total']
    src, dst = (torch.empty(total_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    src.zero_()
    graphs = {'assembled': graph_of(lambda: assemble_matches(**t, out=out), CALLS), 'copy': graph_of(lambda: dst.copy_(src), CALLS)}
    eager = {'assembled_eager': lambda: [assemble_matches(**t, out=out) for _ in range(CALLS)],
             'torch': lambda: [torch_route(t, P, K) for _ in range(CALLS)]}
    for fn in eager.values():
        fn()                                                            # warm-up
    us = {k: [] for k in (*graphs, *eager)}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / CALLS)
        for k, fn in eager.items():
            us[k].append(timed(fn) * 1e3 / CALLS)
    for k in us:
        rec[k + '_us'] = stats(us[k])
    rec['spread_us'] = max(rec[k + '_us']['max'] - rec[k + '_us']['min'] for k in us)
    med = lambda k: rec[k + '_us']['median']
    rec['rows_per_s'] = N / (med('assembled') * 1e-6)
    rec['algorithmic_bytes_per_s'] = total_bytes / (med('assembled') * 1e-6)
    rec['ratio_to_copy'] = med('assembled') / med('copy')
    rec['torch_over_assembled'] = med('torch') / med('assembled')
    rec['torch_over_assembled_eager'] = med('torch') / med('assembled_eager')
    rec['host_over_assembled'] = rec['host_ms_for_all_pairs'] * 1e3 / med('assembled')
    rec['less_device_time_than_torch'] = med('assembled') < med('torch') and med('assembled_eager') < med('torch')
    rec['less_wall_time_than_host'] = med('assembled_eager') < rec['host_ms_for_all_pairs'] * 1e3
    rec['within_3x_of_copy'] = rec['ratio_to_copy'] <= 3.0
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'match_assembly_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--keypoints', type=int, default=2048)
    ap.add_argument('--scale', type=int, default=1)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('match_assembly_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/match_assembly_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__, 'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/match_assembly_probe.py', 'imagematching_oetr_amd/csrc/match_assembly.hip',
                                             'tests/match_assembly_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'bytes_per_row_of_side0': BYTES_PER_ROW0,
           'bytes_per_row_of_side1': BYTES_PER_ROW1, 'cells': []}
    dev = None
    if not args.dry_run:
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
    for name, pairs in CELLS:
        c = cell(dev, name, max(1, pairs // args.scale), args.keypoints, args.dry_run)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    if args.dry_run:
        print(json.dumps(rec, indent=1))
        print('dry run: stopped before the first device call; nothing written')
        return
    rec['expectations'] = {k + '_in_every_cell': all(c[k] for c in rec['cells'])
                           for k in ('less_device_time_than_torch', 'less_wall_time_than_host', 'within_3x_of_copy')}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
