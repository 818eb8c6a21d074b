"""What matching descriptor sets by nearest neighbours costs on the device (include/oetr_nn_match.h,
csrc/nn_match.hip), in one run.

Cells: 256 pairs x 2048 x 2048 descriptors of D = 256, and 1024 pairs x 1024 x 1024 of D = 128; unit-norm descriptors,
half of side 0's rows with a planted partner; ratio threshold 0.8, mutual check on.  Per cell
  matched       one ``oetr_nn_match`` call through ``match_descriptors`` on device tensors (the joined form), captured
                into a HIP graph of CALLS back-to-back calls and replayed between device events;
  roof share    the FLOPs the call ISSUES (both directions, rows padded to the kernel's 64 x 128 tiles) per second, over
                the 157.3 TFLOP/s of gfx950's f32-input MFMA;
  (a) torch     the same matcher written in torch on the device, pair by pair as a caller has to run it today:
                ``einsum('bdn,bdm->bnm')``, ``topk(2)`` per row and per column, the ratio test, the mutual check.  Timed
                EAGERLY between device events on TORCH_PAIRS pairs and scaled to the cell's pairs;
  agreement     the share of rows on which (a) and the call give the same ``matches0`` on those pairs (torch sums in
                another order and leaves tied indices open: recorded, not asserted - tests/test_gpu_nn_match.py holds
                the call to its specification bit for bit).
All variants alternate over ROUNDS after a warm-up; medians.

    python tools/nn_match_probe.py [--out profiles/nn_match_probe.json] [--dry-run] [--scale S]

``--dry-run`` does everything up to the first device call - input generation (on the CPU, at the cell's shape with
two pairs), route (a) on CPU tensors, the FLOP counts, the JSON skeleton (printed, not written) - and needs no GPU.
``--scale`` divides the pair counts for a rehearsal; the record says what was run.

EXPECTED (recorded per cell and overall as met / missed, not gated): less device time than (a)."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402

CALLS, ROUNDS = 10, 9
CELLS = ((256, 2048, 256), (1024, 1024, 128))             # pairs, descriptors per side and pair, D
RATIO, MUTUAL = 0.8, True
ROOF_TFLOPS = 157.3                                       # f32-input MFMA, MI355X
QUERY_TILE, KEY_TILE = 64, 128                            # csrc/nn_match.hip: NN_QT, NN_KT
TORCH_PAIRS = 16
ASSEMBLE_1024_PAIRS_US = 48.9                             # profiles/match_assembly_probe.json: 1024 pairs x 2048


def make_descriptors(P, K, D, dev, seed):
    """Unit-norm rows; half of side 0's rows are a side-1 row of their pair plus noise of relative size 0.01 - 0.08."""
    g = torch.Generator(device=dev).manual_seed(seed)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)
    d1 = unit(torch.randn(P, K, D, device=dev, generator=g))
    d0 = unit(torch.randn(P, K, D, device=dev, generator=g))
    partner = torch.randint(0, K, (P, K // 2), device=dev, generator=g)
    noise = torch.randn(P, K // 2, D, device=dev, generator=g) / D ** 0.5
    noise *= 0.01 + 0.07 * torch.rand(P, K // 2, 1, device=dev, generator=g)
    d0[:, :K // 2] = unit(torch.gather(d1, 1, partner[..., None].expand(-1, -1, D)) + noise)
    return d0.reshape(P * K, D).contiguous(), d1.reshape(P * K, D).contiguous()


def torch_find_nn(sim, ratio_sq):
    """Nearest neighbour of every row of ``sim`` under the ratio test, as a caller writes it in torch."""
    best, index = sim.topk(2, dim=-1)
    dist = 2 * (1 - best)
    ok = dist[..., 0] <= ratio_sq * dist[..., 1]
    return torch.where(ok, index[..., 0], -1), torch.where(ok, (best[..., 0] + 1) / 2, 0.0)


def torch_route(pairs0, pairs1):
    """Route (a) on channels-first per-pair tensors ``[1,D,K]``: one similarity matrix, two ``topk`` per pair."""
    out = []
    for a, b in zip(pairs0, pairs1):
        sim = torch.einsum('bdn,bdm->bnm', a, b)
        m0, s0 = torch_find_nn(sim, RATIO ** 2)
        m1, _ = torch_find_nn(sim.transpose(1, 2), RATIO ** 2)
        back = torch.gather(m1, -1, m0.clamp(min=0))
        keep = (m0 > -1) & (back == torch.arange(m0.shape[-1], device=m0.device))
        out.append((torch.where(keep, m0, -1), s0))
    return out


def cell(dev, P, K, D, dry_run):
    pad = lambda n, t: -(-n // t) * t
    useful = 2 * 2.0 * K * K * D * P                      # both directions, 2 FLOP per multiply-add
    issued = 2 * 2.0 * pad(K, QUERY_TILE) * pad(K, KEY_TILE) * D * P
    rec = {'cell': f'{P} pairs x {K} x {K} descriptors, D = {D}', 'pairs': P, 'descriptors_per_side': K, 'D': D,
           'ratio_threshold': RATIO, 'do_mutual_check': MUTUAL, 'flop_useful': useful, 'flop_issued': issued}
    where = torch.device('cpu') if dry_run else dev
    d0, d1 = make_descriptors(2 if dry_run else P, K, D, where, seed=K + D)
    n = min(TORCH_PAIRS, 2 if dry_run else P)
    first0 = [d0[p * K:(p + 1) * K].t().contiguous()[None] for p in range(n)]        # the reference's layout [B,D,N]
    first1 = [d1[p * K:(p + 1) * K].t().contiguous()[None] for p in range(n)]
    theirs = torch_route(first0, first1)
    rec['torch_pairs_timed'] = n
    rec['torch_matched_share'] = float(torch.cat([m.flatten() for m, _ in theirs]).gt(-1).float().mean())
    if dry_run:
        return rec
    from imagematching_oetr_amd import match_counts, match_descriptors
    off = (torch.arange(P + 1, device=dev) * K).int()
    kw = dict(offsets0=off, offsets1=off, max_k0=K, max_k1=K, ratio_threshold=RATIO, do_mutual_check=MUTUAL)
    out = match_descriptors(d0, d1, **kw)
    counts = match_counts(out)
    assert (counts[:, :2] == K).all() and (counts[:, 3] <= counts[:, 2]).all()
    rec['matched_share'] = float(counts[:, 3].sum() / (P * K))
    mine = out['matches0'][:n * K].view(n, K)
    rec['torch_agreement_share'] = float(torch.stack([m[0] for m, _ in theirs]).eq(mine).float().mean())
    graph = graph_of(lambda: match_descriptors(d0, d1, **kw, out=out), CALLS)
    torch_route(first0, first1)                                                     # warm-up
    ms = {'matched': [], 'torch': []}
    for _ in range(ROUNDS):
        ms['matched'].append(timed(graph.replay) / CALLS)
        ms['torch'].append(timed(lambda: torch_route(first0, first1)) * P / n)
    for k in ms:
        rec[k + '_ms'] = stats(ms[k])
    med = lambda k: rec[k + '_ms']['median']
    rec['tflops_issued'] = issued / (med('matched') * 1e-3) / 1e12
    rec['tflops_useful'] = useful / (med('matched') * 1e-3) / 1e12
    rec['share_of_f32_mfma_roof'] = rec['tflops_issued'] / ROOF_TFLOPS
    rec['torch_over_matched'] = med('torch') / med('matched')
    rec['less_device_time_than_torch'] = med('matched') < med('torch')
    if P == 1024:
        rec['over_assemble_matches_of_1024_pairs'] = med('matched') * 1e3 / ASSEMBLE_1024_PAIRS_US
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'nn_match_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--scale', type=int, default=1)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('nn_match_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/nn_match_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__, 'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/nn_match_probe.py', 'imagematching_oetr_amd/csrc/nn_match.hip',
                                             'tests/nn_match_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'roof_tflops': ROOF_TFLOPS, 'scale': args.scale, 'cells': []}
    dev = None
    if not args.dry_run:
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
    for pairs, K, D in CELLS:
        c = cell(dev, max(1, pairs // args.scale), K, D, args.dry_run)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    if args.dry_run:
        print(json.dumps(rec, indent=1))
        print('dry run: stopped before the first device call; nothing written')
        return
    rec['expectations'] = {'less_device_time_than_torch_in_every_cell': all(c['less_device_time_than_torch']
                                                                            for c in rec['cells'])}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec['expectations']))


if __name__ == '__main__':
    main()
