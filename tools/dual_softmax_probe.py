"""What matching dense feature grids by a dual softmax costs on the device (include/oetr_dual_softmax.h,
csrc/dual_softmax.hip), in one run.

Cells: 64 pairs x 4800 x 4800 tokens of D = 256 (the 480 x 640 crop at 1/8: 60 x 80 grids), and 256 pairs x 1200 x 1200
of D = 256 (30 x 40 grids); unit-variance Gaussian tokens, half of side 0's tokens with a planted partner; temperature
0.1, threshold 0.2, border 2.  Per cell
  checked       CHECK_PAIRS pairs of the cell's call compared with the numpy specification (tests/dual_softmax_oracle.py)
                bit for bit, every output, before anything is timed - in the cells of at most MAX_CHECKED_TOKENS tokens
                per side (the specification takes minutes per pair beyond that);
  dense         one ``oetr_dual_softmax_match`` call through ``match_dense`` on device tensors (the joined form), captured
                into a HIP graph of CALLS back-to-back calls and replayed between device events;
  per sweep     the issued FLOPs of one sweep (both directions, rows padded to the kernel's 64 x 128 tiles) are a third
                of the call's; the call's time over three is recorded as the time per sweep (the launches of one call
                are not timed apart: that needs a profiler run of its own);
  roof share    the FLOPs the call ISSUES per second, over the 157.3 TFLOP/s of gfx950's f32-input MFMA, the roof
                tools/nn_match_probe.py uses;
  (a) torch     the same head in torch float32 on the device, pair by pair as a caller has to run it today: ``einsum``,
                ``softmax(dim=1) * softmax(dim=2)``, threshold, border mask, the two ``== max`` tests.  Timed EAGERLY
                between device events on TORCH_PAIRS pairs and scaled to the cell's pairs;
  (b) nn        ``oetr_nn_match`` (``match_descriptors``, mutual check on, no thresholds) on the SAME rows in the same
                run, likewise in a graph: one sweep where the dual softmax does three, so 3x its time is the floor.
All variants alternate over ROUNDS after a warm-up; medians.

    python tools/dual_softmax_probe.py [--out profiles/dual_softmax_probe.json] [--dry-run] [--scale S]

``--dry-run`` does everything up to the first device call - input generation (on the CPU, two pairs of 8 x 10 grids at
the cell's D), route (a) and the specification on them, the FLOP counts, the JSON skeleton (printed, not written) -
and needs no GPU.  ``--scale`` divides the pair counts for a rehearsal; the record says what was run.

EXPECTED (written before any measurement; recorded per cell as met / missed, not gated): (a) less device
time than torch; (b) between 3x and 4.5x the time of ``oetr_nn_match`` on the same rows."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402

CALLS, ROUNDS = 10, 9
CELLS = ((64, 60, 80, 256), (256, 30, 40, 256))           # pairs, grid rows, grid columns (both sides), D
TEMPERATURE, THRESHOLD, BORDER, CELL = 0.1, 0.2, 2, 8
ROOF_TFLOPS = 157.3                                       # f32-input MFMA, MI355X
QUERY_TILE, KEY_TILE = 64, 128                            # csrc/dual_softmax.hip: DS_QT, DS_KT
SWEEPS = 3
TORCH_PAIRS, CHECK_PAIRS = 4, 4
# the numpy specification walks D one fmaf at a time over the whole matrix: minutes per pair at 4800 x 4800, so the
# large cell is timed without the comparison (tests/test_gpu_dual_softmax.py holds the kernels to it on every tile edge)
MAX_CHECKED_TOKENS = 1200
NN_RATIO_EXPECTED = (3.0, 4.5)


def make_tokens(P, K, D, dev, seed):
    """Unit-variance Gaussian rows; half of side 0's rows are a side-1 row of their pair plus noise of relative size 0.05 - 0.3."""
    g = torch.Generator(device=dev).manual_seed(seed)
    f1 = torch.randn(P, K, D, device=dev, generator=g)
    f0 = torch.randn(P, K, D, device=dev, generator=g)
    partner = torch.stack([torch.randperm(K, device=dev, generator=g)[:K // 2] for _ in range(P)])
    noise = torch.randn(P, K // 2, D, device=dev, generator=g) * (0.05 + 0.25 * torch.rand(P, K // 2, 1, device=dev, generator=g))
    f0[:, :K // 2] = torch.gather(f1, 1, partner[..., None].expand(-1, -1, D)) + noise
    return f0.reshape(P * K, D).contiguous(), f1.reshape(P * K, D).contiguous()


def torch_route(pairs0, pairs1, h, w):
    """Route (a) on per-pair token rows ``[1,K,D]``: the published head as a caller writes it in torch."""
    out = []
    for a, b in zip(pairs0, pairs1):
        sim = torch.einsum('nld,nsd->nls', a, b) / (a.shape[-1] * TEMPERATURE)
        conf = torch.softmax(sim, 1) * torch.softmax(sim, 2)
        mask = conf > THRESHOLD
        grid = mask.view(1, h, w, h, w)
        grid[:, :BORDER] = grid[:, -BORDER:] = grid[:, :, :BORDER] = grid[:, :, -BORDER:] = False
        grid[:, :, :, :BORDER] = grid[:, :, :, -BORDER:] = grid[:, :, :, :, :BORDER] = grid[:, :, :, :, -BORDER:] = False
        mask = mask * (conf == conf.max(dim=2, keepdim=True)[0]) * (conf == conf.max(dim=1, keepdim=True)[0])
        value, index = mask.max(dim=2)
        out.append((torch.where(value, index, -1), conf.max(dim=2)[0]))
    return out


def cell(dev, P, h, w, D, dry_run):
    import dual_softmax_oracle as dso
    import nn_match_oracle as nmo
    if dry_run:
        P, h, w = 2, 8, 10
    K = h * w
    pad = lambda n, t: -(-n // t) * t
    useful = SWEEPS * 2 * 2.0 * K * K * D * P                # three sweeps, both directions, 2 FLOP per multiply-add
    issued = SWEEPS * 2 * 2.0 * pad(K, QUERY_TILE) * pad(K, KEY_TILE) * D * P
    rec = {'cell': f'{P} pairs x {K} x {K} tokens ({h} x {w} grids), D = {D}', 'pairs': P, 'grid': [h, w], 'D': D,
           'temperature': TEMPERATURE, 'threshold': THRESHOLD, 'border_rm': BORDER, 'flop_useful': useful,
           'flop_issued': issued}
    where = torch.device('cpu') if dry_run else dev
    f0, f1 = make_tokens(P, K, D, where, seed=K + D)
    n = min(TORCH_PAIRS, P)
    first0 = [f0[p * K:(p + 1) * K][None] for p in range(n)]
    first1 = [f1[p * K:(p + 1) * K][None] for p in range(n)]
    theirs = torch_route(first0, first1, h, w)
    rec['torch_pairs_timed'] = n
    rec['torch_matched_share'] = float(torch.cat([m.flatten() for m, _ in theirs]).gt(-1).float().mean())
    scale = dso.scale_of(D, TEMPERATURE)
    wants = []
    for p in range(min(CHECK_PAIRS, P) if K <= MAX_CHECKED_TOKENS else 0):       # the specification of the checked pairs
        A, B = f0[p * K:(p + 1) * K].cpu().numpy(), f1[p * K:(p + 1) * K].cpu().numpy()
        wants.append(dso.match_t((nmo.similarity(A, B) * scale).astype(np.float32), (h, w), (h, w), THRESHOLD, BORDER))
    rec['specification_matched_share'] = float(np.mean([(x['matches0'] > -1).mean() for x in wants])) if wants else None
    if dry_run:
        return rec
    from imagematching_oetr_amd import dense_match_counts, match_counts, match_dense, match_descriptors
    off = (torch.arange(P + 1, device=dev) * K).int()
    grids = torch.tensor([[h, w]], dtype=torch.int32, device=dev).expand(P, 2).contiguous()
    kw = dict(offsets0=off, offsets1=off, grids0=grids, grids1=grids, max_k0=K, max_k1=K, temperature=TEMPERATURE,
              threshold=THRESHOLD, border_rm=BORDER, cell=CELL)
    out = match_dense(f0, f1, **kw)
    counts = dense_match_counts(out)
    assert (counts[:, :2] == K).all() and (counts[:, 3] <= counts[:, 2]).all()
    for p, want in enumerate(wants):                                             # bit for bit, before anything is timed
        rows = slice(p * K, (p + 1) * K)
        for key in ('matches0', 'matching_scores0', 'matches1'):
            assert out[key][rows].cpu().numpy().tobytes() == want[key].tobytes(), (p, key)
        assert counts[p].tolist() == want['counts'].tolist(), p
    rec['pairs_checked_bit_for_bit'] = len(wants)
    rec['matched_share'] = float(counts[:, 3].sum() / (P * K))
    mine = out['matches0'][:n * K].view(n, K)
    rec['torch_agreement_share'] = float(torch.stack([m[0] for m, _ in theirs]).eq(mine).float().mean())
    nn_kw = dict(offsets0=off, offsets1=off, max_k0=K, max_k1=K, do_mutual_check=True)
    nn_out = match_descriptors(f0, f1, **nn_kw)
    assert (match_counts(nn_out)[:, :2] == K).all()
    dense = graph_of(lambda: match_dense(f0, f1, **kw, out=out), CALLS)
    nn = graph_of(lambda: match_descriptors(f0, f1, **nn_kw, out=nn_out), CALLS)
    torch_route(first0, first1, h, w)                                            # warm-up
    ms = {'dense': [], 'nn': [], 'torch': []}
    for _ in range(ROUNDS):
        ms['dense'].append(timed(dense.replay) / CALLS)
        ms['nn'].append(timed(nn.replay) / CALLS)
        ms['torch'].append(timed(lambda: torch_route(first0, first1, h, w)) * P / n)
    for k in ms:
        rec[k + '_ms'] = stats(ms[k])
    med = lambda k: rec[k + '_ms']['median']
    rec['per_sweep_ms'] = med('dense') / SWEEPS
    rec['tflops_issued'] = issued / (med('dense') * 1e-3) / 1e12
    rec['tflops_useful'] = useful / (med('dense') * 1e-3) / 1e12
    rec['share_of_f32_mfma_roof'] = rec['tflops_issued'] / ROOF_TFLOPS
    rec['torch_over_dense'] = med('torch') / med('dense')
    rec['dense_over_nn'] = med('dense') / med('nn')
    rec['expectation_a_less_device_time_than_torch'] = 'met' if med('dense') < med('torch') else 'missed'
    lo, hi = NN_RATIO_EXPECTED
    rec['expectation_b_3x_to_4p5x_nn_match'] = 'met' if lo <= rec['dense_over_nn'] <= hi else 'missed'
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'dual_softmax_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--scale', type=int, default=1)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('dual_softmax_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/dual_softmax_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__,
           'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/dual_softmax_probe.py', 'imagematching_oetr_amd/csrc/dual_softmax.hip',
                                             'imagematching_oetr_amd/csrc/dual_softmax_math.h',
                                             'imagematching_oetr_amd/csrc/nn_match.hip', 'tests/dual_softmax_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'roof_tflops': ROOF_TFLOPS, 'scale': args.scale, 'cells': []}
    dev = None
    if not args.dry_run:
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
    for pairs, h, w, D in CELLS:
        c = cell(dev, max(CHECK_PAIRS, pairs // args.scale), h, w, D, args.dry_run)
        rec['cells'].append(c)
        print(json.dumps(c), flush=True)
    if args.dry_run:
        print(json.dumps(rec, indent=1))
        print('dry run: stopped before the first device call; nothing written')
        return
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
