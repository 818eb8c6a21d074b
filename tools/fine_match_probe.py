"""What refining dense matches to sub-pixel costs on the device (include/oetr_fine_match.h, csrc/fine_match.hip), in
one run.

Cells: 64 pairs x 60 x 80 coarse / 240 x 320 fine grids (the 480 x 640 crop at 1/8 and 1/2), and 256 pairs x 30 x 40 /
120 x 160; C = 128, W = 5, stride 4; 5/16 of side 0's tokens matched (1500 of 4800) to distinct tokens of side 1;
unit-variance Gaussian fine features.  Per cell
  checked     before anything is timed: the gathered windows of the first TORCH_PAIRS pairs EQUAL what ``unfold`` of the
              whole maps + index gives, and the head's output on the first CHECK_ROWS list rows equals the numpy
              specification (tests/fine_match_oracle.py) bit for bit;
  windows     one ``oetr_fine_windows`` call through ``fine_windows`` on device tensors (the joined form), captured into
              a HIP graph of CALLS back-to-back calls and replayed between device events;
  refine      one ``oetr_fine_refine`` call through ``refine_matches`` on the gathered windows, likewise;
  (a) copy_   a ``copy_`` of each entry's algorithmic bytes, likewise in a graph: the window bytes of both sides for the
              gather (it reads as many as it writes), ``(1 + W * W) * C * 4`` per match for the head;
  (b) torch   the same step in eager torch on the device, pair by pair as a caller has to run it today: ``unfold`` of
              both whole fine maps, the rearrangement to ``[L, W*W, C]`` and the index by ``nonzero`` of the matches;
              and ``einsum`` + ``softmax`` + expectation + std on the gathered windows.  Timed EAGERLY between device
              events on TORCH_PAIRS pairs and scaled to the cell's pairs;
  (c) NCHW    what a caller whose fine maps are ``[C, hf, wf]`` pays for the permuting copy to token rows, per call.
All variants alternate over ROUNDS after a warm-up; medians.

    python tools/fine_match_probe.py [--out profiles/fine_match_probe.json] [--dry-run] [--scale S]

``--dry-run`` does everything up to the first device call - input generation (on the CPU, two pairs of 8 x 10 coarse
grids at the cell's C), route (b) and the specification on them, the byte counts, the JSON skeleton (printed, not
written) - and needs no GPU.  ``--scale`` divides the pair counts for a rehearsal; the record says what was run.

EXPECTED (written before any measurement; recorded per cell as met / missed, not gated): (a) the gather
within 3x and the head within 2x of the ``copy_`` of their bytes; (b) each entry takes less device time than its
eager torch step."""
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
CELLS = ((64, 60, 80), (256, 30, 40))                     # pairs, coarse grid rows, coarse grid columns (both sides)
C, W, STRIDE, CELL = 128, 5, 4, 8
MATCHED_SHARE = 5 / 16                                    # 1500 of 4800
TORCH_PAIRS, CHECK_ROWS = 4, 256
COPY_RATIO_EXPECTED = {'windows': 3.0, 'refine': 2.0}


def make_inputs(P, h, w, dev, seed):
    """Fine maps as joined token rows ``[P * hf * wf, C]`` per side, and ``matches0`` ``[P * h * w]``."""
    g = torch.Generator(device=dev).manual_seed(seed)
    K, F = h * w, h * w * STRIDE * STRIDE
    fine0 = torch.randn(P * F, C, device=dev, generator=g)
    fine1 = torch.randn(P * F, C, device=dev, generator=g)
    n = int(K * MATCHED_SHARE)
    matches = torch.full((P, K), -1, dtype=torch.int32, device=dev)
    for p in range(P):
        rows = torch.randperm(K, device=dev, generator=g)[:n]
        matches[p, rows] = torch.randperm(K, device=dev, generator=g)[:n].int()
    return fine0, fine1, matches.reshape(-1), n


def torch_windows(fine0, fine1, matches, h, w):
    """Route (b), the gather, for ONE pair: ``fine*`` ``[hf * wf, C]`` token rows of one pair."""
    hf, wf = h * STRIDE, w * STRIDE
    out = []
    for fine in (fine0, fine1):
        m = fine.view(1, hf, wf, C).permute(0, 3, 1, 2)
        u = torch.nn.functional.unfold(m, kernel_size=(W, W), stride=STRIDE, padding=W // 2)
        out.append(u.view(C, W * W, -1).permute(2, 1, 0))            # [L, WW, C], a view
    i = torch.nonzero(matches > -1)[:, 0]                            # reads back
    return out[0][i], out[1][matches[i].long()], i


def torch_head(win0, win1, kp1_of_match, fine_cell):
    """Route (b), the head, on gathered windows ``[M, WW, C]``."""
    sim = torch.einsum('mc,mrc->mr', win0[:, W * W // 2], win1) / C ** 0.5
    heat = torch.softmax(sim, 1)
    lin = torch.linspace(-1, 1, W, device=win0.device)
    gx, gy = lin.repeat(W), lin.repeat_interleave(W)
    x, y = heat @ gx, heat @ gy
    var = torch.stack([heat @ gx ** 2 - x ** 2, heat @ gy ** 2 - y ** 2], -1)
    std = torch.sqrt(torch.clamp(var, min=1e-10)).sum(-1)
    xy = torch.stack([x, y], -1)
    return torch.cat([xy, std[:, None]], -1), kp1_of_match + xy * (W // 2) * fine_cell


def cell(dev, P, h, w, dry_run):
    import dual_softmax_oracle as dso
    import fine_match_oracle as fmo
    if dry_run:
        P, h, w = 2, 8, 10
    K, F, WW = h * w, h * w * STRIDE * STRIDE, W * W
    where = torch.device('cpu') if dry_run else dev
    fine0, fine1, matches, n = make_inputs(P, h, w, where, seed=K)
    M = P * n
    window_bytes = 2 * M * WW * C * 4
    head_bytes = M * (1 + WW) * C * 4
    rec = {'cell': f'{P} pairs x {h} x {w} coarse / {h * STRIDE} x {w * STRIDE} fine, C = {C}, W = {W}, {n} matches per pair',
           'pairs': P, 'grid': [h, w], 'C': C, 'W': W, 'stride': STRIDE, 'matches': M, 'window_bytes': window_bytes,
           'head_bytes': head_bytes, 'unfold_bytes_per_image': K * WW * C * 4}
    pairs = min(TORCH_PAIRS, P)
    kp = torch.from_numpy(np.tile(dso.keypoints(h, w, CELL), (P, 1))).to(where)
    theirs = [torch_windows(fine0[p * F:(p + 1) * F], fine1[p * F:(p + 1) * F], matches[p * K:(p + 1) * K], h, w)
              for p in range(pairs)]
    t0 = torch.cat([a for a, _, _ in theirs])
    t1 = torch.cat([b for _, b, _ in theirs])
    kp1_of_match = torch.cat([kp[p * K:(p + 1) * K][matches[p * K:(p + 1) * K][i].long()] for p, (_, _, i) in enumerate(theirs)])
    their_expec, _ = torch_head(t0, t1, kp1_of_match, CELL / STRIDE)
    rows = min(CHECK_ROWS, len(t0))
    want_expec, _ = fmo.head(t0[:rows].cpu().numpy(), t1[:rows].cpu().numpy(), W)
    rec['torch_pairs_timed'] = pairs
    rec['specification_vs_torch_expec_max_abs'] = float(np.abs(want_expec - their_expec[:rows].cpu().numpy()).max())
    if dry_run:
        return rec
    from imagematching_oetr_amd import fine_match_counts, fine_windows, refine_matches
    off = (torch.arange(P + 1, device=dev) * K).int()
    foff = (torch.arange(P + 1, device=dev) * F).int()
    grids = torch.tensor([[h, w]], dtype=torch.int32, device=dev).expand(P, 2).contiguous()
    fgrids = (grids * STRIDE).contiguous()
    coarse = dict(matches0=matches, keypoints0=kp, keypoints1=kp, _inputs=(None, None, off, off, grids, grids))
    kw = dict(fine_offsets0=foff, fine_offsets1=foff, fine_grids0=fgrids, fine_grids1=fgrids, window=W, stride=STRIDE,
              max_matches=M, max_k0=K)
    win = fine_windows(coarse, fine0, fine1, **kw)
    fine = refine_matches(win, coarse, fine_cell=CELL / STRIDE)
    counts = fine_match_counts(fine)
    assert (counts[:, 0] == n).all() and (counts[:, 1] == n).all() and (counts[:, 2] == 0).all()
    m = len(t0)                                                      # the first pairs' windows: EQUAL to unfold + index
    assert torch.equal(win['win0'][:m], t0) and torch.equal(win['win1'][:m], t1)
    assert fine['expec'][:rows].cpu().numpy().tobytes() == want_expec.tobytes()  # bit for bit, before anything is timed
    rec['rows_checked_bit_for_bit'] = rows
    rec['windows_checked_equal'] = m
    src_w = torch.empty(window_bytes // 4, device=dev)
    dst_w = torch.empty_like(src_w)
    src_h = torch.empty(head_bytes // 4, device=dev)
    dst_h = torch.empty_like(src_h)
    # (c) the first pairs' maps as an NCHW caller holds them
    nchw = [f[:pairs * F].view(pairs, h * STRIDE, w * STRIDE, C).permute(0, 3, 1, 2).contiguous() for f in (fine0, fine1)]
    graphs = {'windows': graph_of(lambda: fine_windows(coarse, fine0, fine1, **kw, out=win), CALLS),
              'refine': graph_of(lambda: refine_matches(win, coarse, fine_cell=CELL / STRIDE, out=fine), CALLS),
              'copy_windows': graph_of(lambda: dst_w.copy_(src_w), CALLS),
              'copy_refine': graph_of(lambda: dst_h.copy_(src_h), CALLS)}

    def eager_windows():
        for p in range(pairs):
            torch_windows(fine0[p * F:(p + 1) * F], fine1[p * F:(p + 1) * F], matches[p * K:(p + 1) * K], h, w)

    def permute_nchw():
        for f in nchw:
            f.permute(0, 2, 3, 1).contiguous()

    eager_windows(), torch_head(t0, t1, kp1_of_match, CELL / STRIDE), permute_nchw()      # warm-up
    ms = {k: [] for k in list(graphs) + ['torch_windows', 'torch_refine', 'nchw_permute']}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            ms[k].append(timed(g.replay) / CALLS)
        ms['torch_windows'].append(timed(eager_windows) * P / pairs)
        ms['torch_refine'].append(timed(lambda: torch_head(t0, t1, kp1_of_match, CELL / STRIDE)) * M / len(t0))
        ms['nchw_permute'].append(timed(permute_nchw) * P / pairs)
    for k in ms:
        rec[k + '_ms'] = stats(ms[k])
    med = lambda k: rec[k + '_ms']['median']
    for k in ('windows', 'refine'):
        rec[k + '_over_copy'] = med(k) / med('copy_' + k)
        rec['torch_over_' + k] = med('torch_' + k) / med(k)
        rec['expectation_a_' + k + '_within_%gx_of_copy' % COPY_RATIO_EXPECTED[k]] = \
            'met' if rec[k + '_over_copy'] <= COPY_RATIO_EXPECTED[k] else 'missed'
        rec['expectation_b_' + k + '_less_device_time_than_torch'] = 'met' if med(k) < med('torch_' + k) else 'missed'
    rec['windows_gbytes_per_s'] = 2 * window_bytes / (med('windows') * 1e-3) / 1e9      # read + written
    rec['refine_gbytes_per_s'] = head_bytes / (med('refine') * 1e-3) / 1e9
    rec['nchw_permute_over_windows'] = med('nchw_permute') / med('windows')
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'fine_match_probe.json'))
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--scale', type=int, default=1)
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit('fine_match_probe.py measures on the GPU: none visible (--dry-run rehearses the host side)')
    torch.set_grad_enabled(False)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/fine_match_probe.py', 'dry_run': args.dry_run, 'torch': torch.__version__,
           'numpy': np.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/fine_match_probe.py', 'imagematching_oetr_amd/csrc/fine_match.hip',
                                             'imagematching_oetr_amd/csrc/fine_match_math.h',
                                             'tests/fine_match_oracle.py')},
           'calls_per_graph': CALLS, 'rounds': ROUNDS, 'scale': args.scale, 'cells': []}
    dev = None
    if not args.dry_run:
        dev = torch.device('cuda', 0)
        rec['device'] = torch.cuda.get_device_name(dev)
    for pairs, h, w in CELLS:
        c = cell(dev, max(TORCH_PAIRS, pairs // args.scale), h, w, args.dry_run)
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
