"""What the feature bank costs and buys (include/oetr_bank.h, imagematching_oetr_amd/bank.py), in one run:

1. k_bank_gather beside a ``Tensor.copy_`` of the same number of bytes - the yardstick: the same bytes moved
   with no index.  Each variant is captured into a HIP graph of CALLS back-to-back launches (the host's enqueue
   cost is not part of the number) and replayed between device events; the variants alternate over ROUNDS.
2. pairs/s of ``forward_pairs_indexed`` against ``forward_pairs`` on the SAME pair list over 64 images of
   640 x 640 (already on the device), at 1, 4 and 16 pairs per image, ``hip_streams`` 1 and 3, device events
   around synchronised regions, every cell alternated over ROUNDS after a warm-up pass through all of them.

    python tools/bank_probe.py [--out profiles/bank_probe.json]

One JSON record.  Exit status 1 when the ordinal chain indexed(reuse 16) > indexed(reuse 4) > forward_pairs(reuse 4)
fails (it follows from the trunk being 95 % of a forward_dummy call).  The gather is EXPECTED not to be slower than
copy_ beyond the spread the run itself shows; that is recorded per shape (``gather_not_slower_than_copy``), not gated."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import torch  # noqa: E402
from probe_common import graph_of, stats, timed  # noqa: E402
import imagematching_oetr_amd as pkg  # noqa: E402

CALLS, ROUNDS = 100, 9          # gather / copy: launches per graph, alternated rounds
E2E_ROUNDS = 3
IMAGES, SIZE = 64, 640


def gather_vs_copy(eng, dev, n, hf, wf, bank_images=64):
    L = hf * wf
    gen = torch.Generator().manual_seed(n)
    bank = torch.randn(bank_images, L, 256, generator=gen).to(dev)
    i1 = torch.randint(bank_images, (n,), generator=gen).to(dev, torch.int32)
    i2 = torch.randint(bank_images, (n,), generator=gen).to(dev, torch.int32)
    tokens = torch.empty(2 * n * L, 256, device=dev)
    t1, t2 = tokens[:n * L], tokens[n * L:]
    src = torch.randn(2 * n * L, 256, generator=gen).to(dev)
    dst = torch.empty_like(src)
    eng.bank_gather(bank, i1, bank, i2, t1, t2)
    assert torch.equal(t1, bank[i1.long()].reshape(-1, 256)) and torch.equal(t2, bank[i2.long()].reshape(-1, 256))
    graphs = {'gather': graph_of(lambda: eng.bank_gather(bank, i1, bank, i2, t1, t2), CALLS),
              'copy': graph_of(lambda: dst.copy_(src), CALLS)}
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(timed(g.replay) * 1e3 / CALLS)
    moved = 2 * tokens.numel() * 4           # read + written
    out = {'pairs': n, 'grid': [hf, wf], 'bytes_read_plus_written': moved, 'bank_images': bank_images}
    for k in us:
        out[k + '_us'] = stats(us[k])
        out[k + '_TBps'] = moved / (out[k + '_us']['median'] * 1e-6) / 1e12
    spread = max(out[k + '_us']['max'] - out[k + '_us']['min'] for k in us)
    out['spread_us'] = spread
    out['gather_not_slower_than_copy'] = out['gather_us']['median'] <= out['copy_us']['median'] + spread
    return out


def pair_list(reuse):
    if reuse == 1:
        return [(2 * i, 2 * i + 1) for i in range(IMAGES // 2)]
    return [(i, (i + d) % IMAGES) for d in range(1, reuse // 2 + 1) for i in range(IMAGES)]


def end_to_end(model, dev):
    gen = torch.Generator().manual_seed(3)
    images = [torch.rand(1, SIZE, SIZE, 3, generator=gen).to(dev) for _ in range(IMAGES)]
    lists = {r: pair_list(r) for r in (1, 4, 16)}
    variants = {
        'forward_pairs': lambda idx: pkg.forward_pairs(model, [(images[i], images[j]) for i, j in idx], max_batch=8),
        'forward_pairs_indexed': lambda idx: pkg.forward_pairs_indexed(model, images, idx, max_batch=8, trunk_batch=16)}
    cells = [(s, r, v) for s in (1, 3) for r in (1, 4, 16) for v in variants]
    ms = {c: [] for c in cells}
    for rnd in range(E2E_ROUNDS + 1):        # round 0: warm-up (MIOpen's choices, workspaces, side streams)
        for s, r, v in cells:
            model.hip_streams = s
            t = timed(lambda: variants[v](lists[r]))
            if rnd:
                ms[(s, r, v)].append(t)
    # the two routes agree (two trunk runs: the project's 0.05 px)
    model.hip_streams = 1
    a, b = variants['forward_pairs'](lists[4]), variants['forward_pairs_indexed'](lists[4])
    err = max(float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()))
    out = {'images': IMAGES, 'image_size': [SIZE, SIZE], 'max_batch': 8, 'trunk_batch': 16, 'rounds': E2E_ROUNDS,
           'max_box_difference_px_reuse4': err, 'cells': []}
    rate = {}
    for s, r, v in cells:
        st = stats(ms[(s, r, v)])
        rate[(s, r, v)] = len(lists[r]) / (st['median'] * 1e-3)
        out['cells'].append({'hip_streams': s, 'pairs_per_image': r, 'pairs': len(lists[r]), 'variant': v,
                             'ms': st, 'pairs_per_s': rate[(s, r, v)]})
    out['ordinal'] = {}
    for s in (1, 3):
        i16, i4, p4 = (rate[(s, 16, 'forward_pairs_indexed')], rate[(s, 4, 'forward_pairs_indexed')],
                       rate[(s, 4, 'forward_pairs')])
        out['ordinal'][f'hip_streams_{s}'] = {'indexed_reuse16_gt_indexed_reuse4': i16 > i4,
                                              'indexed_reuse4_gt_forward_pairs_reuse4': i4 > p4}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'bank_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bank_probe.py measures on the GPU: none visible')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = pkg.OETR(pkg.get_cfg_defaults().OETR).eval().to(dev)
    sha = lambda p: hashlib.sha256((REPO / p).read_bytes()).hexdigest()[:16]
    rec = {'tool': 'tools/bank_probe.py', 'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__,
           'sha256_16': {p: sha(p) for p in ('tools/bank_probe.py', 'imagematching_oetr_amd/csrc/bank.hip')},
           'gather_vs_copy': {'calls_per_graph': CALLS, 'rounds': ROUNDS,
                              'shapes': [gather_vs_copy(model.engine(), dev, 8, 20, 20),
                                         gather_vs_copy(model.engine(), dev, 32, 32, 32)]},
           'end_to_end': end_to_end(model, dev)}
    ok = all(all(v.values()) for v in rec['end_to_end']['ordinal'].values())
    rec['ordinal_conditions_hold'] = ok
    rec['gather_expectation_met'] = all(s['gather_not_slower_than_copy'] for s in rec['gather_vs_copy']['shapes'])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(rec))
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
