"""Whole-workgroup cycles of k_encoder64 by workgroup class - ragged (one-row-tile body) against full (two-row-tile
body) - at 8 pairs 640x640 (library built with -DOETR_PHASE_TIMING; profiles/shared_tail_phases.txt).
usage: phase_timing_rows.py [tail_share]      tail_share: -1 automatic (the default), 0 off (oetr_set_tail_share)

Stamps 0..8 (phase B) are those of the forward's last launch (<B, decoder prep>), stamps 9..12 (phase A behind LN-A) those
of the last <B,A> launch before it: a block index maps to the same tile in every launch, so both belong to the same
workgroup; the LN-A phase (stamp 8 -> 9) straddles two launches and is left out."""
import ctypes, os, sys
from pathlib import Path
REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
os.environ['OETR_HIP_LIB'] = str(REPO / 'tools/variants/timing/liboetr_hip.so')
import numpy as np, torch
import imagematching_oetr_amd as pkg
torch.set_grad_enabled(False)
dev = torch.device('cuda', 0)
model = pkg.OETR(pkg.get_cfg_defaults().OETR).eval()
n = 8
torch.manual_seed(0)
f1 = (torch.rand(n, 256, 20, 20) - 0.5).to(dev); f2 = (torch.rand(n, 256, 20, 20) - 0.5).to(dev)
pos = model.pos_encoding(f1.cpu()).contiguous().to(dev)
eng = pkg.HotPathEngine(model.hot_path_state(), device=dev, precision='f32_split_f16', enc_tile=64)
eng.set_tail_share(int(sys.argv[1]) if len(sys.argv) > 1 else -1)
eng.forward(f1, f2, pos, pos, (640, 640), (640, 640))
nwg = eng.debug_encoder_grid()     # 112 = 8 x 14 tiles, or 104 with the two ragged tails of a pair in one workgroup
per = nwg // n


def remap(bid, nw):                # common.h: xcd_remap
    q, r, xcd, idx = nw >> 3, nw & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


rem = np.array([remap(b, nwg) for b in range(nwg)]) % per
ragged = (rem == 6) | (rem == 13) if per == 14 else rem == 12     # tiles 6 and 13 of 14, or the shared tile 12 of 13
lib = eng.lib
lib.oetr_debug_read_tbuf.argtypes = [ctypes.c_void_p, ctypes.c_int]
res = []
for rep in range(12):
    for _ in range(2):
        eng.forward(f1, f2, pos, pos, (640, 640), (640, 640), stages=True, enc_layers=3)
    eng.forward(f1, f2, pos, pos, (640, 640), (640, 640), stages=True, enc_layers=8)
    torch.cuda.synchronize()
    buf = (ctypes.c_longlong * (16 * nwg))()
    assert lib.oetr_debug_read_tbuf(buf, nwg) == 0
    t = np.frombuffer(buf, dtype=np.int64).reshape(nwg, 16)[:, :13].astype(np.float64)
    b, a, pro = t[:, 8] - t[:, 0], t[:, 12] - t[:, 9], t[:, 1] - t[:, 0]
    res.append((b[ragged].mean(), b[~ragged].mean(), a[ragged].mean(), a[~ragged].mean(), pro[ragged].mean(), pro[~ragged].mean()))
med = np.median(np.array(res), axis=0)
print(f'workgroups {nwg}, ragged {int(ragged.sum())}; median over 12 forwards of the per-class mean, s_memtime ticks:')
print(f'  phase B (stamps 0..8):   ragged {med[0]:8.0f}  full {med[1]:8.0f}  ratio {med[0] / med[1]:.3f}')
print(f'  phase A (stamps 9..12):  ragged {med[2]:8.0f}  full {med[3]:8.0f}  ratio {med[2] / med[3]:.3f}')
print(f'  prologue (stamps 0..1):  ragged {med[4]:8.0f}  full {med[5]:8.0f}')
cr, cf = med[0] + med[2], med[1] + med[3]
print(f'  whole workgroup (B + A): c_r {cr:.0f}  c_f {cf:.0f}  c_r / c_f {cr / cf:.3f}')
if per == 14:
    print(f'  one ragged workgroup per pair fewer would save 8 c_r / (96 c_f + 16 c_r) = {8 * cr / (96 * cf + 16 * cr) * 100:.2f} % of the encoder\'s CU time')
