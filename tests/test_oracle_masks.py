"""forward_dummy's optional masks (reference src/model.py:229; LinearAttention q_mask / kv_mask,
linear_attention.py:37-41; the decoder's memory_mask, transformer.py:361-381; the heat map's
masked_fill, model.py:166-171): the oracle against vectors produced by the imported reference
(oracle/gen_golden.py: gen_attention_masked, MASK_CASES).  CPU only."""
import glob
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import oetr_oracle as orc
from tests.test_oracle_golden import _close, _sub, load_hot_case

torch.set_grad_enabled(False)
MASKED = sorted(glob.glob(str(Path(__file__).parent / 'golden' / 'hotmask_*.npz')))


def load_masks(g):
    n = int(g['n'])
    m1 = orc.make_masks(int(g['mask_seed']), n, *g['grid1'], kind=str(g['mask_kind']))
    m2 = orc.make_masks(int(g['mask_seed']) + 100, n, *g['grid2'], kind=str(g['mask_kind']))
    # 0/1 kinds are stored as uint8, the fractional patterns as float32: compared exactly either way
    for m, stored in ((m1, g['mask1']), (m2, g['mask2'])):
        assert stored.dtype in (np.uint8, np.float32), stored.dtype
        assert np.array_equal(m.numpy().astype(stored.dtype), stored), 'seeded masks differ'
        assert np.array_equal(m.numpy(), stored.astype(np.float32))
    assert 0 < m1.mean() < 1 and 0 < m2.mean() < 1
    return m1, m2


def test_masked_linear_attention_matches_reference(golden_dir):
    g = np.load(golden_dir / 'attention_masked.npz')
    for (L, S) in g['cases']:
        tag = f'L{L}_S{S}'
        gen = torch.Generator().manual_seed(int(g[tag + '_seed']))
        q = (torch.rand(2, L, 8, 32, generator=gen) - 0.5) * 4
        k = (torch.rand(2, S, 8, 32, generator=gen) - 0.5) * 4
        v = (torch.rand(2, S, 8, 32, generator=gen) - 0.5) * 2
        qm = (torch.rand(2, L, generator=gen) >= 0.25).float()
        km = (torch.rand(2, S, generator=gen) >= 0.25).float()
        km[0] = 1.0
        fps = np.stack([orc.checksum(t) for t in (q, k, v, qm, km)])
        assert np.array_equal(fps, g[tag + '_in_fp']), 'seeded inputs differ'
        out = orc.linear_attention(q, k, v, q_mask=qm, kv_mask=km).reshape(2, L, 256)
        _close(_sub(out, g[tag + '_step']), g[tag + '_lin'], 1e-6, 1e-6, tag)
        assert (out[qm == 0] == 0).all()          # a masked query's message is exactly zero


@pytest.mark.parametrize('path', MASKED, ids=lambda p: p.split('hotmask_')[-1][:-4])
def test_masked_hot_path_matches_reference(path):
    g, w, f1, f2 = load_hot_case(path)
    m1, m2 = load_masks(g)
    (hf1, wf1), (hf2, wf2) = g['grid1'], g['grid2']
    p1, p2 = orc.position_table(hf1, wf1), orc.position_table(hf2, wf2)
    x1, x2, t1, t2 = orc.tokens(f1), orc.tokens(f2), orc.tokens(p1), orc.tokens(p2)
    for li in (0, 1):
        y1, y2 = orc.encoder_stack(x1, x2, t1, t2, w, n_layers=li + 1, mask1=m1.flatten(1),
                                   mask2=m2.flatten(1))
        _close(_sub(y1, g[f'enc{li}_x1_step']), g[f'enc{li}_x1'], 2e-5, 1e-5, f'enc{li} x1')
        _close(_sub(y2, g[f'enc{li}_x2_step']), g[f'enc{li}_x2'], 2e-5, 1e-5, f'enc{li} x2')
    st = orc.hot_path(f1, f2, w, tuple(g['img1']), tuple(g['img2']), return_stages=True,
                      mask1=m1, mask2=m2)
    plain = orc.hot_path(f1, f2, w, tuple(g['img1']), tuple(g['img2']), return_stages=True)
    for s, m in (('1', m1), ('2', m2)):
        _close(_sub(st['memory' + s], g[f'memory{s}_step']), g['memory' + s], 5e-5, 1e-5, 'memory' + s)
        _close(st['hs' + s].numpy(), g['hs' + s], 1e-4, 1e-5, 'hs' + s)
        _close(st['logits' + s].numpy(), g['logits' + s], 2e-3, 1e-4, 'logits' + s)
        assert (st['logits' + s][m.flatten(1) == 0] == orc.MASK_FILL).all()
        _close(st['cxy' + s].numpy(), g['cxy' + s], 2e-2, 0, 'cxy' + s)
        _close(st['tlbr' + s].numpy(), g['tlbr' + s], 1e-5, 0, 'tlbr' + s)
        _close(st['box' + s].numpy(), g['box' + s], 3e-2, 0, 'box' + s)
        iou = orc.bbox_iou_aligned(st['box' + s], torch.from_numpy(g['box' + s]))
        assert (iou >= 1 - 1e-3).all(), iou
        # the masks matter: the unmasked forward of the same inputs is somewhere else
        assert (st['hs' + s] - plain['hs' + s]).abs().max() > 1e-3



WEIGHTED = Path(__file__).parent / 'golden' / 'hotmask_s10_7x9_5x13_sharp.npz'


def _kv_mask_once(q, k, v, eps=orc.ATTN_EPS, q_mask=None, kv_mask=None):
    """linear_attention with V left unmasked: the state would carry m instead of m^2."""
    S = v.shape[1]
    fq = (torch.nn.functional.elu(q) + 1) * (1 if q_mask is None else q_mask[:, :, None, None])
    fk = (torch.nn.functional.elu(k) + 1) * (1 if kv_mask is None else kv_mask[:, :, None, None])
    kv = torch.einsum('nshd,nshv->nhdv', fk, v / S)
    z = 1 / (torch.einsum('nlhd,nhd->nlh', fq, fk.sum(dim=1)) + eps)
    return (torch.einsum('nlhd,nhdv,nlh->nlhv', fq, kv, z) * S).contiguous()


def test_oracle_reproduces_the_fractional_mask_golden(monkeypatch):
    """hotmask_s10 holds float32 masks that are not 0/1 (weights in (0, 1], 1.5, 1e-6; a cleared
    32-row tile; a lone last token): it pins the reference's own mask semantics - phi(K) AND V
    multiplied by the mask (linear_attention.py:37-41), so the state carries m^2 and the key sum m -
    not our restatement of them.  The fp32 oracle reproduces it; the oracle with m in the state does not."""
    g, w, f1, f2 = load_hot_case(str(WEIGHTED))
    m1, m2 = load_masks(g)
    assert g['mask1'].dtype == np.float32 and g['mask2'].dtype == np.float32
    for m in (m1[0], m2[0]):
        assert ((m > 0) & (m < 1)).any() and (m == 1.5).any() and (m == np.float32(1e-6)).any() and (m == 0).any()
    im1, im2 = tuple(g['img1']), tuple(g['img2'])
    st = orc.hot_path(f1, f2, w, im1, im2, return_stages=True, mask1=m1, mask2=m2)
    for s, m in (('1', m1), ('2', m2)):
        _close(_sub(st['memory' + s], g[f'memory{s}_step']), g['memory' + s], 5e-5, 1e-5, 'memory' + s)
        _close(st['hs' + s].numpy(), g['hs' + s], 1e-4, 1e-5, 'hs' + s)
        _close(st['logits' + s].numpy(), g['logits' + s], 2e-3, 1e-4, 'logits' + s)
        _close(st['cxy' + s].numpy(), g['cxy' + s], 2e-2, 0, 'cxy' + s)
        _close(st['box' + s].numpy(), g['box' + s], 3e-2, 0, 'box' + s)
        flat = m.flatten(1)
        assert (st['logits' + s][flat == 0] == orc.MASK_FILL).all()
        assert (st['logits' + s][flat != 0] > -1e8).all()            # 1e-6 is a weight, not a fill
        assert torch.from_numpy(g['logits' + s])[flat == 0].eq(orc.MASK_FILL).all()
        # image 2: only the last token is valid - the soft-argmax puts all weight on it
        hf, wf = g['grid' + s]
        stride = int(g['img' + s][0]) // int(hf)
        want = torch.tensor([(wf - 1 + 0.5) * stride, (hf - 1 + 0.5) * stride])
        assert (torch.from_numpy(g['cxy' + s][2]) - want).abs().max() <= 1e-3
    monkeypatch.setattr(orc, 'linear_attention', _kv_mask_once)
    wrong = orc.hot_path(f1, f2, w, im1, im2, return_stages=True, mask1=m1, mask2=m2)
    assert np.abs(wrong['hs1'].numpy() - g['hs1']).max() > 1e-2
    # (on 0/1 masks m^2 == m: the restatement is the same function there)
    ones = (m1 != 0).float(), (m2 != 0).float()
    a = orc.hot_path(f1, f2, w, im1, im2, return_stages=True, mask1=ones[0], mask2=ones[1])
    monkeypatch.undo()
    b = orc.hot_path(f1, f2, w, im1, im2, return_stages=True, mask1=ones[0], mask2=ones[1])
    assert torch.allclose(a['hs1'], b['hs1'], atol=1e-6)
