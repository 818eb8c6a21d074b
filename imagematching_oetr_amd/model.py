"""Drop-in ``OETR`` module: reference constructor, state-dict keys and
``forward_dummy(image1, image2, mask1=None, mask2=None)`` signature, with the
feature-correlation transformer and the regression heads executed by the
hand-written HIP library (``csrc/`` -> ``liboetr_hip.so``).

Mirrors reference ``src/model.py:38-252`` (inference half) and
``build_detectors`` (:380-384).  The ResNet trunk runs as torch ops (host code,
MIOpen); the neck (input_proj, PatchMerging, input_proj2) and everything from
``feature_correlation`` to the final boxes go through the C ABI declared in
``include/oetr_hip.h``.  There is no
CPU or eager fallback for that part: if the extension is missing or the
tensors are not on a GPU the call raises.

The hot-path sub-modules below are *parameter containers*: they exist so that
``state_dict()``/``load_state_dict(strict=True)`` match a reference checkpoint
key for key and so that random init follows the reference's
(Xavier-uniform on the transformer matrices, ``transformer.py:308-311``).
Their ``forward`` is never called.
"""
import collections
import dataclasses

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import losses

from .backbone import PatchMerging, PositionEncodingSine, ResnetEncoder
from .hip_engine import (FLAG_EXCHANGE, FLAG_F16_RANGE, FLAG_INVALID, HotPathEngine, NeckEngine, OetrExchangeError,
                         OetrRangeError,
                         hot_path_keys, neck_keys)


class _EncoderLayerParams(nn.Module):
    # reference transformer.py:76-102
    def __init__(self, d):
        super().__init__()
        self.q_proj = nn.Linear(d, d, bias=False)
        self.k_proj = nn.Linear(d, d, bias=False)
        self.v_proj = nn.Linear(d, d, bias=False)
        self.merge = nn.Linear(d, d, bias=False)
        self.mlp = nn.Sequential(nn.Linear(d, 2 * d, bias=False), nn.GELU(),
                                 nn.Linear(2 * d, d, bias=False))
        self.pre_norm_q = nn.LayerNorm(d)
        self.pre_norm_kv = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)


class _MultiHeadAttentionParams(nn.Module):
    # reference transformer.py:46-53
    def __init__(self, d):
        super().__init__()
        self.q_proj = nn.Linear(d, d)
        self.k_proj = nn.Linear(d, d)
        self.v_proj = nn.Linear(d, d)
        self.merge = nn.Linear(d, d, bias=False)


class _DecoderLayerParams(nn.Module):
    # reference transformer.py:190-222; q/k/v_proj and merge at this level are
    # parameters the reference registers but never uses.
    def __init__(self, d):
        super().__init__()
        self.q_proj = nn.Linear(d, d, bias=False)
        self.k_proj = nn.Linear(d, d, bias=False)
        self.v_proj = nn.Linear(d, d, bias=False)
        self.self_attn = _MultiHeadAttentionParams(d)
        self.multihead_attn = _MultiHeadAttentionParams(d)
        self.merge = nn.Linear(d, d, bias=False)
        self.mlp = nn.Sequential(nn.Linear(d, 2 * d, bias=False),
                                 nn.ReLU(True),
                                 nn.Linear(2 * d, d, bias=False))
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)
        self.norm3 = nn.LayerNorm(d)


class _DecoderParams(nn.Module):
    def __init__(self, d, num_layers):
        super().__init__()
        self.layers = nn.ModuleList(
            [_DecoderLayerParams(d) for _ in range(num_layers)])


class _QueryTransformerParams(nn.Module):
    # reference transformer.py:287-311 (nhead=8, 4x(self,cross), 2 decoder layers)
    def __init__(self, d, nhead=8, num_layers=4):
        super().__init__()
        self.nhead = nhead
        self.encoder = nn.ModuleList(
            [_EncoderLayerParams(d) for _ in range(2 * num_layers)])
        self.decoder = _DecoderParams(d, 2)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)


@dataclasses.dataclass(slots=True)
class _Batch:
    """A submitted batch whose deferred check has not been settled (``OETR._inflight``)."""
    boxes: tuple            # (box1, box2): views of one [2,n,4] block - its storage identifies the batch
    tickets: list           # FlagTickets of the batch's status words
    rerun: object           # rerun(exchange_only) -> the boxes to copy in when the batch tripped; None: unchecked
    stream: object = None   # side stream of the throughput mode (None: the caller's stream)
    done: object = None     # event behind the batch on `stream`
    tainted: bool = False   # enqueued on `stream` behind a failed decoder exchange: re-run as well


class OETR(nn.Module):
    """OETR overlap estimator with the MI355X-native hot path."""

    def __init__(self, cfg):
        super().__init__()
        self.backbone = ResnetEncoder(cfg)
        self.d_model = self.backbone.last_layer // 4
        d = self.d_model
        self.input_proj = nn.Conv2d(self.backbone.last_layer, d, kernel_size=1)
        self.input_proj2 = nn.Conv2d(2 * d, d, kernel_size=1)
        self.patchmerging = PatchMerging((20, 20), d, norm_layer=nn.LayerNorm,
                                         patch_size=[4, 8, 16])
        self.tlbr_reg = nn.Sequential(nn.Linear(d, d, False),
                                      nn.ReLU(inplace=True), nn.Linear(d, 4))
        self.heatmap_conv = nn.Sequential(
            nn.Conv2d(d, d, (3, 3), padding=(1, 1), stride=(1, 1), bias=True),
            nn.GroupNorm(32, d), nn.ReLU(inplace=True),
            nn.Conv2d(d, 1, (1, 1)))
        self.query_embed1 = nn.Embedding(1, d)
        self.query_embed2 = nn.Embedding(1, d)
        self.transformer = _QueryTransformerParams(d, nhead=8, num_layers=4)
        self.pos_encoding = PositionEncodingSine(d, max_shape=cfg.NECK.MAX_SHAPE)
        self.max_shape = cfg.NECK.MAX_SHAPE
        self.cycle = cfg.LOSS.CYCLE_OVERLAP
        self.oiou = cfg.LOSS.OIOU          # IouOverlapLoss(oiou=cfg.LOSS.OIOU), reference model.py:89
        self.softmax_temperature = 1
        #: GEMM arithmetic of the HIP hot path: 'f32_split_f16' (default, fp32-class),
        #: 'f32' (exact), 'f16' / 'bf16' (operands rounded, reduced parity margin)
        self.hip_precision = 'f32_split_f16'
        #: encoder attention core: 'linear' (the reference's QueryTransformer default) or
        #: 'full' (EncoderLayer(attention='full'), reference transformer.py:86-89)
        self.hip_attention = 'linear'
        #: what forward_dummy does when an f16-based precision ('f32_split_f16', 'f32_split_qk16',
        #: 'f16', and the HIP neck) reports an operand beyond the f16 range (|x| >= 65504):
        #: 'f32' = redo the batch with exact-fp32 MFMA (neck: the torch modules),
        #: 'raise' = OetrRangeError, 'ignore' = do not check
        self.hip_on_overflow = 'f32'
        #: True (default): forward_dummy only ENQUEUES - the status word of batch i is stored into a
        #: pinned host word by the batch's LAST KERNEL (oetr_forward*_flagslot) and is examined when batch
        #: i+2 is submitted (one batch stays in flight behind the one being submitted, so the host
        #: never waits for the device), or by hip_flush(); a tripped batch is then re-run ('f32': its box
        #: tensors are overwritten in place, in stream order) or reported ('raise').  The boxes
        #: of the LAST batch are final after hip_flush().  False: check before returning (one
        #: stream synchronisation per call, as the reference's consumers read boxes at once)
        self.hip_defer_check = True
        #: True: the engines are bound to the weights once and only rebuilt by
        #: invalidate_engine() (skips the per-call parameter identity check)
        self.hip_freeze_weights = False
        #: token rows per encoder workgroup: None = auto, 32 or 64 (HotPathEngine.set_encoder_tile)
        self.hip_enc_tile = None
        #: run input_proj -> PatchMerging -> input_proj2 as HIP kernels when the
        #: features are on a GPU (False: the torch modules, as on CPU)
        self.hip_neck = True
        #: forward_dummy hands the trunk output to the HIP neck and lets it store token-major
        #: into the hot path's workspace (no NCHW feat tensors, no transpose launch);
        #: False: feature_extraction + boxes_from_features as separate steps
        self.hip_fuse_neck = True
        #: arithmetic of the torch / MIOpen TRUNK in forward_dummy on a GPU (host code by
        #: north_star; 93 % of the end-to-end time): None = fp32 as the reference, 'float16' /
        #: 'bfloat16' = the trunk's convolutions under torch.autocast (output cast back to
        #: fp32 for the neck).  OPT-IN: measured drift and speed in profiles/r4_trunk_autocast.txt
        self.hip_trunk_dtype = None
        #: run the trunk in channels_last memory format (MIOpen's NHWC kernels)
        self.hip_trunk_channels_last = False
        #: stages of the trunk ('layer0' .. 'layer3') that STAY fp32 under hip_trunk_dtype: the drift of
        #: an autocast trunk is not spread evenly over the stages (profiles/r4_trunk_autocast.txt)
        self.hip_trunk_fp32_stages = ()
        self._engine = None
        self._engine_key = None
        self._engine_f32 = None
        self._neck_engine = None
        self._neck_key = None
        self._hot_params = None       # cached parameter lists of the identity checks (engine())
        self._neck_params = None
        self._throughput_applied = None   # what _throughput_policy last applied to _engine (None: nothing yet)
        self._split_ok = True         # False once OETR_FLAG_EXCHANGE was seen on this engine (settle_exchange)
        #: A/B knob (bench.py): decoder workgroups per image (1 or 4) on checked routes; None: the automatic rule
        self.hip_decoder_split = None
        #: THROUGHPUT MODE: batches of consecutive forward_dummy / boxes_from_* calls alternate over this
        #: many HIP streams (one workspace per stream in the engines), so that the kernels of batch
        #: i+1 fill the CUs batch i leaves idle; the engines run their throughput settings (64-token
        #: encoder workgroups, direct tail form: fewest CU-microseconds per batch).  The trunk stays
        #: on the caller's stream; every side stream waits for its inputs.  Box tensors are complete
        #: - and range-checked, in submission order - after hip_flush() (forward_pairs* call it); at
        #: most hip_streams x hip_queue_depth batches are in flight.  1 (default): latency mode, everything on the
        #: caller's stream with the automatic rules.
        self.hip_streams = 1
        #: throughput mode: batches QUEUED per side stream before the host settles the oldest.  1: a stream's next
        #: batch is submitted once its previous one has published its status word - the stream stands empty for the
        #: host's reaction and the first launch; 2 (default): the host runs a round ahead, the next batch is already
        #: queued behind the running one (tools/queue_depth_probe.py: +1.2 % steady state, +2 % in a 20-step region;
        #: 3 measures like 2).  A batch's check is then settled when 2k more have been submitted (or at hip_flush()).
        self.hip_queue_depth = 2
        #: the engines' throughput settings without the streams (None: follow hip_streams > 1)
        self.hip_throughput = None
        self._inflight = collections.deque()   # _Batch records: submitted, not yet settled, oldest first
        self._side_streams = []
        self._submitted = 0
        self._last_side = None        # side stream of the most recent batch (None: the caller's stream)
        self._graph_tickets = []      # status reads captured into HIP graphs (hip_graph_check)
        self._bank_epoch = 0          # bumped by invalidate_engine(): feature banks filled before are stale

    # ---------------------------------------------------------------- host
    def neck(self, x):
        """Backbone output [n,1024,hb,wb] -> feat [n,256,hb//2,wb//2]
        (reference ``src/model.py:113-118``): the HIP neck on a GPU, the torch
        modules otherwise (host code either way)."""
        if self.hip_neck and x.is_cuda:
            eng = self.neck_engine()
            feat = eng.forward(x)
            if self.hip_on_overflow != 'ignore' and eng.query_flags() & FLAG_INVALID:
                if self.hip_on_overflow == 'raise':
                    raise OetrRangeError('backbone features exceed the f16 range of the HIP neck')
                return self._neck_torch(x)      # exact fp32 route (torch/MIOpen)
            return feat
        return self._neck_torch(x)

    def _neck_torch(self, x):
        return self.input_proj2(self.patchmerging(self.input_proj(x)))

    def trunk(self, images):
        """``self.backbone(images)`` (reference ``src/models/backbone.py:159-174``) with the
        opt-in GPU settings ``hip_trunk_dtype`` / ``hip_trunk_channels_last``; always returns
        the contiguous fp32 ``[n,1024,hb,wb]`` map the neck takes."""
        if not images.is_cuda or (self.hip_trunk_dtype is None and not self.hip_trunk_channels_last):
            return self.backbone(images)
        if self.hip_trunk_channels_last and not getattr(self, '_trunk_cl', False):
            self.backbone.to(memory_format=torch.channels_last)
            self._trunk_cl = True
        if self.hip_trunk_dtype is None:
            return self.backbone(images).contiguous()
        dt = {'float16': torch.float16, 'bfloat16': torch.bfloat16}[self.hip_trunk_dtype]
        if not self.hip_trunk_fp32_stages:
            with torch.autocast('cuda', dtype=dt):
                out = self.backbone(images)
            return out.float().contiguous()
        # stage by stage (the same sequence as ResnetEncoder.forward, reference backbone.py:159-174)
        bb = self.backbone
        x = images.permute(0, 3, 1, 2).contiguous()
        if bb.cfg.NORM_INPUT:
            x = (x - 0.45) / 0.225
        stages = ['layer0', 'layer1', 'layer2'] + {'layer3': ['layer3'], 'layer4': ['layer3', 'layer4']}.get(bb.cfg.BACKBONE.LAYER, [])
        for name in stages:
            if name in self.hip_trunk_fp32_stages:
                x = getattr(bb, name)(x.float())
            else:
                with torch.autocast('cuda', dtype=dt):
                    x = getattr(bb, name)(x)
        return x.float().contiguous()

    def feature_extraction(self, image1, image2, mask1=None, mask2=None):
        """Reference ``src/model.py:109-130``.  Same-sized image batches go through
        the trunk and the neck as ONE batch of 2N images (per-sample ops: same
        results, half the launches)."""
        if image1.shape == image2.shape and not self.training:
            # (eval only: in train() mode one batch of 2N would change the BatchNorm
            #  statistics against the reference's two separate trunk calls)
            n = image1.shape[0]
            f = self.neck(self.trunk(torch.cat([image1, image2], dim=0)))
            feat1, feat2 = f[:n], f[n:]
        else:
            bb1, bb2 = self.trunk(image1), self.trunk(image2)
            for bb in (bb1, bb2):       # refuse before the first neck launch, whichever side is too small
                if bb.shape[2] < 2 or bb.shape[3] < 2:
                    raise ValueError(f'image too small: backbone map {tuple(bb.shape[2:])} gives an empty token grid')
            feat1, feat2 = self.neck(bb1), self.neck(bb2)
        hf1, wf1 = feat1.shape[2:]
        hf2, wf2 = feat2.shape[2:]
        return (feat1, feat2, self.pos_encoding(feat1), self.pos_encoding(feat2),
                hf1, wf1, hf2, wf2)

    # -------------------------------------------------------------- engine
    def hot_path_state(self):
        sd = self.state_dict()
        return {k: sd[k] for k in hot_path_keys()}

    def invalidate_engine(self):
        """Drop the HIP engines (repacked weight copies, folded decoder constants):
        the next call rebuilds them from the module's current parameters.  Needed
        after writes the identity check below cannot see - ``param.data.copy_()``,
        ``param.data.mul_()``, an EMA swap through ``.data`` (neither move the storage
        nor bump ``param._version``) - and after REPLACING a Parameter object of a
        sub-module (the check walks a cached list of the parameter objects; ``.to()``,
        ``load_state_dict`` and this method refresh it)."""
        self.hip_flush()
        self._bank_epoch += 1         # feature banks hold what the OLD weights computed (bank.FeatureBank)
        self._engine = self._engine_key = self._engine_f32 = None
        self._neck_engine = self._neck_key = None
        self._hot_params = self._neck_params = None

    def _apply(self, fn, *args, **kwargs):   # .to() / .cuda() / .half(): storages move
        self.invalidate_engine()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.invalidate_engine()
        return super().load_state_dict(*args, **kwargs)

    def engine(self):
        """HIP engine bound to the current hot-path weights; rebuilt when a
        weight tensor was replaced or written in place through autograd-visible
        ops (see :meth:`invalidate_engine` for the writes it cannot see)."""
        if self.hip_freeze_weights and self._engine is not None and \
                self._engine_key[:3] == (self.hip_precision, self.hip_enc_tile, self.hip_attention):
            self._throughput_policy(self._engine)
            return self._engine
        if self._hot_params is None:      # (151 get_parameter() lookups cost ~0.5 ms: done once)
            self._hot_params = [self.get_parameter(k) for k in hot_path_keys()]
        params = self._hot_params
        key = (self.hip_precision, self.hip_enc_tile, self.hip_attention) + tuple(
            (p.data_ptr(), p._version) for p in params)
        if self._engine is None or key != self._engine_key:
            self._engine_f32 = None
            dev = params[0].device
            if dev.type != 'cuda':
                raise RuntimeError(
                    'OETR hot path needs the model on a GPU (HIP) device; '
                    f'weights are on {dev}. There is no CPU implementation.')
            self._engine = HotPathEngine(self.hot_path_state(), device=dev,
                                         precision=self.hip_precision,
                                         enc_tile=self.hip_enc_tile,
                                         attention=self.hip_attention)
            self._engine_key = key
            self._split_ok = True
            self._throughput_applied = None
        self._throughput_policy(self._engine)
        return self._engine

    def _throughput_policy(self, eng):
        """Latency or throughput settings of the engine (``hip_streams`` / ``hip_throughput``):
        the setters mutate the handle, so a change is applied with nothing in flight."""
        want = bool(self.hip_streams > 1 if self.hip_throughput is None else self.hip_throughput)
        if self._throughput_applied == want:
            return
        if self._throughput_applied is not None:      # (first call on a fresh engine: nothing in flight yet)
            self.hip_flush()
            torch.cuda.synchronize(eng.device)
        two_plane = eng.precision in ('f32_split_f16', 'f32_split_qk16')
        if self.hip_enc_tile is None and eng.precision != 'f32' and eng.attention == 'linear':
            eng.set_encoder_tile(64 if want else 0)
        if two_plane:
            eng.set_tail_mode(2 if want else 0)
        self._throughput_applied = want

    def _decoder_policy(self, eng, checked):
        """The four-workgroup decoder chain (``oetr_set_decoder_split``) waits for its peers and
        reports a residency time-out through ``OETR_FLAG_EXCHANGE`` - outputs invalid.  It is
        therefore allowed (automatic rule, 0) only on calls whose status word WILL be read and
        acted on; every other route - precisions without a range guard, ``hip_on_overflow =
        'ignore'``, the reference's inner seams - runs one workgroup per image, which waits for
        nobody.  Also off for good once a time-out was seen on this engine."""
        want = 0 if (checked and self._split_ok and self.hip_streams <= 4) else 1
        if want == 0 and self.hip_decoder_split:
            want = int(self.hip_decoder_split)
        if eng._dec_split_set != want:
            eng.set_decoder_split(want)

    def exact_engine(self):
        """Exact-fp32 MFMA engine on the same weights: the route taken when an
        f16-based precision reports an operand out of range."""
        main = self.engine()
        if self.hip_precision == 'f32':
            return main
        if self._engine_f32 is None:
            self._engine_f32 = HotPathEngine(self.hot_path_state(), device=main.device,
                                             precision='f32', attention=self.hip_attention)
            self._engine_f32.set_decoder_split(1)    # the re-run route waits for nobody (FLAG_EXCHANGE)
        return self._engine_f32

    def neck_engine(self):
        """HIP neck bound to the current neck weights (rebuilt when they change)."""
        if self.hip_freeze_weights and self._neck_engine is not None:
            return self._neck_engine
        if self._neck_params is None:
            self._neck_params = [self.get_parameter(k) for k in neck_keys()]
        params = self._neck_params
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._neck_engine is None or key != self._neck_key:
            sd = self.state_dict()
            self._neck_engine = NeckEngine({k: sd[k] for k in neck_keys()},
                                           device=params[0].device)
            self._neck_key = key
        return self._neck_engine

    def _check_masks(self, mask1, mask2, encoder=True):
        """forward_dummy's optional masks (reference ``src/model.py:229``; [N,hf,wf] at the token
        grid's resolution, any numeric / bool dtype): both or neither; the encoder kernels carry
        them in the default arithmetic with linear attention (``oetr_forward_masked``)."""
        if mask1 is None and mask2 is None:
            return False
        if mask1 is None or mask2 is None:
            raise ValueError('masks: pass both mask1 and mask2, or neither')
        if encoder and (self.hip_precision not in ('f32_split_f16', 'f32_split_qk16', 'f32') or self.hip_attention != 'linear'):
            raise NotImplementedError(
                "masks are built for hip_precision='f32_split_f16' / 'f32_split_qk16' / 'f32' with linear attention (the "
                "reference's FullAttention turns a masked query row into NaN, linear_attention.py:74-81); "
                f"this model runs hip_precision='{self.hip_precision}', hip_attention='{self.hip_attention}'")
        return True

    # ---------------------------------------------- reference inner seams
    def feature_correlation(self, feat1, feat2, pos1, pos2, mask1=None,
                            mask2=None):
        """Reference ``src/model.py:132-143``: -> hs1, hs2 [N,1,C],
        memory1 [N,L1,C], memory2 [N,L2,C]."""
        self._check_masks(mask1, mask2)
        eng = self.engine()
        self._decoder_policy(eng, checked=False)     # a seam call reads no status word
        return eng.feature_correlation(feat1, feat2, pos1, pos2, mask1, mask2)

    def center_estimation(self, hs1, hs2, memory1, memory2, hf1, wf1, hf2,
                          wf2, mask1=None, mask2=None):
        """Reference ``src/model.py:145-186``; image heights come from the
        last ``forward_dummy`` call (``self.h1``/``self.h2``) as there."""
        self._check_masks(mask1, mask2, encoder=False)
        return self.engine().center_estimation(hs1, hs2, memory1, memory2, hf1,
                                               wf1, hf2, wf2, self.h1, self.h2, mask1, mask2)

    def size_regression(self, hs1, hs2):
        """Reference ``src/model.py:188-191``."""
        return self.engine().size_regression(hs1, hs2)

    # ------------------------------------------------------------ inference
    @torch.no_grad()
    def forward_dummy(self, image1, image2, mask1=None, mask2=None):
        """Reference ``src/model.py:229-252``: images [N,H,W,3] in [0,1] ->
        (box1, box2), each [N,4] xyxy pixels.  ``mask1`` / ``mask2`` [N,hf,wf]: the
        reference's optional masks at the token grid's resolution (padded batches)."""
        masked = self._check_masks(mask1, mask2)
        # the deferred checks of earlier batches, oldest first - the same count _submit keeps in flight
        # (latency mode: ONE batch stays behind the one being submitted, the host never waits for the device)
        k = self._stream_count()
        self._settle_down_to(self._inflight_cap(k) - 1 if k > 1 else (1 if self.hip_defer_check else 0))
        h1, w1 = image1.shape[1:3]
        h2, w2 = image2.shape[1:3]
        self.h1, self.w1, self.h2, self.w2 = h1, w1, h2, w2
        if masked:
            feat1, feat2, pos1, pos2, _, _, _, _ = self.feature_extraction(image1, image2)
            return self.boxes_from_features(feat1, feat2, pos1, pos2, (h1, w1), (h2, w2), mask1, mask2)
        if self.hip_neck and self.hip_fuse_neck and image1.is_cuda and not self.training:
            # trunk -> HIP neck storing token-major straight into the hot path's workspace
            if image1.shape == image2.shape:
                n = image1.shape[0]
                bb = self.trunk(torch.cat([image1, image2], dim=0))
                return self.boxes_from_backbone(bb[:n], bb[n:], (h1, w1), (h2, w2), both=bb)
            return self.boxes_from_backbone(self.trunk(image1), self.trunk(image2),
                                            (h1, w1), (h2, w2))
        feat1, feat2, pos1, pos2, _, _, _, _ = self.feature_extraction(
            image1, image2)
        return self.boxes_from_features(feat1, feat2, pos1, pos2, (h1, w1), (h2, w2))

    def boxes_from_backbone(self, bb1, bb2, hw1, hw2, both=None):
        """Trunk outputs [N,1024,hb,wb] -> (box1, box2): the HIP neck writes its result
        token-major into the hot-path workspace (``oetr_neck_forward_tokens`` ->
        ``oetr_forward_tokens``), so the NCHW ``feat`` tensors of reference
        ``src/model.py:113-118`` and their ``flatten(2).permute(0, 2, 1)``
        (``transformer.py:338-345``) never exist.  ``both``: the 2N-image tensor
        ``bb1``/``bb2`` are halves of (one neck call).  Same values as
        ``feature_extraction`` + ``boxes_from_features``, which is also the route taken
        when a range flag trips."""
        eng, neck = self.engine(), self.neck_engine()
        n = int(bb1.shape[0])
        hf1, wf1 = int(bb1.shape[2]) // 2, int(bb1.shape[3]) // 2
        hf2, wf2 = int(bb2.shape[2]) // 2, int(bb2.shape[3]) // 2
        checked = self.hip_on_overflow != 'ignore'
        self._decoder_policy(eng, checked)
        meta = lambda h, w: torch.empty(1, 1, h, w, device='meta')   # pos_encoding reads sizes only
        pos1, pos2 = self.pos_encoding(meta(hf1, wf1)), self.pos_encoding(meta(hf2, wf2))

        def enqueue():
            bufs = eng.token_buffers(n, hf1, wf1, hf2, wf2)
            eng.load_pos_tokens(bufs, pos1, pos2)
            # checked: the neck ORs its range bit into the hot-path workspace's status word, and the
            # forward call's last kernel publishes that ONE word into a pinned host slot (ABI 6: no
            # copy / fill dispatch behind the batch).  The engine's word is read in every checked
            # precision: OETR_FLAG_EXCHANGE is not a range matter.
            word = eng._current_ws() if checked else None
            if both is not None:
                neck.forward_tokens(both, bufs['tokens'], status_word=word)
            else:
                neck.forward_tokens(bb1, bufs['tokens1'], status_word=word)
                neck.forward_tokens(bb2, bufs['tokens2'], status_word=word)
            if not checked:
                return eng.forward_tokens(n, hf1, wf1, hf2, wf2, hw1, hw2), []
            boxes, ticket = eng.forward_tokens(n, hf1, wf1, hf2, wf2, hw1, hw2, publish=True)
            return boxes, [ticket]

        def rerun(exchange_only=False):   # the unfused route carries the per-stage handling (raise / exact fp32)
            feat1, feat2 = self.neck(bb1), self.neck(bb2)
            return self._boxes_checked(feat1, feat2, self.pos_encoding(feat1), self.pos_encoding(feat2),
                                       hw1, hw2)
        return self._submit(enqueue, rerun if checked else None, [bb1, bb2] if both is None else [both])

    # ------------------------------------------------------ feature banks
    def feature_bank(self, image_hw, capacity):
        """A :class:`~imagematching_oetr_amd.bank.FeatureBank` for up to ``capacity`` images of size
        ``image_hw`` = (H, W): the trunk and the neck run ONCE per image (``bank.add``), pairs are then
        given by slot number (:meth:`boxes_from_bank`).  Needs the model on a GPU."""
        from .bank import FeatureBank
        return FeatureBank(self, image_hw, capacity)

    @torch.no_grad()
    def boxes_from_bank(self, bank1, idx1, bank2, idx2):
        """(box1, box2), each [n,4]: pair ``p`` is (image ``idx1[p]`` of ``bank1``, image ``idx2[p]`` of
        ``bank2``) - what ``forward_dummy`` returns for those two images, without their trunk and neck
        (``oetr_forward_bank``: one gather launch assembles the batch from the banks' token rows, then
        the token-resident hot path).  ``bank2`` may be ``bank1``; ``idx``: sequences of slot numbers as
        ``bank.add`` returned them, checked on the host (``IndexError``).  The bank-fed sibling of
        :meth:`boxes_from_backbone`: same deferred range check, ``hip_flush``, ``hip_settled`` and
        throughput mode.  No masks on this route."""
        for b in (bank1, bank2):
            b._check_usable(self)
        idx = []
        for b, ix, name in ((bank1, idx1, 'idx1'), (bank2, idx2, 'idx2')):
            host = torch.as_tensor(ix, dtype=torch.int64).reshape(-1).cpu()
            if host.numel() and (int(host.min()) < 0 or int(host.max()) >= len(b)):
                raise IndexError(f'{name}: slot outside the {len(b)} filled slots of the bank')
            idx.append(host)
        n = idx[0].numel()
        if n == 0 or idx[1].numel() != n:
            raise ValueError(f'idx1 / idx2 must name the same, non-zero number of pairs (got {n}, {idx[1].numel()})')
        eng = self.engine()
        (hf1, wf1), (hf2, wf2) = bank1.grid, bank2.grid
        hw1, hw2 = bank1.image_hw, bank2.image_hw
        self.h1, self.w1, self.h2, self.w2 = hw1[0], hw1[1], hw2[0], hw2[1]
        checked = self.hip_on_overflow != 'ignore' and eng.precision in eng.F16_RANGE
        self._decoder_policy(eng, checked)
        meta = lambda h, w: torch.empty(1, 1, h, w, device='meta')   # pos_encoding reads sizes only
        pos1, pos2 = self.pos_encoding(meta(hf1, wf1)), self.pos_encoding(meta(hf2, wf2))
        rows1, rows2 = bank1.rows, bank2.rows
        i1 = idx[0].to(device=eng.device, dtype=torch.int32)
        i2 = idx[1].to(device=eng.device, dtype=torch.int32)

        def enqueue():
            bufs = eng.token_buffers(n, hf1, wf1, hf2, wf2)
            eng.load_pos_tokens(bufs, pos1, pos2)
            if not checked:
                return eng.forward_bank(rows1, i1, rows2, i2, hf1, wf1, hf2, wf2, hw1, hw2), []
            boxes, ticket = eng.forward_bank(rows1, i1, rows2, i2, hf1, wf1, hf2, wf2, hw1, hw2, publish=True)
            return boxes, [ticket]

        def rerun(exchange_only=False):   # the same rows as NCHW features through the immediate route
            feat1 = rows1[i1.long()].permute(0, 2, 1).reshape(n, -1, hf1, wf1).contiguous()
            feat2 = rows2[i2.long()].permute(0, 2, 1).reshape(n, -1, hf2, wf2).contiguous()
            return self._boxes_checked(feat1, feat2, self.pos_encoding(feat1), self.pos_encoding(feat2), hw1, hw2)
        return self._submit(enqueue, rerun if checked else None, [rows1, rows2, i1, i2])

    # -------------------------------------- submission, deferred range check
    #: the status-word ring of an engine holds 16 words (hip_engine._FlagReader.SLOTS), the automatic decoder
    #: rule assumes at most four forwards in flight, and the HIP runtime carries four streams without sharing
    #: a hardware queue: more than eight in flight has no use and would make the ring wait for unread words
    MAX_STREAMS = 8

    def _stream_count(self):
        k = int(self.hip_streams)
        if not 1 <= k <= self.MAX_STREAMS:
            raise ValueError(f'hip_streams must be in 1..{self.MAX_STREAMS}, got {self.hip_streams}')
        return k

    def _inflight_cap(self, k):
        """Batches in flight in the throughput mode: ``hip_queue_depth`` per side stream, at most seven in all
        (one status word per batch, sixteen in an engine's ring), never fewer than one per stream."""
        return max(k, min(k * max(1, int(self.hip_queue_depth)), 7))

    def _streams(self, k):
        dev = self.engine().device
        while len(self._side_streams) < k:
            self._side_streams.append(torch.cuda.Stream(device=dev))
        return self._side_streams

    def _submit(self, enqueue, rerun, inputs):
        """``enqueue()`` -> (boxes, tickets): the HIP calls of one batch and the asynchronous reads of
        the status words behind them.  One stream (default): on the caller's stream, after the
        deferred check of the previous batch.  ``hip_streams`` = k > 1: on side stream (batch index
        mod k), which first waits for the caller's stream (the batch's inputs); at most
        ``hip_queue_depth`` batches per stream stay in flight (`_inflight_cap`), their checks are settled
        oldest first.  ``rerun`` None: nothing to check."""
        k = self._stream_count()
        capturing = torch.cuda.is_current_stream_capturing()
        if k == 1 or capturing:
            # one batch stays in flight behind the one being submitted (its status word is still on
            # its way): settling it here would make the host wait for the device before every submit
            self._settle_down_to(0 if (capturing or not self.hip_defer_check) else 1)
            self._last_side = None
            boxes, tickets = enqueue()
            if rerun is None:
                return boxes
            if capturing:
                # part of a HIP graph: nothing can be examined now, and every replay rewrites the
                # words - hip_graph_check() reads them after the caller has synchronised a replay
                self._graph_tickets += tickets
                return boxes
            batch = _Batch(boxes, tickets, rerun)
        else:
            self._settle_down_to(self._inflight_cap(k) - 1)
            dev = self.engine().device
            side = self._streams(k)[self._submitted % k]
            self._submitted += 1
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                boxes, tickets = enqueue()
                done = torch.cuda.Event()
                done.record(side)
            for t in inputs:                      # allocated on the caller's stream, read on `side`
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(side)
            batch = _Batch(boxes, tickets, rerun, side, done)
            self._last_side = side
        # deferred mode: the check runs at a later submit / hip_flush(); immediate mode: now
        self._inflight.append(batch)
        if not self.hip_defer_check:
            self._settle_down_to(0)
        return boxes

    def hip_settled(self, boxes):
        """True once the deferred check of the batch that returned ``boxes`` has been settled - its
        values are final (``parallel.BoxGatherer(model=...)`` issues a batch's all-gather only then).
        A batch is found by the storage of its box block, so ``boxes`` may be either of its two
        tensors or any view of them.  Batches settle oldest first: when k x ``hip_queue_depth`` more
        have been submitted (``hip_streams = k``; two in the latency mode) or at ``hip_flush()``."""
        key = boxes.untyped_storage().data_ptr()
        return not any(b.boxes[0].untyped_storage().data_ptr() == key for b in self._inflight)

    def hip_batch_stream(self):
        """The HIP stream the most recently submitted batch was enqueued on (throughput mode:
        one of the side streams; otherwise the caller's current stream) - for work that must be
        ordered right behind that batch without waiting for hip_flush(), e.g. an asynchronous
        all-gather of its boxes."""
        if self._last_side is not None and self.hip_streams > 1:
            return self._last_side
        return torch.cuda.current_stream(self.engine().device)

    # ------------------------------------------------ deferred range check
    @property
    def _pending(self):
        """The most recently submitted batch whose check has not been settled (None: none)."""
        return self._inflight[-1] if self._inflight else None

    def hip_graph_check(self):
        """Range guard of forward calls CAPTURED into a HIP graph (their status reads are graph
        nodes writing pinned host words): call after synchronising a replay.  A captured batch
        cannot be re-run from here, so a tripped word raises ``OetrRangeError`` whatever
        ``hip_on_overflow`` says (except 'ignore': nothing was captured)."""
        flags = 0
        for t in self._graph_tickets:
            flags |= t.value()
        if flags & FLAG_EXCHANGE:
            self._exchange_failed()
            raise OetrExchangeError('a batch replayed from a HIP graph lost its split-decoder exchange '
                                    '(OETR_FLAG_EXCHANGE): re-capture the graph (the engine now runs one '
                                    'decoder workgroup per image) or re-submit the batch eagerly')
        if flags & FLAG_F16_RANGE:
            raise OetrRangeError('a batch replayed from a HIP graph overflowed the f16 operand range: '
                                 're-submit it eagerly (exact-fp32 re-run) or use hip_precision "f32"')

    def hip_graph_release(self):
        """Forget the status reads of captured graphs (call when those graphs are discarded, e.g.
        before re-capturing for another shape): their pinned words go back to the engines'
        free lists, ``hip_graph_check`` starts from an empty list."""
        for t in self._graph_tickets:
            t.release()
        self._graph_tickets = []

    def _exchange_failed(self, side=None):
        """OETR_FLAG_EXCHANGE was read from the main engine's word (of the workspace of stream
        ``side``; None = the caller's): re-initialise that status block and keep the decoder on one
        workgroup per image from here on."""
        self._split_ok = False
        if self._engine is not None:
            if side is None:
                self._engine.settle_exchange()
            else:
                with torch.cuda.stream(side):
                    self._engine.settle_exchange()

    def _settle_down_to(self, keep):
        """Settle submitted batches, oldest first, until at most ``keep`` are in flight: the
        caller's stream is ordered behind the batch (side streams), its status words are read
        (they have long arrived unless the batch is the newest), a tripped batch is re-run and
        its box tensors are corrected in place."""
        while len(self._inflight) > keep:
            batch = self._inflight.popleft()
            if batch.stream is not None:
                cur = torch.cuda.current_stream(batch.boxes[0].device)
                cur.wait_event(batch.done)
                for b in batch.boxes:
                    b.record_stream(cur)       # allocated on the side stream, consumed on the caller's stream
            if batch.rerun is not None:
                self._settle(batch)

    def _settle(self, batch):
        flags = 0
        for t in batch.tickets:
            flags |= t.value()
        if not flags & FLAG_INVALID and not batch.tainted:
            return
        if flags & FLAG_EXCHANGE:
            # a residency time-out of the split decoder, not a property of the inputs: the same
            # precision is submitted again (one workgroup per image); only a range overflow of
            # THAT run takes the exact-fp32 / raise route.  Batches already enqueued BEHIND this one
            # on the same stream used the failed call's status block (its call counters are not
            # trustworthy): they are re-run as well when their turn comes.
            for later in self._inflight:
                if later.stream is batch.stream:
                    later.tainted = True
            self._exchange_failed(batch.stream)
        good = batch.rerun(exchange_only=not flags & FLAG_F16_RANGE)   # may raise under hip_on_overflow == 'raise'
        for dst, src in zip(batch.boxes, good):
            dst.copy_(src)          # in place and in stream order: holders of the boxes see the re-run

    def hip_flush(self):
        """Complete every submitted batch's deferred range check (``hip_defer_check``), oldest
        first: waits for those batches' status words only (published by each batch's last kernel)
        and orders the caller's stream behind the side streams of the throughput mode.
        A tripped batch is re-run in exact fp32 into the box tensors it returned ('f32') or raises
        ``OetrRangeError`` ('raise').  Called automatically as far as needed when the next batch is
        submitted; call it before consuming the boxes of the LAST batch(es)."""
        self._settle_down_to(0)

    def boxes_from_features(self, feat1, feat2, pos1, pos2, hw1, hw2, mask1=None, mask2=None):
        """Everything after ``feature_extraction`` (reference ``src/model.py:239-252``)
        as one fused HIP call, with the f16 range guard of the chosen precision (deferred
        like ``forward_dummy``'s under ``hip_defer_check``; the exact-fp32 re-run carries the
        masks too)."""
        self._check_masks(mask1, mask2)
        eng = self.engine()
        checked = self.hip_on_overflow != 'ignore' and eng.precision in eng.F16_RANGE
        self._decoder_policy(eng, checked)

        def call(e, publish=False):
            return e.forward(feat1, feat2, pos1, pos2, hw1, hw2, mask1=mask1, mask2=mask2, publish=publish)

        def enqueue():
            if not checked:
                return call(eng), []
            boxes, ticket = call(eng, publish=True)       # status word published by the last kernel
            return boxes, [ticket]

        def rerun(exchange_only=False):
            return (self._checked_call if exchange_only else self._exact_call)(call)[0]
        return self._submit(enqueue, rerun if checked else None, [feat1, feat2, pos1, pos2, mask1, mask2])

    def _exact_call(self, call):
        """The route of a call whose GEMM operands overflowed the f16 range: ``OetrRangeError`` under
        ``hip_on_overflow = 'raise'``, else ``call(engine)`` on the exact-fp32 engine -> (result, engine)."""
        if self.hip_on_overflow == 'raise':
            raise OetrRangeError(
                f"a GEMM operand reached |x| >= 65504 under hip_precision="
                f"'{self.hip_precision}'; set hip_precision to 'f32' or 'bf16'")
        eng = self.exact_engine()
        return call(eng), eng

    def _checked_call(self, call, checked=True):
        """Immediate (synchronising) check: ``call(engine)`` on the main engine, its status word read at
        once (``checked``; False: neither read nor a split decoder).  ``OETR_FLAG_EXCHANGE`` (only while
        the split is still allowed: first time-out) -> ``call`` again at the same precision, one decoder
        workgroup per image; ``OETR_FLAG_F16_RANGE`` -> :meth:`_exact_call`.  -> (result, engine)."""
        eng = self.engine()
        self._decoder_policy(eng, checked)
        out = call(eng)
        flags = eng.query_flags() if checked else 0
        if flags & FLAG_EXCHANGE:
            self._exchange_failed()
            out = call(eng)
            flags = eng.query_flags()
        if eng.precision in eng.F16_RANGE and flags & FLAG_F16_RANGE:
            return self._exact_call(call)
        return out, eng

    def _boxes_checked(self, feat1, feat2, pos1, pos2, hw1, hw2, mask1=None, mask2=None):
        """Immediate form of ``boxes_from_features``: the re-run route of a tripped fused batch."""
        return self._checked_call(lambda e: e.forward(feat1, feat2, pos1, pos2, hw1, hw2, mask1=mask1,
                                                      mask2=mask2))[0]

    def forward(self, data, validation=False):
        """Training-side pipeline of reference ``src/model.py:255-376`` as a FORWARD
        pass: the pairs selected by ``data['overlap_valid']`` go through the HIP hot
        path, the UNCLAMPED boxes (``obtain_overlap_bbox``, ``:193-226``) are compared
        with ``data['overlap_box1/2']`` and the reference's result dict is returned
        (``pred_bbox1/2``, ``iouloss``, ``wh_loss``, ``loc_loss``, ``iou1/2``,
        ``oiou1/2`` and, with ``LOSS.CYCLE_OVERLAP``, ``cycle_loss``).

        The HIP kernels have no backward: the losses are VALUES (validation, loss
        curves, checkpoint selection).  Called with autograd enabled on parameters that
        require grad this raises instead of silently returning graph-less losses."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(
                'OETR.forward(data): the HIP hot path has no backward kernels - wrap the call '
                'in torch.no_grad() (loss values / metrics), or train with the reference '
                'PyTorch model and load the checkpoint here (same state-dict keys)')
        valid = data['overlap_valid']
        mask1 = mask2 = None
        if 'resize_mask1' in data:       # reference model.py:256-258
            mask1, mask2 = data['resize_mask1'][valid], data['resize_mask2'][valid]
        self._check_masks(mask1, mask2)
        image1, image2 = data['image1'][valid], data['image2'][valid]
        h1, w1 = image1.shape[1:3]
        h2, w2 = image2.shape[1:3]
        self.h1, self.w1, self.h2, self.w2 = h1, w1, h2, w2
        with torch.no_grad():
            feat1, feat2, pos1, pos2, hf1, wf1, hf2, wf2 = self.feature_extraction(image1, image2)
            checked = self.hip_on_overflow != 'ignore' and self.hip_precision in HotPathEngine.F16_RANGE
            st, eng = self._checked_call(lambda e: e.forward(feat1, feat2, pos1, pos2, (h1, w1), (h2, w2),
                                                             stages=True, mask1=mask1, mask2=mask2), checked)
            xyxy1, xyxy2, cxywh1, cxywh2 = losses.obtain_overlap_bbox(
                st['cxy1'], st['tlbr1'], st['cxy2'], st['tlbr2'], (h1, w1), (h2, w2))
            gt1 = data['overlap_box1'][valid].to(xyxy1.device)
            gt2 = data['overlap_box2'][valid].to(xyxy1.device)
            gtc1 = losses.box_xyxy_to_cxywh(gt1, max_h=h1, max_w=w1)
            gtc2 = losses.box_xyxy_to_cxywh(gt2, max_h=h2, max_w=w2)
            s1 = torch.tensor([w1, h1], device=xyxy1.device)
            s2 = torch.tensor([w2, h2], device=xyxy1.device)
            loc = F.l1_loss(cxywh1[:, :2] / s1, gtc1[:, :2] / s1) + F.l1_loss(cxywh2[:, :2] / s2, gtc2[:, :2] / s2)
            wh = (F.l1_loss(cxywh1[:, 2:] / s1, gtc1[:, 2:] / s1) + F.l1_loss(cxywh2[:, 2:] / s2, gtc2[:, 2:] / s2)) / 2
            box_loss = losses.oiou_loss if self.oiou else losses.giou_loss
            iouloss = (box_loss(xyxy1, gt1) + box_loss(xyxy2, gt2)) / 2.0
            results = {
                'pred_bbox1': xyxy1, 'pred_bbox2': xyxy2,
                'iouloss': iouloss.mean(), 'wh_loss': wh.mean(), 'loc_loss': loc.mean(),
                'iou1': losses.bbox_iou_aligned(xyxy1, gt1).mean(),
                'iou2': losses.bbox_iou_aligned(xyxy2, gt2).mean(),
                'oiou1': losses.bbox_oiou(gt1, xyxy1).mean(),
                'oiou2': losses.bbox_oiou(gt2, xyxy2).mean(),
            }
            if self.cycle:
                # centres with the two decoder queries swapped (reference model.py:354-356)
                c1f2, c2f1 = eng.center_estimation(st['hs2'], st['hs1'], st['memory1'], st['memory2'],
                                                   hf1, wf1, hf2, wf2, h1, h2, mask1, mask2)
                _, _, cyc1, cyc2 = losses.obtain_overlap_bbox(c1f2, st['tlbr1'], c2f1, st['tlbr2'],
                                                              (h1, w1), (h2, w2))
                cycle = F.l1_loss(cyc1[:, :2] / s1, gtc1[:, :2] / s1) + F.l1_loss(cyc2[:, :2] / s2, gtc2[:, :2] / s2)
                results['cycle_loss'] = cycle.mean()
        return results


def build_detectors(cfg):
    """Reference ``src/model.py:380-384``."""
    if cfg.MODEL == 'oetr':
        return OETR(cfg)
    raise ValueError(f'OETR.MODEL {cfg.MODEL} not supported.')
