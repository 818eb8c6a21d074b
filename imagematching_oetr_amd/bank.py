"""Feature bank: the trunk and the neck once per IMAGE, pairs given by index.

Every other entry point takes pairs of images and pushes both images of every pair through the
ResNet trunk and the neck, as the reference does (``dloc/core/overlap_features.py:270-294``).  The
jobs the model is used for are pair LISTS over an image SET - retrieval shortlists, SfM pair files,
exhaustive matching - where an image appears in many pairs, and its trunk + neck output depends on
that image alone (no cross-image term before ``feature_correlation``).  A :class:`FeatureBank`
keeps that output, token-major, in device memory; ``OETR.boxes_from_bank`` assembles a batch of
pairs from it by slot number on the device (``oetr_forward_bank``, ``include/oetr_bank.h``) and
runs the hot path.  ``pipeline.forward_pairs_indexed`` is the front-end over an image list.
"""
import torch

from .hip_engine import D_MODEL, FLAG_INVALID, OetrRangeError


class FeatureBank:
    """Token rows of up to ``capacity`` images of ONE size ``image_hw`` = (H, W), created by
    ``model.feature_bank(image_hw, capacity)``::

        slots = bank.add(images)          # [n,H,W,3] in [0,1] -> list of n slot numbers
        slots = bank.add_backbone(bb)     # [n,1024,hb,wb] trunk output (what add() calls after model.trunk)
        box1, box2 = model.boxes_from_bank(bank1, idx1, bank2, idx2)
        bank.clear()

    Memory: one image takes ``(hb // 2) * (wb // 2)`` rows of 1 KB, with ``hb x wb`` the trunk's
    stride-16 map - ``(H / 32) * (W / 32)`` KB for sizes divisible by 32, 400 KB for a 640 x 640
    image.  The rows are allocated (``capacity`` images) at the first ``add``.  Eviction and
    streaming of image sets that do not fit are the caller's business: fill, use, ``clear()``.

    The bank is append-only until :meth:`clear`.  It is valid for the weights it was filled with:
    ``model.invalidate_engine()`` - and so ``.to()`` and ``load_state_dict`` - makes it stale, and a
    stale bank raises ``RuntimeError`` until it is cleared.  In-place edits of TRUNK weights are
    not detected (nor are the writes ``OETR.invalidate_engine`` lists for the engines): clear the
    bank after them.  Eval mode only: train-mode BatchNorm statistics depend on the batch."""

    def __init__(self, model, image_hw, capacity):
        try:
            dev = next(model.parameters()).device
        except StopIteration:
            dev = torch.device('cpu')
        if dev.type != 'cuda':
            raise RuntimeError('a feature bank needs the model on a GPU (HIP) device; weights are on '
                               f'{dev}. There is no CPU implementation.')
        if int(capacity) < 1:
            raise ValueError('capacity must be >= 1')
        self.model, self.device = model, dev
        self.image_hw = (int(image_hw[0]), int(image_hw[1]))
        self.capacity = int(capacity)
        self.grid = None        # (hf, wf): known once the first trunk output has been seen
        self._rows = None       # float32 [capacity, hf*wf, 256]
        self._filled = 0
        self._epoch = model._bank_epoch

    def __len__(self):
        """Filled slots."""
        return self._filled

    @property
    def rows(self):
        """The filled part: float32 [len(bank), hf*wf, 256] (a view; what ``oetr_forward_bank`` reads)."""
        return self._rows[:self._filled]

    def _check_usable(self, model=None):
        if model is not None and model is not self.model:
            raise ValueError('this feature bank belongs to another model')
        if self._epoch != self.model._bank_epoch:
            raise RuntimeError('stale feature bank: the model\'s weights or device changed after it was filled '
                               '(invalidate_engine / .to() / load_state_dict); clear() it and add the images again')

    def clear(self):
        """Empty the bank (slots are handed out from 0 again) and bind it to the model's current
        weights.  Completes every submitted batch first (``model.hip_flush()``): no batch in flight on
        a side stream may still be reading a slot that is about to be rewritten."""
        self.model.hip_flush()
        self._filled = 0
        self._epoch = self.model._bank_epoch

    def _check_add(self, n):
        self._check_usable()
        if self.model.training:
            raise RuntimeError('a feature bank is filled in eval() mode only: train-mode BatchNorm '
                               'statistics depend on the batch an image is added with')
        if self._filled + n > self.capacity:
            raise RuntimeError(f'feature bank full: {self._filled} of {self.capacity} slots filled, '
                               f'{n} more asked for')

    @torch.no_grad()
    def add(self, images):
        """``images`` [n,H,W,3] in [0,1] (any device; moved to the model's) -> their slot numbers.
        ``model.trunk`` on the batch, then the neck straight into the bank's rows."""
        if images.dim() != 4 or tuple(images.shape[1:]) != self.image_hw + (3,):
            raise ValueError(f'images must be [n,{self.image_hw[0]},{self.image_hw[1]},3], got {tuple(images.shape)}')
        self._check_add(int(images.shape[0]))
        return self.add_backbone(self.model.trunk(images.to(self.device, non_blocking=True)))

    @torch.no_grad()
    def add_backbone(self, bb):
        """``bb`` [n,1024,hb,wb]: trunk outputs of n images of the bank's size -> their slot numbers.
        The HIP neck stores token-major into the bank (``oetr_neck_forward_tokens``: no feature
        tensor in between); its f16 range guard is read once per call and follows
        ``model.hip_on_overflow`` as ``OETR.neck`` does: 'f32' recomputes the chunk with the torch
        neck, 'raise' raises ``OetrRangeError``, 'ignore' does not look."""
        model = self.model
        if bb.dim() != 4 or bb.device != self.device:
            raise ValueError(f'bb must be a [n,1024,hb,wb] tensor on {self.device}')
        n, grid = int(bb.shape[0]), (int(bb.shape[2]) // 2, int(bb.shape[3]) // 2)
        self._check_add(n)
        if self._rows is None:
            self.grid = grid
            self._rows = torch.empty(self.capacity, grid[0] * grid[1], D_MODEL, device=self.device)
        elif grid != self.grid:
            raise ValueError(f'trunk output gives a {grid[0]}x{grid[1]} token grid, the bank holds '
                             f'{self.grid[0]}x{self.grid[1]}: one bank = one image size')
        if n == 0:
            return []
        dst = self._rows[self._filled:self._filled + n].view(-1, D_MODEL)

        def torch_neck():
            dst.copy_(model._neck_torch(bb).flatten(2).transpose(1, 2).reshape(-1, D_MODEL))

        if not model.hip_neck:
            torch_neck()
        else:
            eng = model.neck_engine()
            eng.forward_tokens(bb, dst)
            if model.hip_on_overflow != 'ignore' and eng.query_flags() & FLAG_INVALID:
                if model.hip_on_overflow == 'raise':
                    raise OetrRangeError('backbone features exceed the f16 range of the HIP neck')
                torch_neck()      # exact fp32 route (torch/MIOpen)
        first = self._filled
        self._filled += n
        return list(range(first, first + n))
