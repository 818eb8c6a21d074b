"""Plug-in wrapper with the interface of the reference's ``dloc/core/matchers/nearest_neighbor.py:36-67``
(``BaseModel`` contract, ``dloc/core/utils/base_model.py:8-34``): ``NearestNeighbor(conf)(data)`` ->
``{'matches0', 'matching_scores0'}`` with ``data = {'descriptors0': [B,D,N], 'descriptors1': [B,D,M]}``,
through :func:`imagematching_oetr_amd.match_descriptors` - one device call for the whole batch.

As in ``dloc_overlap.py`` there are two ways in: :class:`NearestNeighbor` stands alone, and inside the
reference tree :class:`NearestNeighborPluginMixin` combines with the reference's own ``BaseModel`` in a
three-line ``dloc/core/matchers/<name>.py``.

Where the reference leaves the result open this matcher decides it: a tied maximum goes to
the lowest index, and ``M = 1`` with a ratio threshold passes the ratio test where ``topk(2)`` raises.
"""
import torch

from .dloc_overlap import _BaseModel
from .dense_match import match_dense
from .fine_match import fine_windows, refine_matches
from .nn_match import match_descriptors


class NearestNeighborPluginMixin:
    """``_init`` / ``_forward`` of the nearest-neighbour matcher (reference ``nearest_neighbor.py:36-67``)."""

    default_conf = {
        'ratio_threshold': None,
        'distance_threshold': None,
        'do_mutual_check': True,
    }
    required_data_keys = ['descriptors0', 'descriptors1']

    def _init(self, conf, model_path):
        pass

    def _forward(self, data):
        d0, d1 = data['descriptors0'], data['descriptors1']
        B, D, N = d0.shape
        M = int(d1.shape[2])
        if d1.shape[0] != B or d1.shape[1] != D:
            raise ValueError(f'descriptors0 is {tuple(d0.shape)}, descriptors1 {tuple(d1.shape)}: need [B,D,N] and [B,D,M]')
        dev = d0.device
        steps = torch.arange(B + 1, dtype=torch.int32, device=dev)
        res = match_descriptors(d0.permute(0, 2, 1).reshape(B * N, D), d1.permute(0, 2, 1).reshape(B * M, D),
                                offsets0=steps * N, offsets1=steps * M, max_k0=N, max_k1=M,
                                ratio_threshold=self.conf['ratio_threshold'],
                                distance_threshold=self.conf['distance_threshold'],
                                do_mutual_check=self.conf['do_mutual_check'])
        return {'matches0': res['matches0'].view(B, N).long(),
                'matching_scores0': res['matching_scores0'].view(B, N)}


class NearestNeighbor(NearestNeighborPluginMixin, _BaseModel):
    """The stand-alone form: nothing of the reference needs to be importable."""


class DualSoftmaxPluginMixin:
    """A detector-free matcher in the shape of the reference's ``direct`` plug-ins (``dloc/core/matchers/loftr.py``):
    ``required_inputs`` are the two images, ``net(image0, image1)`` - a torch module or callable given at construction
    - returns the two coarse feature maps ``[B,D,h0,w0]`` and ``[B,D,h1,w1]`` (float32), and the matching head is
    :func:`imagematching_oetr_amd.match_dense`: one device call for the whole batch.  The result has one entry per
    batch element, as the reference's lists have: ``keypoints0`` ``[L,2]``, ``keypoints1`` ``[S,2]`` (every token's
    pixel position in its image), ``matches0`` int64 ``[L]`` with ``-1`` left in place (the reference's ``process()``
    handles those through ``matches > -1``) and ``matching_scores0`` ``[L]``."""

    default_conf = {
        'temperature': 0.1,
        'threshold': 0.2,
        'border_rm': 2,
        'cell': 8,
    }
    required_inputs = ['image0', 'image1']
    required_data_keys = ['image0', 'image1']

    def _init(self, conf, model_path):
        pass

    def _forward(self, data):
        if self.net is None:
            raise ValueError('DualSoftmax needs `net`: a callable (image0, image1) -> the two coarse feature maps')
        f0, f1 = self.net(data['image0'], data['image1'])
        if f0.dim() != 4 or f1.dim() != 4 or f0.shape[:2] != f1.shape[:2]:
            raise ValueError(f'net returned {tuple(f0.shape)} and {tuple(f1.shape)}: need [B,D,h0,w0] and [B,D,h1,w1]')
        B, D, h0, w0 = (int(v) for v in f0.shape)
        h1, w1 = int(f1.shape[2]), int(f1.shape[3])
        L, S = h0 * w0, h1 * w1
        dev = f0.device
        steps = torch.arange(B + 1, dtype=torch.int32, device=dev)
        grids = torch.tensor([[h0, w0], [h1, w1]], dtype=torch.int32, device=dev)
        res = match_dense(f0.permute(0, 2, 3, 1).reshape(B * L, D), f1.permute(0, 2, 3, 1).reshape(B * S, D),
                          offsets0=steps * L, offsets1=steps * S, grids0=grids[0].expand(B, 2).contiguous(),
                          grids1=grids[1].expand(B, 2).contiguous(), max_k0=L, max_k1=S,
                          temperature=self.conf['temperature'], threshold=self.conf['threshold'],
                          border_rm=self.conf['border_rm'], cell=self.conf['cell'])
        return {'keypoints0': list(res['keypoints0'].view(B, L, 2)), 'keypoints1': list(res['keypoints1'].view(B, S, 2)),
                'matches0': list(res['matches0'].view(B, L).long()),
                'matching_scores0': list(res['matching_scores0'].view(B, L))}


class DualSoftmax(DualSoftmaxPluginMixin, _BaseModel):
    """The stand-alone form: ``DualSoftmax(conf, net=net)``; nothing of the reference needs to be importable."""

    def __init__(self, conf, model_path=None, net=None):
        super().__init__(conf, model_path)
        self.net = net


class CoarseToFinePluginMixin:
    """The whole detector-free matcher of the reference's ``direct`` branch (``dloc/core/matchers/loftr.py``), coarse to
    fine: ``net(image0, image1)`` returns the two coarse maps ``[B,D,h,w]`` and the two fine maps ``[B,C,hf,wf]``
    (float32); :func:`imagematching_oetr_amd.match_dense` matches the coarse maps, :func:`fine_windows` gathers the
    fine windows of the matches, ``fine_net(win0, win1)`` - optional, a torch module or callable - returns the
    processed windows ``[M,W*W,C]``, and :func:`refine_matches` is the expectation head.  The result has the
    reference's ``loftr`` keys, one entry per batch element: ``keypoints0`` = ``mkpts0`` ``[m,2]``, ``keypoints1`` =
    ``mkpts1`` ``[m,2]``, ``matches0`` = ``arange(m)`` and ``matching_scores0`` ``[m]`` (the coarse confidence).  This
    is the one place that reads the number of matches back (one read of the list offsets)."""

    default_conf = {**DualSoftmaxPluginMixin.default_conf, 'window': 5, 'stride': 4, 'max_matches': None}
    required_inputs = ['image0', 'image1']
    required_data_keys = ['image0', 'image1']

    def _init(self, conf, model_path):
        pass

    def _forward(self, data):
        if self.net is None:
            raise ValueError('CoarseToFine needs `net`: a callable (image0, image1) -> the two coarse and the two fine '
                             'feature maps')
        c0, c1, f0, f1 = self.net(data['image0'], data['image1'])
        if any(t.dim() != 4 for t in (c0, c1, f0, f1)) or c0.shape[:2] != c1.shape[:2] or f0.shape[:2] != f1.shape[:2] \
                or f0.shape[0] != c0.shape[0]:
            raise ValueError('net must return [B,D,h0,w0], [B,D,h1,w1], [B,C,hf0,wf0], [B,C,hf1,wf1]')
        B, D, h0, w0 = (int(v) for v in c0.shape)
        h1, w1 = int(c1.shape[2]), int(c1.shape[3])
        L, S = h0 * w0, h1 * w1
        dev = c0.device
        steps = torch.arange(B + 1, dtype=torch.int32, device=dev)

        def grids(h, w):
            return torch.tensor([[h, w]], dtype=torch.int32, device=dev).expand(B, 2).contiguous()

        coarse = match_dense(c0.permute(0, 2, 3, 1).reshape(B * L, D), c1.permute(0, 2, 3, 1).reshape(B * S, D),
                             offsets0=steps * L, offsets1=steps * S, grids0=grids(h0, w0), grids1=grids(h1, w1),
                             max_k0=L, max_k1=S, temperature=self.conf['temperature'],
                             threshold=self.conf['threshold'], border_rm=self.conf['border_rm'], cell=self.conf['cell'])
        C = int(f0.shape[1])
        (hf0, wf0), (hf1, wf1) = (int(v) for v in f0.shape[2:]), (int(v) for v in f1.shape[2:])
        cap = B * L if self.conf['max_matches'] is None else int(self.conf['max_matches'])
        windows = fine_windows(coarse, f0.permute(0, 2, 3, 1).reshape(B * hf0 * wf0, C),
                               f1.permute(0, 2, 3, 1).reshape(B * hf1 * wf1, C), fine_offsets0=steps * (hf0 * wf0),
                               fine_offsets1=steps * (hf1 * wf1), fine_grids0=grids(hf0, wf0), fine_grids1=grids(hf1, wf1),
                               window=self.conf['window'], stride=self.conf['stride'], max_matches=cap, max_k0=L)
        win0, win1 = self.fine_net(windows['win0'], windows['win1']) if self.fine_net is not None else (None, None)
        fine = refine_matches(windows, coarse, win0=win0, win1=win1,
                              fine_cell=self.conf['cell'] / self.conf['stride'])
        rows = windows['rows'].long()
        scores = coarse['matching_scores0'][(rows[:, 0] * L + rows[:, 1]).clamp_(min=0)]
        cuts = windows['moffsets'].tolist()                          # the one read
        out = {'keypoints0': [], 'keypoints1': [], 'matches0': [], 'matching_scores0': []}
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            out['keypoints0'].append(fine['mkpts0'][lo:hi])
            out['keypoints1'].append(fine['mkpts1'][lo:hi])
            out['matches0'].append(torch.arange(hi - lo, device=dev))
            out['matching_scores0'].append(scores[lo:hi])
        return out


class CoarseToFine(CoarseToFinePluginMixin, _BaseModel):
    """The stand-alone form: ``CoarseToFine(conf, net=net, fine_net=None)``; nothing of the reference needs to be
    importable."""

    def __init__(self, conf, model_path=None, net=None, fine_net=None):
        super().__init__(conf, model_path)
        self.net = net
        self.fine_net = fine_net
