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
