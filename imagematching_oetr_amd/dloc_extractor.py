"""Plug-in wrapper with the interface of the reference's extractors (``dloc/core/extractors/superpoint.py:22-45``;
``BaseModel`` contract, ``dloc/core/utils/base_model.py:8-34``): ``DenseExtractor(conf, net=net)(data)`` with
``data = {'image': [B,C,H,W]}`` -> ``{'keypoints': [[K,2], ...], 'scores': [[K], ...], 'descriptors': [[D,K], ...]}``,
one entry per image, as SuperPoint returns them.

``net`` is any torch module ``net(image) -> (scores [B,H,W], descriptors [B,D,h,w])``; it stays torch.  The head behind
it - NMS, threshold, border, the best ``max_keypoints``, descriptor sampling - is
:func:`imagematching_oetr_amd.select_keypoints`: one device call for the whole batch.  The statement
is this project's own, modelled on SuperPoint's published post-processing; that code is not part of the reference
checkout, so no parity with it is claimed.  Splitting the joined result into per-image lists reads the offsets back
once; callers that stay on the device use :func:`select_keypoints` itself.

As in ``dloc_matcher.py`` there are two ways in: :class:`DenseExtractor` stands alone, and inside the reference tree
:class:`DenseExtractorPluginMixin` combines with the reference's own ``BaseModel``.
"""
from .dloc_overlap import _BaseModel
from .keypoint_select import keypoint_map_table, select_keypoints


class DenseExtractorPluginMixin:
    """``_init`` / ``_forward`` of a dense extractor with the reference's configuration names
    (``superpoint.py:30-36``).  ``max_keypoints`` -1, the reference's "no limit", means the head's capacity of 4096."""

    default_conf = {
        'nms_radius': 4,
        'keypoint_threshold': 0.005,
        'max_keypoints': -1,
        'remove_borders': 4,
        'cell': 8,
    }
    required_inputs = ['image']
    required_data_keys = ['image']

    def _init(self, conf, model_path):
        pass

    def _forward(self, data):
        scores, descriptors = self.net(data['image'])
        k = int(self.conf['max_keypoints'])
        k = 4096 if k < 0 else k
        res = select_keypoints(keypoint_map_table(scores, descriptors), nms_radius=self.conf['nms_radius'],
                               threshold=self.conf['keypoint_threshold'], remove_borders=self.conf['remove_borders'],
                               max_keypoints=k, cell=self.conf['cell'])
        off = res['offsets'].cpu().tolist()                           # ONE read, which synchronises the stream
        cut = list(zip(off[:-1], off[1:]))
        return {'keypoints': [res['keypoints'][a:b] for a, b in cut],
                'scores': [res['scores'][a:b] for a, b in cut],
                'descriptors': [res['descriptors'][a:b].t() for a, b in cut]}


class DenseExtractor(DenseExtractorPluginMixin, _BaseModel):
    """The stand-alone form: nothing of the reference needs to be importable.  ``net``: the torch module."""

    def __init__(self, conf, model_path=None, net=None):
        super().__init__(conf, model_path)
        if net is None:
            raise ValueError('DenseExtractor needs `net`: a torch module net(image) -> (scores [B,H,W], descriptors [B,D,h,w])')
        self.net = net
