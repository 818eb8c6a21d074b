"""Matcher output assembled into origin-frame match lists on the device, for a whole pair list per call.

Between ``overlap_crop_batch`` and ``score_matches`` stands the tail of the reference's ``process()``
(``dloc/core/overlap_features.py:118-155``): keypoints found in the crops go back into the original
pictures, ``(keypoints / ratio + bbox[:2]) * scales``, and ``matches0`` becomes lists,
``index0 = nonzero(matches > -1)``, ``index1 = matches[valid]``, ``mconf = conf[valid]``.
:func:`assemble_matches` does both for every pair of a call in one HIP call
(``oetr_assemble_matches``, ``include/oetr_match_assembly.h``, ``csrc/match_assembly.hip``) that reads
the geometry records where ``overlap_crop_batch`` left them - on the device - and returns float32
lists ``score_matches`` takes as they are.  The arithmetic is the numpy specification of DESIGN 9.3h,
reproduced bit for bit.  There is no CPU implementation; ``OverlapCropBatch.to_origin`` remains the
host route for a single pair.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that
outlives them; nothing here pins memory.  Inside a graph capture every input must already be a device
tensor.
"""
import ctypes as C

import numpy as np
import torch

from . import hip_engine
from ._inputs import (_host_names, _is_host, _keypoints, _offsets_of, _ptr, _refuse_float64,
                      _refuse_host_inputs_in_capture, _upload)
from .crop_batch import OverlapCropBatch
from .hip_engine import MATCH_ASSEMBLY_COUNTERS, _check, _CropInfo, _stream

_INFO_BYTES = C.sizeof(_CropInfo)


def _device_of(crops):
    return crops.info.device if isinstance(crops, OverlapCropBatch) else crops.device


def _join(name, seq, dev):
    """A sequence with one tensor per pair -> (the tensors joined on ``dev``, their lengths).  Lengths come from the
    shapes: nothing is read."""
    parts = [torch.as_tensor(np.asarray(t)) if not torch.is_tensor(t) else t for t in seq]
    if not parts:
        raise ValueError(f'{name}: an empty sequence')
    return torch.cat([t.to(dev) for t in parts]), [int(t.shape[0]) for t in parts]


@torch.no_grad()
def assemble_matches(crops, scales, kp0, kp1, matches, conf=None, offsets0=None, offsets1=None, min_matches=30,
                     out=None):
    """Origin-frame keypoints and match lists of all pairs of a crop call, in one device call.

    ``crops``: an ``OverlapCropBatch`` (its records are used where they are, no read) or a device tensor
    that holds ``P`` ``oetr_crop_info`` records.  ``scales``: float64 ``[P,2,2]`` - per pair the
    reader's ``scales0`` and ``scales1`` ``(sx, sy)``.  Keypoints and matches come in one of two forms:

    * sequences with one tensor per pair - ``kp0[p]`` ``[K0_p,2]``, ``kp1[p]`` ``[K1_p,2]``, ``matches[p]``
      ``[K0_p]`` (the matcher's ``matches0``), ``conf[p]`` ``[K0_p]``: the lengths come from the shapes,
      the tensors are joined on the device;
    * joined, with ``offsets0`` / ``offsets1``: device int32 ``[P+1]``, non-decreasing; side ``i`` of
      pair ``p`` owns rows ``offsets_i[p] .. offsets_i[p+1]-1``.  This is the form a graph can capture.

    Keypoints are float32 in CROP coordinates (float16 is widened; float64 is refused), matches int32 or
    int64 (taken as they are): row ``a`` of pair ``p`` holds ``b``, an index within side 1 of pair ``p``,
    or a negative value.  ``conf``: float32 ``matching_scores0`` or None.

    Returns a dict of device tensors.  ``origin0`` ``[N0,2]`` / ``origin1`` ``[N1,2]`` float64: what
    ``keypoints_to_origin`` gives, pair by pair.  ``index0``, ``index1`` int32 ``[N0]``, ``k1``, ``k2``
    float32 ``[N0,2]`` (the origin keypoints of each kept match, rounded to float32), ``mconf`` float32
    ``[N0]`` (with ``conf``): the lists pair after pair, list ``p`` in rows
    ``offsets[p] .. offsets[p+1]-1`` (``offsets`` int32 ``[P+1]``); rows from ``offsets[P]`` on are
    written ``-1`` / NaN by every call.  ``counts`` int32 ``[P,4]``: ``K0``, ``K1``, kept, rejected (a
    match ``>= K1_p`` is dropped and counted); four ``-1`` and an empty list for a pair whose crops were
    not made (``valid == -1``; its origin rows are NaN).  ``few`` int32 ``[P]`` / ``n_few`` int32 ``[1]``:
    the pairs with fewer than ``min_matches`` kept matches or not assembled, in list order, the ones the
    reference runs again without crops (``min_matches=None``: no selection); :func:`few_match_pairs`
    reads them.

    ``score_matches(ds, pair_index, res['k1'], res['k2'], offsets=res['offsets'])`` scores the result as
    it is.  Enqueues on torch's current stream of the records' device and reads nothing back.  ``out``:
    the result of an earlier call of the same sizes, written into again with no allocation."""
    joined = torch.is_tensor(kp0) or isinstance(kp0, np.ndarray)
    if joined:
        if offsets0 is None or offsets1 is None:
            raise ValueError('joined keypoints need `offsets0` and `offsets1` (int32 [P+1]); or give one tensor per pair')
        _refuse_float64('kp0', kp0)
        _refuse_float64('kp1', kp1)
    else:
        if offsets0 is not None or offsets1 is not None:
            raise ValueError('`offsets0` / `offsets1` go with joined keypoints, not with one tensor per pair')
        if not (len(kp0) == len(kp1) == len(matches)) or (conf is not None and len(conf) != len(kp0)):
            raise ValueError('kp0, kp1, matches (and conf) must hold one tensor per pair')
        for name, seq in (('kp0', kp0), ('kp1', kp1)):
            for t in seq:
                _refuse_float64(name, t)
    dev = torch.device(_device_of(crops))
    if dev.type != 'cuda':
        raise RuntimeError(f'assemble_matches needs the geometry records on a GPU (HIP) device, got {dev}. There is no '
                           'CPU implementation.')
    info = crops.info if isinstance(crops, OverlapCropBatch) else crops
    named = [('scales', scales), ('offsets0', offsets0), ('offsets1', offsets1)]
    if joined:
        named += [('kp0', kp0), ('kp1', kp1), ('matches', matches), ('conf', conf)]
    host_inputs = _host_names(named)
    if not joined:
        host_inputs.append('per-pair lengths')
        host_inputs += [n for n, seq in (('kp0', kp0), ('kp1', kp1), ('matches', matches), ('conf', conf))
                        if seq is not None and any(_is_host(t) for t in seq)]
    with torch.cuda.device(dev):
        _refuse_host_inputs_in_capture(host_inputs)
        if not joined:
            kp0, len0 = _join('kp0', kp0, dev)
            kp1, len1 = _join('kp1', kp1, dev)
            matches, len_m = _join('matches', matches, dev)
            if len_m != len0:
                raise ValueError('matches[p] must have one entry per row of kp0[p]')
            if conf is not None:
                conf, len_c = _join('conf', conf, dev)
                if len_c != len0:
                    raise ValueError('conf[p] must have one entry per row of kp0[p]')
            P = len(len0)
            offsets0, offsets1 = _offsets_of(len0, dev), _offsets_of(len1, dev)
        else:
            P = int(offsets0.shape[0] if hasattr(offsets0, 'shape') else len(offsets0)) - 1
            offsets0 = _upload('offsets0', offsets0, torch.int32, (P + 1,), dev)
            offsets1 = _upload('offsets1', offsets1, torch.int32, (P + 1,), dev)
        if P < 1:
            raise ValueError('assemble_matches needs at least one pair')
        # rows on 8 bytes: the kernel moves a keypoint as one vector
        kp0 = _keypoints('kp0', kp0, dev, 'geometry records', align=8, rows='K')
        kp1 = _keypoints('kp1', kp1, dev, 'geometry records', align=8, rows='K')
        N0, N1 = int(kp0.shape[0]), int(kp1.shape[0])
        if max(N0, N1) > 2 ** 31 - 1:
            raise ValueError('more than 2^31 - 1 keypoints on a side in one call')
        if _is_host(matches):
            matches = torch.as_tensor(np.asarray(matches) if not torch.is_tensor(matches) else matches).to(dev)
        if matches.dtype not in (torch.int32, torch.int64) or tuple(matches.shape) != (N0,) or matches.device != dev:
            raise ValueError(f'matches must be an int32 or int64 tensor of shape ({N0},) on {dev}')
        matches = matches.contiguous()
        if matches.data_ptr() % matches.element_size():              # an int64 view of int32 storage at an odd element
            matches = matches.clone()
        if conf is not None:
            conf = _upload('conf', conf, torch.float32, (N0,), dev)
        scales = _upload('scales', scales, torch.float64, (P, 2, 2), dev)
        if not info.is_cuda or info.device != dev or not info.is_contiguous() \
                or info.numel() * info.element_size() < P * _INFO_BYTES or info.data_ptr() % 8:
            raise ValueError(f'the geometry records must be a contiguous tensor on {dev} that holds {P} records of '
                             f'{_INFO_BYTES} bytes')
        if isinstance(crops, OverlapCropBatch) and len(crops) != P:
            raise ValueError(f'the crop call has {len(crops)} pairs, the keypoints {P}')
        lib = hip_engine.load_library()
        ws_bytes = int(lib.oetr_match_assembly_workspace_bytes(P))
        select = min_matches is not None
        if out is None:
            i32 = dict(dtype=torch.int32, device=dev)
            out = {'origin0': torch.empty(N0, 2, dtype=torch.float64, device=dev),
                   'origin1': torch.empty(N1, 2, dtype=torch.float64, device=dev),
                   'index0': torch.empty(N0, **i32), 'index1': torch.empty(N0, **i32),
                   'k1': torch.empty(N0, 2, device=dev), 'k2': torch.empty(N0, 2, device=dev),
                   'offsets': torch.empty(P + 1, **i32), 'counts': torch.empty(P, MATCH_ASSEMBLY_COUNTERS, **i32),
                   '_workspace': torch.empty(ws_bytes, dtype=torch.uint8, device=dev)}
            if conf is not None:
                out['mconf'] = torch.empty(N0, device=dev)
            if select:
                out['few'], out['n_few'] = torch.empty(P, **i32), torch.empty(1, **i32)
        elif (tuple(out['origin0'].shape) != (N0, 2) or tuple(out['origin1'].shape) != (N1, 2)
              or tuple(out['offsets'].shape) != (P + 1,) or ('mconf' in out) != (conf is not None)
              or ('few' in out) != select or out['origin0'].device != dev):
            raise ValueError('`out` is the result of a call of other sizes (keypoints, pairs, conf, min_matches)')
        for name, align in (('origin0', 16), ('origin1', 16), ('k1', 8), ('k2', 8)):
            if out[name].data_ptr() % align:
                raise ValueError(f"`out['{name}']` must start on a multiple of {align} bytes (the kernel writes whole "
                                 'rows as vectors); hand back the tensors an earlier call allocated')
        _check(lib, lib.oetr_assemble_matches(
            info.data_ptr(), scales.data_ptr(), P, _ptr(kp0), offsets0.data_ptr(), N0, _ptr(kp1), offsets1.data_ptr(),
            N1, _ptr(matches), matches.element_size(), _ptr(conf), int(min_matches) if select else 0,
            out['_workspace'].data_ptr(), ws_bytes, _ptr(out['origin0']), _ptr(out['origin1']), _ptr(out['index0']),
            _ptr(out['index1']), _ptr(out['k1']), _ptr(out['k2']), _ptr(out.get('mconf')), out['offsets'].data_ptr(),
            out['counts'].data_ptr(), out['few'].data_ptr() if select else None,
            out['n_few'].data_ptr() if select else None, _stream(dev)), 'oetr_assemble_matches')
        # what the enqueued kernels read stays referenced as long as the result does
        out['_inputs'] = (crops, info, scales, kp0, kp1, offsets0, offsets1, matches, conf)
    return out


def few_match_pairs(result):
    """The pairs of an :func:`assemble_matches` result with fewer than ``min_matches`` matches or not
    assembled - the ones the reference runs again without crops - as a host list, in list order.  ONE
    read (``n_few`` and ``few`` together), which synchronises the stream."""
    if 'few' not in result:
        raise ValueError('the result was assembled with min_matches=None: there is no selection')
    both = torch.cat([result['n_few'], result['few']]).cpu().tolist()
    return both[1:1 + both[0]]
