"""The input seam the evaluation wrappers share (``covis``, ``covis_set``, ``match_score``, ``keypoint_score``,
``match_assembly``, ``homography``, ``pose_ransac``): host or device inputs turned into the checked device tensors a
HIP entry takes.  The front door of the entries that take match lists - ``k1`` / ``k2`` ``[M,2]`` cut into one list
per pair by ``lengths`` or ``offsets`` - is here once, in three steps (``_match_list_args``, ``_match_keypoints``,
``_match_offsets``) because its callers learn the number of pairs at different moments.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that outlives
them; only ``_pair_tensor(..., pin=True)`` pins memory.  Private: the public names live in the feature modules.
"""
import numpy as np
import torch

from .hip_engine import MATCH_SCORE_PARAM_DOUBLES


NO_CPU = 'There is no CPU implementation.'


def _is_host(x):
    return not (torch.is_tensor(x) and x.is_cuda)


def _device_of(what, tensors):
    """The GPU of the first device tensor among ``tensors``, else the current GPU; raises without one."""
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError(f'{what} needs a GPU (HIP) device: the inputs are on the CPU and no GPU is present. '
                           + NO_CPU)
    return torch.device('cuda', torch.cuda.current_device())


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, 'shape') else tuple(np.asarray(x).shape)


def _ptr(t):
    """The address an entry takes for ``t``: ``None`` (NULL) for ``None`` and for an empty tensor."""
    return t.data_ptr() if t is not None and t.numel() else None


def _workspace(out, need, dev):
    """The workspace the result ``out`` carries as ``out['workspace']``, allocated afresh - and stored back - when it
    is missing or smaller than ``need`` bytes."""
    workspace = out.get('workspace')
    if workspace is None or workspace.numel() < need:
        workspace = out['workspace'] = torch.empty(need, dtype=torch.uint8, device=dev)
    return workspace


def _dtype_of(x):
    return x.dtype if torch.is_tensor(x) else np.asarray(x).dtype


def _refuse_float64(name, k):
    if _dtype_of(k) in (torch.float64, np.dtype(np.float64)):
        raise ValueError(f'{name} is float64: the score is defined on float32 keypoints (widened exactly); rounding '
                         'float64 keypoints here would change the score. Convert them to float32 yourself.')


def _host_names(named, lengths=None):
    """The names among ``named`` (``(name, input)`` pairs) whose input is on the host, for
    ``_refuse_host_inputs_in_capture``; ``lengths`` is a host input whenever it is given."""
    return [n for n, x in named if x is not None and _is_host(x)] + (['lengths'] if lengths is not None else [])


def _refuse_host_inputs_in_capture(names):
    """``names``: the inputs of a call that are on the host.  Call it with the call's device current."""
    if names and torch.cuda.is_current_stream_capturing():
        raise ValueError(f'inside a graph capture every input must be a device tensor; on the host: {names}')


def _keypoints(name, k, dev, what, align=None, rows='M'):
    """``k`` -> contiguous float32 ``[rows,2]`` on ``dev``; float16 widened; a host array is uploaded (blocking).
    ``what``: what else lives on ``dev``, for the message.  ``align``: the bytes a row must start on for a kernel
    that moves it as one vector; a view that starts elsewhere is copied."""
    if _is_host(k):
        k = torch.as_tensor(np.asarray(k) if not torch.is_tensor(k) else k)
    if k.dtype not in (torch.float32, torch.float16):
        raise ValueError(f'{name} must be float32 or float16, got {k.dtype}')
    if k.dim() != 2 or k.shape[1] != 2:
        raise ValueError(f'{name} must be [{rows},2], got {tuple(k.shape)}')
    if k.is_cuda and k.device != dev:
        raise ValueError(f'{name} is on {k.device}, the {what} on {dev}')
    k = k.to(device=dev, dtype=torch.float32).contiguous()           # from the host: a blocking copy
    return k.clone() if align and k.data_ptr() % align else k


def _upload(name, x, dtype, shape, dev):
    """A device tensor as it is (checked), a host array by a blocking copy."""
    if _is_host(x):
        x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(dtype).reshape(shape).to(dev)
    if x.dtype != dtype or tuple(x.shape) != tuple(shape) or x.device != dev:
        raise ValueError(f'{name} must be a {dtype} tensor of shape {tuple(shape)} on {dev}')
    return x.contiguous()


def _offsets_of(lengths, dev):
    """Host lengths -> their int32 ``[len + 1]`` offsets on ``dev`` (summed in int64; a blocking copy)."""
    return torch.as_tensor(np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int32)).to(dev)


def _match_list_args(k1, k2, lengths, offsets):
    """What a match-list entry refuses before it looks for a device."""
    if (lengths is None) == (offsets is None):
        raise ValueError('give exactly one of `lengths` (host sequence) and `offsets` (device int32 [P+1])')
    _refuse_float64('k1', k1)
    _refuse_float64('k2', k2)


def _match_keypoints(k1, k2, dev, what):
    """``k1``, ``k2`` -> ``(k1, k2, M)``: both through ``_keypoints``, with the ``M`` rows they share."""
    k1, k2 = _keypoints('k1', k1, dev, what), _keypoints('k2', k2, dev, what)
    M = int(k1.shape[0])
    if int(k2.shape[0]) != M:
        raise ValueError(f'k1 has {M} rows, k2 {int(k2.shape[0])}')
    if M > 2 ** 31 - 1:
        raise ValueError('more than 2^31 - 1 matches in one call')
    return k1, k2, M


def _match_offsets(lengths, offsets, P, M, dev):
    """The int32 ``[P+1]`` offsets on ``dev`` of ``P`` lists over ``M`` rows: of checked host ``lengths``, or the
    ``offsets`` given (a device tensor as it is, a host array uploaded)."""
    if lengths is None:
        return _upload('offsets', offsets, torch.int32, (P + 1,), dev)
    lengths = [int(n) for n in lengths]
    if len(lengths) != P or any(n < 0 for n in lengths) or sum(lengths) != M:
        raise ValueError(f'`lengths` must hold {P} non-negative lengths summing to {M} rows')
    return _offsets_of(lengths, dev)


def _pair_tensor(dev, pair_index, pin=False):
    """``pair_index`` -> int32 ``[P,2]`` on ``dev``: a device tensor is taken as it is (checked), a host sequence
    is uploaded - blocking, or with ``pin`` from pinned memory without waiting."""
    if _is_host(pair_index):
        host = torch.as_tensor(np.asarray(pair_index, dtype=np.int32).reshape(-1, 2))
        return host.pin_memory().to(dev, non_blocking=True) if pin and host.numel() else host.to(dev)
    if pair_index.dtype != torch.int32 or pair_index.dim() != 2 or pair_index.shape[1] != 2 or pair_index.device != dev:
        raise ValueError(f'a device pair_index must be int32 [P,2] on {dev}')
    return pair_index


def _pair_blocks(depth_set, pair_index, params, default_params):
    """What a scoring entry takes of its ``P >= 1`` pairs: ``idx1``, ``idx2`` contiguous int32 ``[P]`` split out of
    the device ``pair_index``, the set's committed table, and the float64 ``[P,20]`` blocks - ``params`` checked
    (a host array uploaded), or ``default_params(depth_set, idx1, idx2)`` for ``None``."""
    idx1, idx2 = pair_index[:, 0].contiguous(), pair_index[:, 1].contiguous()
    table, _ = depth_set._commit()
    if params is None:
        params = default_params(depth_set, idx1, idx2)
    else:
        params = _upload('params', params, torch.float64, (int(pair_index.shape[0]), MATCH_SCORE_PARAM_DOUBLES),
                         pair_index.device)
    return idx1, idx2, table, params
