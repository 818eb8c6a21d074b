"""The input seam the depth-and-pose wrappers share (``covis_set``, ``match_score``, ``keypoint_score``,
``match_assembly``): host or device inputs turned into the checked device tensors a HIP entry takes.

Host inputs (lists, numpy arrays, CPU tensors) are uploaded with BLOCKING copies from memory that outlives
them; only ``_pair_tensor(..., pin=True)`` pins memory.  Private: the public names live in the feature modules.
"""
import numpy as np
import torch

from .hip_engine import MATCH_SCORE_PARAM_DOUBLES


def _is_host(x):
    return not (torch.is_tensor(x) and x.is_cuda)


def _dtype_of(x):
    return x.dtype if torch.is_tensor(x) else np.asarray(x).dtype


def _refuse_float64(name, k):
    if _dtype_of(k) in (torch.float64, np.dtype(np.float64)):
        raise ValueError(f'{name} is float64: the score is defined on float32 keypoints (widened exactly); rounding '
                         'float64 keypoints here would change the score. Convert them to float32 yourself.')


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
