"""CPU tests of the match-list front door in ``_inputs.py``: the three steps ``score_matches``,
``score_matches_homography`` and ``estimate_poses`` share, called directly with ``dev = torch.device('cpu')`` - their
results and their messages, which are the wrappers' messages."""
import re

import numpy as np
import pytest
import torch

from imagematching_oetr_amd import _inputs

CPU = torch.device('cpu')
EXACTLY_ONE = 'give exactly one of `lengths` (host sequence) and `offsets` (device int32 [P+1])'


def raises(message):
    return pytest.raises(ValueError, match='^' + re.escape(message) + '$')


def test_lengths_become_int32_offsets():
    got = _inputs._match_offsets((3, 0, 4), None, 3, 7, CPU)
    assert got.dtype == torch.int32 and got.device == CPU and got.tolist() == [0, 3, 3, 7]
    got = _inputs._match_offsets(np.array([5]), None, 1, 5, CPU)
    assert got.dtype == torch.int32 and got.tolist() == [0, 5]
    assert _inputs._match_offsets([], None, 0, 0, CPU).tolist() == [0]


def test_given_offsets_are_uploaded_unchanged():
    got = _inputs._match_offsets(None, [2, 2, 6], 2, 9, CPU)
    assert got.dtype == torch.int32 and got.tolist() == [2, 2, 6]
    assert _inputs._match_offsets(None, torch.tensor([2, 2, 6]), 2, 9, CPU).dtype == torch.int32


@pytest.mark.parametrize('lengths, P, M', [((3, 4), 3, 7),         # a wrong count
                                           ((8, -1), 2, 7),        # a negative length
                                           ((3, 3), 2, 7)])        # a wrong sum
def test_bad_lengths_are_refused(lengths, P, M):
    with raises(f'`lengths` must hold {P} non-negative lengths summing to {M} rows'):
        _inputs._match_offsets(lengths, None, P, M, CPU)


def test_exactly_one_of_lengths_and_offsets():
    k = np.zeros((2, 2), np.float32)
    with raises(EXACTLY_ONE):
        _inputs._match_list_args(k, k, [2], torch.tensor([0, 2], dtype=torch.int32))
    with raises(EXACTLY_ONE):
        _inputs._match_list_args(k, k, None, None)
    _inputs._match_list_args(k, k, [2], None)
    _inputs._match_list_args(k, k, None, torch.tensor([0, 2], dtype=torch.int32))


def test_float64_refusal_names_the_argument():
    f32, f64 = np.zeros((2, 2), np.float32), torch.zeros(2, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match='^k1 is float64: the score is defined on float32 keypoints'):
        _inputs._match_list_args(f64, f32, [2], None)
    with pytest.raises(ValueError, match='^k2 is float64: the score is defined on float32 keypoints'):
        _inputs._match_list_args(f32, f64.numpy(), [2], None)


def test_keypoints_share_their_rows():
    k1, k2, M = _inputs._match_keypoints(np.ones((3, 2), np.float16), torch.zeros(3, 2), CPU, 'other inputs')
    assert M == 3 and k1.dtype == k2.dtype == torch.float32 and k1.tolist() == [[1.0, 1.0]] * 3
    with raises('k1 has 3 rows, k2 2'):
        _inputs._match_keypoints(torch.zeros(3, 2), torch.zeros(2, 2), CPU, 'other inputs')
    with raises('k2 must be [M,2], got (3, 3)'):
        _inputs._match_keypoints(torch.zeros(3, 2), torch.zeros(3, 3), CPU, 'other inputs')


def test_workspace_is_kept_until_it_is_too_small():
    out = {}
    first = _inputs._workspace(out, 64, CPU)
    assert first.dtype == torch.uint8 and first.numel() == 64 and out['workspace'] is first
    assert _inputs._workspace(out, 16, CPU) is first and out['workspace'] is first
    larger = _inputs._workspace(out, 65, CPU)
    assert larger.numel() == 65 and out['workspace'] is larger


def test_host_names_and_ptr():
    named = (('params', None), ('k1', np.zeros((1, 2), np.float32)), ('k2', torch.zeros(1, 2)))
    assert _inputs._host_names(named) == ['k1', 'k2']
    assert _inputs._host_names(named, lengths=[1]) == ['k1', 'k2', 'lengths']
    assert _inputs._ptr(None) is None
    assert _inputs._ptr(torch.zeros(0, 2)) is None
    t = torch.zeros(1, 2)
    assert _inputs._ptr(t) == t.data_ptr() != 0
