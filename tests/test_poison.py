"""tests/poison.py on the CPU: the three allocators fill what they return, for
every dtype, 0-size and 0-dim buffers included; the originals come back on
exit, also on error; the random pattern is seeded and does not recurse into
numpy's own np.empty calls."""
import numpy as np
import pytest
import torch

from poison import poisoned


def _bytes(x):
    if isinstance(x, torch.Tensor):
        x = x.contiguous().reshape(-1).view(torch.uint8).numpy()
        return x
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("pattern", [0x00, 0xFF, 0x5A])
def test_fixed_patterns_fill_every_dtype(pattern):
    with poisoned(pattern) as f:
        arrs = [np.empty(7, np.float32), np.empty((3, 5), np.int64), np.empty((), np.float64),
                np.empty(0, np.uint8), np.empty((2, 3), np.uint16, order="F"),
                np.empty(4, dtype=[("a", np.int32), ("b", np.float32)])]
        tens = [torch.empty(9), torch.empty((2, 3), dtype=torch.int32), torch.empty(()),
                torch.empty(0, dtype=torch.uint8), torch.empty(5, dtype=torch.bool),
                torch.empty_like(torch.zeros(4, dtype=torch.float64)),
                torch.empty(3, 4, dtype=torch.int64)]
        obj = np.empty(3, dtype=object)
    for a in arrs + tens:
        assert (_bytes(a) == pattern).all()
    assert obj.tolist() == [None, None, None]  # pointers are not bytes to overwrite
    assert f.count() == len(arrs) + len(tens)
    assert f.count("host", np.float32, 28) == 1 and f.count("host", torch.int64, 96) == 1
    assert f.count(min_bytes=1) == len(arrs) + len(tens) - 2  # the two 0-size buffers
    if pattern == 0xFF:
        assert np.isnan(arrs[0]).all() and (arrs[1] == -1).all() and torch.isnan(tens[0]).all()
        assert (tens[1] == -1).all()


def test_random_is_seeded_and_does_not_recurse():
    def draw(seed):
        with poisoned("random", seed=seed):
            return np.empty(1000, np.uint8).copy(), torch.empty(300, dtype=torch.float32).clone(), \
                np.empty((1 << 20) + 17, np.uint8)[-40:].copy()
    a, b = draw(1), draw(1)
    assert all(np.array_equal(_bytes(x), _bytes(y)) for x, y in zip(a, b))
    c = draw(2)
    assert not np.array_equal(a[0], c[0])
    assert len(set(a[0].tolist())) > 100  # bytes, not one value
    # two buffers of one size do not get the same bytes
    with poisoned("random"):
        x, y = np.empty(64, np.uint8), np.empty(64, np.uint8)
    assert not np.array_equal(x, y)


def test_originals_restored_also_on_error():
    orig = (torch.empty, torch.empty_like, np.empty)
    with pytest.raises(RuntimeError, match="inside"):
        with poisoned(0xFF):
            assert torch.empty is not orig[0] and np.empty is not orig[2]
            raise RuntimeError("inside")
    assert (torch.empty, torch.empty_like, np.empty) == orig
    with poisoned(0x00):
        pass
    assert (torch.empty, torch.empty_like, np.empty) == orig
    with pytest.raises(ValueError):
        with poisoned("zeros"):
            pass
    assert (torch.empty, torch.empty_like, np.empty) == orig


def test_guard_mode_leaves_pageable_host_buffers_alone():
    """Guard bands go around device and page-locked uint8 buffers only (the GPU
    suite checks those); everything else is filled as without the mode."""
    with poisoned(0x5A, guard=True) as f:
        u = torch.empty(100, dtype=torch.uint8)
        x = torch.empty(7)
        a = np.empty(9, np.uint8)
    assert all((_bytes(b) == 0x5A).all() for b in (u, x, a))
    assert f.guards == [] and f.assert_guards_intact() == 0 and f.count() == 3
    assert u.untyped_storage().nbytes() == 100


def test_workspace_condition():
    with poisoned(0xFF) as f:
        torch.empty(100, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="no device uint8 buffer"):
        f.assert_workspace(64, "host only")
