"""executor._stacked: the stacked [left; right] feature batch is a view only where both
halves lie in ONE storage.  Two separate tensors with adjacent addresses (the caching
allocator places equal-sized allocations back to back) must be copied: a view of the
first cannot span the second's storage."""
import numpy as np
import torch

from leastereo_amd.executor import _stacked


def test_slices_of_one_tensor_are_stacked_as_a_view():
    f = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).view(2, 3, 4, 5)
    s = _stacked(f[:1], f[1:])
    assert s.data_ptr() == f.data_ptr() and torch.equal(s, f)


def test_adjacent_tensors_of_two_storages_are_copied():
    n = 3 * 4 * 5
    a = np.arange(2 * n, dtype=np.float32)
    fl = torch.from_numpy(a[:n]).view(1, 3, 4, 5)   # two storages of n floats each,
    fr = torch.from_numpy(a[n:]).view(1, 3, 4, 5)   # the second directly after the first
    assert fr.data_ptr() == fl.data_ptr() + 4 * n
    assert fl.untyped_storage().data_ptr() != fr.untyped_storage().data_ptr()
    s = _stacked(fl, fr)
    assert s.shape == (2, 3, 4, 5) and torch.equal(s, torch.cat((fl, fr), 0))
    assert s.data_ptr() != fl.data_ptr()
