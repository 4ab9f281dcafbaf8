"""depth_mask_images reads a size group of maps in place only when they share one storage: maps of separate storages that happen to lie back to
back in memory (the caching allocator carves small blocks from one segment) are stacked instead. torch.frombuffer gives two such tensors on the
CPU deterministically."""
import numpy as np
import torch

from muggled_dpt_amd import postprocess as pp


def test_adjacent_maps_of_separate_storages_are_stacked():
    buf = np.arange(2 * 16 * 16, dtype=np.float32)
    a = torch.frombuffer(memoryview(buf[:256]), dtype=torch.float32).view(16, 16)
    b = torch.frombuffer(memoryview(buf[256:]), dtype=torch.float32).view(16, 16)
    assert b.data_ptr() == a.data_ptr() + a.numel() * 4 and a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
    x = pp._size_group_batch([a, b])
    assert x.shape == (2, 16, 16) and torch.equal(x[0], a) and torch.equal(x[1], b)
    assert x.untyped_storage().data_ptr() not in (a.untyped_storage().data_ptr(), b.untyped_storage().data_ptr())


def test_rows_of_one_tensor_are_read_in_place():
    t = torch.rand(3, 8, 5)
    x = pp._size_group_batch(list(t.unbind(0)))
    assert x.data_ptr() == t.data_ptr() and torch.equal(x, t)
    y = pp._size_group_batch([t[0], t[2]])  # one storage, not back to back: a copy
    assert y.data_ptr() != t.data_ptr() and torch.equal(y, t[[0, 2]])
