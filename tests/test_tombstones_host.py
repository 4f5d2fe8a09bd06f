"""Tombstones, the host side (no GPU): the three entry points are exported, reject null arguments,
and the Python wrappers reject ids that are no non-negative integers before calling the library."""
import ctypes

import numpy as np
import pytest

E_INVALID = -1


def test_symbols_exported(bsr_mod):
    L = bsr_mod.lib()
    for name in ("bsr_index_delete", "bsr_index_live_count", "bsr_index_deleted_mask"):
        assert hasattr(L, name), name


def test_null_arguments(bsr_mod):
    L = bsr_mod.lib()
    ids = np.zeros(4, np.uint64)
    out = ctypes.c_uint64(77)
    assert L.bsr_index_delete(None, ids.ctypes.data, 4, ctypes.byref(out)) == E_INVALID
    assert b"null index" in L.bsr_last_error()
    assert L.bsr_index_delete(None, None, 0, None) == E_INVALID
    assert L.bsr_index_live_count(None, ctypes.byref(out)) == E_INVALID
    assert L.bsr_index_live_count(None, None) == E_INVALID
    assert L.bsr_index_deleted_mask(None, ids.ctypes.data, 4) == E_INVALID
    assert L.bsr_index_deleted_mask(None, None, 0) == E_INVALID


class _NoLibrary:
    """Stands where the index handle would: reaching the library with it is the failure."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library")


@pytest.mark.parametrize("ids", [[1.5, 2.0], np.array([0.0]), ["a"], [True, False], [-1], np.array([3, -7, 2]),
                                 [[1, 2], [3, -4]]])
def test_wrapper_rejects_bad_ids(bsr_mod, monkeypatch, ids):
    ix = bsr_mod.Index.__new__(bsr_mod.Index)  # (no device here: the checks come before any handle use)
    ix._h = None
    monkeypatch.setattr(bsr_mod, "lib", lambda: _NoLibrary())
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.delete(ids)
    assert e.value.status == E_INVALID


def test_wrapper_rejects_bad_tensors(bsr_mod, monkeypatch):
    import torch
    ix = bsr_mod.Index.__new__(bsr_mod.Index)
    ix._h = None
    monkeypatch.setattr(bsr_mod, "lib", lambda: _NoLibrary())
    for t in (torch.tensor([1.0, 2.0]), torch.tensor([1, 2], dtype=torch.int32), torch.tensor([4, -1])):
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.delete(t)
        assert e.value.status == E_INVALID
