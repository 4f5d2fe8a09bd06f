"""In-place update, the host side (no GPU): bsr_index_update is exported and declared with its
signature, rejects a null index without a device, and the Python wrapper rejects ids and rows that
do not match before calling the library."""
import os
import re

import numpy as np
import pytest

E_INVALID, E_DIM = -1, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported(bsr_mod):
    assert hasattr(bsr_mod.lib(), "bsr_index_update")
    assert hasattr(bsr_mod.Index, "update")


def test_declared_in_header():
    with open(os.path.join(ROOT, "include", "bsr.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert ("int bsr_index_update(bsr_index* ix, const uint64_t* ids, const void* rows, uint64_t n_ids);"
            in text)


def test_null_index(bsr_mod):
    L = bsr_mod.lib()
    ids = np.zeros(4, np.uint64)
    rows = np.zeros((4, 8), np.float32)
    assert L.bsr_index_update(None, ids.ctypes.data, rows.ctypes.data, 4) == E_INVALID
    assert b"null index" in L.bsr_last_error()
    assert L.bsr_index_update(None, None, None, 0) == E_INVALID


class _NoLibrary:
    """Stands where the library would: reaching it is the failure."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library")


def _index(bsr_mod, monkeypatch, dim=8, dtype=None):
    ix = bsr_mod.Index.__new__(bsr_mod.Index)  # (no device here: the checks come before any handle use)
    ix._h, ix.dim, ix.max_k = None, dim, 64
    ix.dtype = bsr_mod.BSR_F32 if dtype is None else dtype
    monkeypatch.setattr(bsr_mod, "lib", lambda: _NoLibrary())
    return ix


@pytest.mark.parametrize("ids,shape,status", [
    ([1, 2, 3], (2, 8), E_INVALID),       # fewer rows than ids
    ([1], (2, 8), E_INVALID),             # more rows than ids
    ([], (1, 8), E_INVALID),
    ([1, 2], (8,), E_INVALID),            # one row for two ids
    ([1, 2], (2, 7), E_DIM),              # a row length other than dim
    ([1, 2], (2, 9), E_DIM),
])
def test_wrapper_rejects_mismatched_shapes(bsr_mod, monkeypatch, ids, shape, status):
    ix = _index(bsr_mod, monkeypatch)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.update(np.asarray(ids, np.int64), np.zeros(shape, np.float32))
    assert e.value.status == status


@pytest.mark.parametrize("ids", [[1.5, 2.0], ["a", "b"], [-1, 2], np.array([3, -7])])
def test_wrapper_rejects_bad_ids(bsr_mod, monkeypatch, ids):
    ix = _index(bsr_mod, monkeypatch)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.update(ids, np.zeros((2, 8), np.float32))
    assert e.value.status == E_INVALID


def test_wrapper_rejects_bad_tensors(bsr_mod, monkeypatch):
    import torch
    ix = _index(bsr_mod, monkeypatch)
    ids = torch.tensor([1, 2])
    for rows in (torch.zeros((3, 8)), torch.zeros((2, 7)), torch.zeros((2, 8), dtype=torch.float64),
                 torch.zeros((2, 16))[:, ::2]):
        with pytest.raises(bsr_mod.BsrError):
            ix.update(ids, rows)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.update(torch.tensor([1, 2], dtype=torch.int32), torch.zeros((2, 8)))
    assert e.value.status == E_INVALID
    # a bf16 index takes 2-byte elements
    ix = _index(bsr_mod, monkeypatch, dtype=bsr_mod.BSR_BF16)
    with pytest.raises(bsr_mod.BsrError):
        ix.update(ids, torch.zeros((2, 8)))
