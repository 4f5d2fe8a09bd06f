"""Compaction, the host side (no GPU): bsr_index_compact is exported, rejects a null index with a
message, and the Python wrapper rejects a global_offset that is no non-negative integer below 2^64
before calling the library."""
import ctypes

import numpy as np
import pytest

E_INVALID = -1


def test_symbol_exported(bsr_mod):
    assert hasattr(bsr_mod.lib(), "bsr_index_compact")
    assert bsr_mod.BSR_COMPACT_SHRINK == 1


def test_null_index(bsr_mod):
    L = bsr_mod.lib()
    ids = np.zeros(4, np.uint64)
    cnt = ctypes.c_uint64(77)
    assert L.bsr_index_compact(None, 0, 0, ids.ctypes.data, 4, ctypes.byref(cnt)) == E_INVALID
    assert b"null index" in L.bsr_last_error()
    assert cnt.value == 77 and not ids.any()
    assert L.bsr_index_compact(None, 5, bsr_mod.BSR_COMPACT_SHRINK, None, 0, None) == E_INVALID
    assert b"null index" in L.bsr_last_error()


class _NoLibrary:
    """Stands where the library would: reaching it is the failure."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library")


@pytest.mark.parametrize("offset", [-1, -2 ** 63, 2 ** 64, 1.0, 2.5, np.float32(3), "7", True, np.bool_(False), [1],
                                    np.array([1, 2])])
def test_wrapper_rejects_bad_offset(bsr_mod, monkeypatch, offset):
    ix = bsr_mod.Index.__new__(bsr_mod.Index)  # (no device here: the check comes before any handle use)
    ix._h = None
    monkeypatch.setattr(bsr_mod, "lib", lambda: _NoLibrary())
    for shrink in (False, True):
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.compact(global_offset=offset, shrink=shrink)
        assert e.value.status == E_INVALID
