"""dawn_index_update without a device: the argument checks come before anything touches an index."""
import numpy as np

from dawnsearch_amd import _lib


def test_update_rejects_null_arguments():
    ids = np.asarray([1, 2, 3], dtype=np.uint64)
    v = np.zeros((3, 384), dtype=np.float32)
    v[:, 0] = 1.0
    upd = np.full(3, 9, dtype=np.uintp)
    lib = _lib.lib
    assert lib.dawn_index_update(None, 3, ids.ctypes.data, v.ctypes.data, upd.ctypes.data) == _lib.ERR_INVALID_ARG
    assert lib.dawn_index_update(None, 0, None, None, None) == _lib.ERR_INVALID_ARG
    assert "NULL" in _lib.last_error()
    assert upd.tolist() == [9, 9, 9]  # (nothing written for a call that never started)
