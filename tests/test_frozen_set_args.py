"""CPU: the argument checks of alphazero.pool_unique / azmi_pool_unique that are made before any device is touched."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


def test_no_records_need_no_device(az):
    first, dups = az.pool_unique(np.zeros(0, np.uint64))
    assert first.dtype == np.uint32 and first.size == 0 and dups == 0
    first, dups = az.pool_unique([], valid=[])
    assert first.size == 0 and dups == 0


def test_a_record_count_the_table_cannot_hold_is_refused_by_name(az):
    nu, nd = C.c_uint32(7), C.c_uint32(7)
    one = np.zeros(1, np.uint64)
    out = np.zeros(1, np.uint32)
    for n in ((1 << 30) + 1, 0xFFFFFFFF):      # nothing is read: the count is checked first
        rc = az.lib.azmi_pool_unique(one.ctypes.data, None, n, out.ctypes.data, C.byref(nu), C.byref(nd), 0, None)
        assert rc == -1
        msg = az.lib.azmi_last_error().decode()
        assert f"n = {n} records" in msg and "at most 1073741824 records" in msg


def test_null_and_shape_arguments(az):
    one = np.zeros(1, np.uint64)
    out = np.zeros(1, np.uint32)
    nu, nd = C.c_uint32(), C.c_uint32()
    for args in ((None, None, 1, out.ctypes.data, C.byref(nu), C.byref(nd)), (one.ctypes.data, None, 1, None, C.byref(nu), C.byref(nd)),
                 (one.ctypes.data, None, 1, out.ctypes.data, None, C.byref(nd)), (one.ctypes.data, None, 0, out.ctypes.data, C.byref(nu), None)):
        assert az.lib.azmi_pool_unique(*args, 0, None) == -1
        assert "azmi_pool_unique: null argument" in az.lib.azmi_last_error().decode()
    with pytest.raises(RuntimeError, match="one valid flag per key"):
        az.pool_unique(np.arange(4, dtype=np.uint64), np.ones(3, bool))
    with pytest.raises(RuntimeError, match="one-dimensional"):
        az.pool_unique(np.zeros((2, 2), np.uint64))


def test_records_without_a_device_fail_loudly(az):
    import torch
    if torch.cuda.is_available():
        return      # the GPU suite covers the call itself
    with pytest.raises(RuntimeError, match="no HIP device"):
        az.pool_unique(np.arange(4, dtype=np.uint64))
