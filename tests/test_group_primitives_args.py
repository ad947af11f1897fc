"""CPU: azmi_debug_group_select (the descent's lane-group primitives on their own, tests/test_gpu_group_primitives.py) is in the
ctypes table and checks its arguments on the host before it looks for a device."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from alphazero import _capi
    return _capi


def test_symbol_is_in_the_ctypes_table(capi):
    assert "azmi_debug_group_select" in capi.SYMBOLS
    restype, argtypes = capi.SYMBOLS["azmi_debug_group_select"]
    assert restype is C.c_int and len(argtypes) == 14
    assert capi.lib.azmi_abi_version() == 1          # the entry point is additive


def test_none_buffers_are_an_error_not_a_crash(capi):
    bufs = [np.zeros(64, np.uint32) for _ in range(12)]
    ptrs = [b.ctypes.data_as(C.c_void_p) for b in bufs]
    for missing in range(12):
        args = list(ptrs)
        args[missing] = None
        assert capi.lib.azmi_debug_group_select(0, 1, *args) == -1
        assert "null buffer" in capi.lib.azmi_last_error().decode()
    with pytest.raises(RuntimeError, match="null buffer"):
        capi.check(capi.lib.azmi_debug_group_select(0, 1, *([None] * 12)))
    assert capi.lib.azmi_debug_group_select(0, 0, *ptrs) == -1
    assert "rows" in capi.lib.azmi_last_error().decode()
