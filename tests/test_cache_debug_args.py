"""CPU: azmi_debug_cache_find_group / azmi_debug_cache_insert_locked (the cache's probe groups and the pipeline's locked insert on
their own, tests/test_gpu_cache_edges.py) are in the ctypes table and check their arguments on the host before they look for a
device.  A cache object cannot be made without a device; where a check needs one to look at, a block of zeros stands in - a
cache of capacity 0, which is in no layout.  The refusals that need a real cache (num_policy > 64, a ghost ring longer than a
wave shard - also the engines' own refusal of such a cache) are pinned by their text in
tests/test_gpu_cache_edges.py::test_debug_entry_points_refuse_what_they_do_not_cover and
::test_engines_refuse_a_ghost_ring_longer_than_a_wave_shard."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from alphazero import _capi
    return _capi


def _err(capi):
    return capi.lib.azmi_cache_last_error().decode()


def _buffers(n=4):
    keys = np.arange(1, n + 1, dtype=np.uint64)
    hit = np.zeros(n, np.uint8)
    pol, val = np.zeros((n, 7), np.float32), np.zeros((n, 3), np.float32)
    return keys, hit, pol, val


def test_symbols_are_in_the_ctypes_table(capi):
    vp, u32 = C.c_void_p, C.c_uint32
    assert capi.SYMBOLS["azmi_debug_cache_find_group"] == (C.c_int, [vp, u32, vp, u32, vp, vp, vp])
    assert capi.SYMBOLS["azmi_debug_cache_insert_locked"] == (C.c_int, [vp, vp, vp, vp, u32, u32, C.POINTER(u32)])
    assert capi.lib.azmi_abi_version() == 1          # the entry points are additive
    from alphazero import drivers
    assert callable(drivers.cache_find_group) and callable(drivers.cache_insert_locked)


def test_null_arguments_are_an_error_not_a_crash(capi):
    zeros = np.zeros(4096, np.uint8)                 # stands in for a cache; never looked at before the null checks
    keys, hit, pol, val = _buffers()
    args = [zeros.ctypes.data, 8, keys.ctypes.data, 4, hit.ctypes.data, pol.ctypes.data, val.ctypes.data]
    for missing in (0, 2, 4, 5, 6):
        a = list(args); a[missing] = None
        assert capi.lib.azmi_debug_cache_find_group(*a) == -1
        assert _err(capi) == "azmi_debug_cache_find_group: null argument"
    failed = C.c_uint32(7)
    args = [zeros.ctypes.data, keys.ctypes.data, pol.ctypes.data, val.ctypes.data, 4, 2, C.byref(failed)]
    for missing in (0, 1, 2, 3, 6):
        a = list(args); a[missing] = None
        assert capi.lib.azmi_debug_cache_insert_locked(*a) == -1
        assert _err(capi) == "azmi_debug_cache_insert_locked: null argument"
    assert failed.value == 7


def test_nothing_to_do_succeeds_without_a_device(capi):
    zeros = np.zeros(4096, np.uint8)
    for lanes in (8, 64):
        assert capi.lib.azmi_debug_cache_find_group(zeros.ctypes.data, lanes, None, 0, None, None, None) == 0
    failed = C.c_uint32(7)
    assert capi.lib.azmi_debug_cache_insert_locked(zeros.ctypes.data, None, None, None, 0, 1, C.byref(failed)) == 0
    assert failed.value == 0


def test_refusals_by_their_text(capi):
    zeros = np.zeros(4096, np.uint8)
    keys, hit, pol, val = _buffers()
    for lanes in (0, 1, 16, 32, 63, 128):            # before n == 0 and before the cache is looked at
        for n in (0, 4):
            assert capi.lib.azmi_debug_cache_find_group(zeros.ctypes.data, lanes, keys.ctypes.data, n, hit.ctypes.data, pol.ctypes.data, val.ctypes.data) == -1
            assert _err(capi) == f"azmi_debug_cache_find_group: group_lanes {lanes} is not a lane group of the engines (8 or 64)"
    failed = C.c_uint32(7)
    for waves in (0, 8193):
        assert capi.lib.azmi_debug_cache_insert_locked(zeros.ctypes.data, keys.ctypes.data, pol.ctypes.data, val.ctypes.data, 4, waves, C.byref(failed)) == -1
        assert _err(capi) == "azmi_debug_cache_insert_locked: waves must be 1 .. 8192"
    # a cache that is not laid out in 64-entry wave shards (here: capacity 0)
    assert capi.lib.azmi_debug_cache_find_group(zeros.ctypes.data, 64, keys.ctypes.data, 4, hit.ctypes.data, pol.ctypes.data, val.ctypes.data) == -1
    assert _err(capi) == "azmi_debug_cache_find_group: not a cache of 64-entry wave shards (max_size / shards = 0, ghost_size / shards = 0)"
    assert capi.lib.azmi_debug_cache_insert_locked(zeros.ctypes.data, keys.ctypes.data, pol.ctypes.data, val.ctypes.data, 4, 2, C.byref(failed)) == -1
    assert _err(capi) == "azmi_debug_cache_insert_locked: not a cache of 64-entry wave shards (max_size / shards = 0, ghost_size / shards = 0)"
    assert not zeros.any()
