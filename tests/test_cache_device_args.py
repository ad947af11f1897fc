"""CPU: what the device-pointer cache entries (azmi_cache_find_rows, azmi_cache_insert_rows, azmi_net_forward_cached,
azmi_search_leaf_keys) and the Python layer over them answer without a device: the ctypes table, null arguments by name, n == 0,
and the dtype / shape / contiguity checks of alphazero._args.device_tensor, which judges a tensor before it asks where it lives.
A cache or a net cannot be made without a device; where a check needs one to hold, a block of zeros stands in and is never
looked at (tests/test_cache_debug_args.py does the same).  The refusals that need real objects - a cache of another shape than
the net, host and device arguments mixed - are in tests/test_gpu_cache_device.py."""
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


def test_symbols_are_in_the_ctypes_table(capi):
    vp, u32 = C.c_void_p, C.c_uint32
    assert capi.SYMBOLS["azmi_cache_find_rows"] == (C.c_int, [vp, vp, u32, vp, vp, vp, vp, vp, vp])
    assert capi.SYMBOLS["azmi_cache_insert_rows"] == (C.c_int, [vp, vp, vp, vp, vp, vp, u32, vp])
    assert capi.SYMBOLS["azmi_net_forward_cached"] == (C.c_int, [vp, vp, vp, vp, u32, vp, vp, vp, vp])
    assert capi.SYMBOLS["azmi_search_leaf_keys"] == (C.c_int, [vp, vp, C.POINTER(C.c_void_p), C.POINTER(u32)])
    assert capi.lib.azmi_abi_version() == 1          # the entry points are additive
    import alphazero
    assert callable(alphazero.cached_forward) and callable(alphazero.ShardedS3FIFOCache.find_rows) and callable(alphazero.MCTSBatch.leaf_keys)


def test_null_arguments_are_named(capi):
    zeros = np.zeros(4096, np.uint8)                 # stands in for a cache / a net; never looked at before the null checks
    buf = np.zeros(64, np.uint64)
    z, b = zeros.ctypes.data, buf.ctypes.data
    find = [z, b, 4, b, b, b, b, b, None]
    for at, name in ((0, "cache"), (1, "d_keys"), (3, "d_hit"), (4, "d_pi"), (5, "d_v")):
        a = list(find); a[at] = None
        assert capi.lib.azmi_cache_find_rows(*a) == -1
        assert _err(capi) == f"azmi_cache_find_rows: null argument: {name}"
    for at in (6, 7):                                # the miss list and its count go together
        a = list(find); a[at] = None
        assert capi.lib.azmi_cache_find_rows(*a) == -1
        assert "d_miss_rows and d_miss_count go together" in _err(capi)
    insert = [z, b, b, b, b, b, 4, None]
    for at, name in ((0, "cache"), (1, "d_keys"), (2, "d_pi"), (3, "d_v")):
        a = list(insert); a[at] = None
        assert capi.lib.azmi_cache_insert_rows(*a) == -1
        assert _err(capi) == f"azmi_cache_insert_rows: null argument: {name}"
    cached = [z, z, b, b, 4, b, b, b, None]
    for at, name in ((0, "net"), (1, "cache"), (2, "d_canon"), (3, "d_keys"), (5, "d_v"), (6, "d_pi"), (7, "d_hit")):
        a = list(cached); a[at] = None
        assert capi.lib.azmi_net_forward_cached(*a) == -1
        assert _err(capi) == f"azmi_net_forward_cached: null argument: {name}"
    n = (1 << 30) + 1                                # more rows than a call takes: refused before the device is looked for
    assert capi.lib.azmi_cache_find_rows(z, b, n, b, b, b, None, None, None) == -1 and "at most 2^30 rows" in _err(capi)
    assert capi.lib.azmi_cache_insert_rows(z, b, b, b, None, None, n, None) == -1 and "at most 2^30 rows" in _err(capi)
    keys, rows = C.c_void_p(5), C.c_uint32(7)
    assert capi.lib.azmi_search_leaf_keys(None, None, C.byref(keys), C.byref(rows)) == -1
    assert "leaf_keys: null argument" in capi.lib.azmi_last_error().decode() and (keys.value, rows.value) == (5, 7)
    assert not zeros.any() and not buf.any()


def test_nothing_to_do_succeeds_without_a_device(capi):
    zeros = np.zeros(4096, np.uint8)
    z = zeros.ctypes.data
    assert capi.lib.azmi_cache_find_rows(z, None, 0, None, None, None, None, None, None) == 0
    assert capi.lib.azmi_cache_insert_rows(z, None, None, None, None, None, 0, None) == 0
    assert capi.lib.azmi_net_forward_cached(z, z, None, None, 0, None, None, None, None) == 0
    assert not zeros.any()


def test_tensor_checks_name_the_argument_before_any_device(capi):
    torch = pytest.importorskip("torch")
    from alphazero import _args
    keys = torch.arange(8, dtype=torch.int64)
    ok = (("torch.int64", "torch.uint64"), (None,))
    cases = [
        (np.arange(8), "keys", ok, "keys must be a CUDA tensor"),                                    # a host array
        (keys.to(torch.int32), "keys", ok, "keys must be int64 or uint64, got int32"),
        (torch.arange(16, dtype=torch.int64)[::2], "keys", ok, "keys must be contiguous"),
        (keys.reshape(2, 4), "keys", ok, r"keys must have shape \[n\], got \[2, 4\]"),
        (torch.zeros((8, 7), dtype=torch.float64), "policies", (("torch.float32",), (8, 7)), "policies must be float32, got float64"),
        (torch.zeros((8, 6)), "policies", (("torch.float32",), (8, 7)), r"policies must have shape \[8, 7\], got \[8, 6\]"),
        (torch.zeros((7, 8)).t(), "values", (("torch.float32",), (8, 7)), "values must be contiguous"),
        (torch.zeros(3), "rows", (("torch.int32", "torch.uint32"), (None,)), "rows must be int32 or uint32, got float32"),
        (torch.zeros(2, dtype=torch.int32), "row_count", (("torch.int32", "torch.uint32"), (1,)), r"row_count must have shape \[1\], got \[2\]"),
        (keys, "keys", ok, "keys must be a CUDA tensor like the keys .* got a cpu tensor"),          # well-formed, but on the host
    ]
    for x, name, (dtypes, shape), text in cases:
        with pytest.raises(RuntimeError, match="insert_many: " + text):
            _args.device_tensor(x, "insert_many", name, dtypes, shape, 0)
    assert _args.is_tensor(keys) and not _args.is_device_tensor(keys) and not _args.is_tensor(np.arange(3)) and not _args.is_tensor([1, 2])
