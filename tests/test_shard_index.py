"""The cache shard of a position key: shard_of (dev_cache.h: a multiply by a constant of the cache and one correction) against
Python's integer `hash % shards`.  The host's compilation of the function runs without a GPU (azmi_debug_shard_index with
device < 0); the device's compilation - the one the probes, the locked insert and the batch insert run - is the same check
in a kernel, marked gpu.

Shard counts: what the engine creates for max_cache_size = 1, 64, 200 000 and 128 000 000 (max(1, max_cache_size / 64):
engine.hip, Cache.for_engine), i.e. 1, 1, 3125, 2 000 000, plus powers of two, 2^32 - 1 and a few odd counts the stand-alone
cache accepts.  Hashes: 0, 1, 2^64 - 1, 2^32 - 1, 2^32, m * shards - 1, m * shards, m * shards + 1 for several m (the largest m
the 64 bits hold among them), and 100 000 seeded random 64-bit values.  Every case must match."""
import ctypes as C

import numpy as np
import pytest

ENGINE_SIZES = (1, 64, 200_000, 128_000_000)
OTHER_SHARDS = (2, 3, 7, 64, 255, 1 << 16, (1 << 16) + 1, 1 << 21, 1 << 31, (1 << 31) + 1, (1 << 32) - 1)
TOP = (1 << 64) - 1


def engine_shards(max_cache_size):
    return max(1, max_cache_size // 64)


def hashes_for(shards, rng):
    hs = [0, 1, TOP, (1 << 32) - 1, 1 << 32]
    top_m = TOP // shards
    for m in (1, 2, 3, 1000, (1 << 32) // shards, (1 << 32) // shards + 1, top_m // 3, top_m - 1, top_m):
        for d in (-1, 0, 1):
            h = m * shards + d
            if 0 <= h <= TOP:
                hs.append(h)
    head = np.asarray(hs, np.uint64)
    return np.concatenate([head, rng.integers(0, 1 << 64, 100_000, dtype=np.uint64)])


def cases():
    rng = np.random.default_rng(20261020)
    out = []
    for shards in [engine_shards(m) for m in ENGINE_SIZES] + list(OTHER_SHARDS):
        h = hashes_for(shards, rng)
        want = np.asarray([int(x) % shards for x in h.tolist()], np.uint32)
        out.append((shards, h, want))
    return out


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from alphazero import _capi
    return _capi


@pytest.fixture(scope="module")
def shared_cases():
    return cases()


def run(capi, device, shards, h):
    got = np.full(len(h), 0xFFFFFFFF, np.uint32)
    capi.check(capi.lib.azmi_debug_shard_index(device, shards, h.ctypes.data_as(C.c_void_p), len(h), got.ctypes.data_as(C.c_void_p)))
    return got


def compare(shards, h, want, got):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"shards {shards}: hash {int(h[bad[0]]):#018x} -> {got[bad[0]]}, hash % shards = {want[bad[0]]} ({bad.size} of {len(h)} differ)"


def test_engine_shard_counts():
    assert [engine_shards(m) for m in ENGINE_SIZES] == [1, 1, 3125, 2_000_000]


def test_host_shard_index_is_the_remainder(capi, shared_cases):
    for shards, h, want in shared_cases:
        compare(shards, h, want, run(capi, -1, shards, h))


def test_arguments_are_checked_on_the_host(capi):
    h = np.zeros(4, np.uint64)
    out = np.zeros(4, np.uint32)
    assert capi.lib.azmi_debug_shard_index(-1, 0, h.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == -1
    assert capi.lib.azmi_debug_shard_index(-1, 5, None, 4, out.ctypes.data_as(C.c_void_p)) == -1
    assert capi.lib.azmi_debug_shard_index(-1, 5, h.ctypes.data_as(C.c_void_p), 4, None) == -1
    assert capi.lib.azmi_debug_shard_index(-1, 5, None, 0, None) == 0


@pytest.mark.gpu
def test_device_shard_index_is_the_remainder(capi, shared_cases):
    for shards, h, want in shared_cases:
        compare(shards, h, want, run(capi, 0, shards, h))
