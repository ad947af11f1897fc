"""The device-side S3-FIFO position caches (azmi_cache_*)."""
import ctypes as C

import numpy as np

from ._capi import lib


class ShardedS3FIFOCache:
    """py_wrapper.cc:250-259 + find/insert of S3FIFOCache (:222-248), on the device (azmi_cache_*)."""

    def __init__(self, max_size, shards, ghost_size, num_policy, num_value, device=0):
        h = C.c_void_p()
        rc = lib.azmi_cache_create(max_size, shards, ghost_size, num_policy, num_value, device, C.byref(h))
        if rc != 0:
            raise RuntimeError(lib.azmi_cache_last_error().decode())
        self._h, self._np, self._nv = h, num_policy, num_value
        self._args = (int(max_size), int(shards), int(ghost_size), int(device))
        self._nominal_max = None      # set when the cache was re-laid out for an engine (see _ensure_engine_layout)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.azmi_cache_destroy(self._h)
            self._h = None

    def _ensure_engine_layout(self):
        """Called when the cache is handed to a PlayManager: the engine probes 64-entry shards, the reference's callers pass
        any `shards` (cache_utils.create_sharded_cache defaults to 1).  A cache that has not been used yet is re-created in
        the engine's layout behind the same object (capacity rounded down to a multiple of 64; max_size() keeps reporting
        the requested size, like the reference's own shard rounding; a ghost ring longer than the cache is clamped to it: a
        64-entry shard keeps at most 64 ghost keys); one that already holds entries cannot be converted."""
        max_size, shards, ghost, device = self._args
        if max_size // max(1, shards) == 64 and ghost // max(1, shards) <= 64:      # (a wave shard keeps at most 64 ghost keys)
            return
        st = self._stats()
        if st["hits"] or st["misses"] or st["size"]:
            raise RuntimeError("this cache has been used with another shard layout (max_size / shards != 64, or ghost_size / shards "
                               "> 64); create it with ShardedS3FIFOCache.for_engine before the first use to share it with a PlayManager")
        new_shards = max(1, max_size // 64)
        h = C.c_void_p()
        ghost = max(0, min(ghost, new_shards * 64))
        rc = lib.azmi_cache_create(new_shards * 64, new_shards, ghost, self._np, self._nv, device, C.byref(h))
        if rc != 0:
            raise RuntimeError(lib.azmi_cache_last_error().decode())
        lib.azmi_cache_destroy(self._h)
        self._h = h
        self._nominal_max = (max_size // max(1, shards)) * max(1, shards)
        self._args = (new_shards * 64, new_shards, ghost, device)

    @classmethod
    def for_engine(cls, max_size, num_policy, num_value, device=0):
        """A cache in the layout the engine probes (64-entry shards, ghost = 9/10 like play_manager.cc:195-203), to be
        passed as PlayManager(gs, params, caches=[...]) and kept from one PlayManager to the next."""
        shards = max(1, int(max_size) // 64)
        return cls(shards * 64, shards, shards * 64 * 9 // 10, num_policy, num_value, device)

    def insert_many(self, hashes, policies, values):
        h = np.ascontiguousarray(hashes, np.uint64)
        p = np.ascontiguousarray(policies, np.float32).reshape(len(h), self._np)
        v = np.ascontiguousarray(values, np.float32).reshape(len(h), self._nv)
        if lib.azmi_cache_insert_many(self._h, h.ctypes.data, p.ctypes.data, v.ctypes.data, len(h)) != 0:
            raise RuntimeError(lib.azmi_cache_last_error().decode())

    def insert(self, hash, policy, value):
        self.insert_many([hash], [policy], [value])

    def find_many(self, hashes):
        h = np.ascontiguousarray(hashes, np.uint64)
        hit = np.zeros(len(h), np.uint8)
        p = np.zeros((len(h), self._np), np.float32)
        v = np.zeros((len(h), self._nv), np.float32)
        if lib.azmi_cache_find_many(self._h, h.ctypes.data, len(h), hit.ctypes.data, p.ctypes.data, v.ctypes.data) != 0:
            raise RuntimeError(lib.azmi_cache_last_error().decode())
        return hit.astype(bool), p, v

    def find(self, hash, num_policy=None, num_value=None):
        hit, p, v = self.find_many([hash])
        return (p[0], v[0]) if hit[0] else None

    _STAT_KEYS = ("hits", "misses", "evictions", "reinserts", "size", "max_size")     # the row of azmi_cache_stats

    def _stats(self):
        out = np.zeros(len(self._STAT_KEYS), np.uint64)
        lib.azmi_cache_stats(self._h, out.ctypes.data)
        return dict(zip(self._STAT_KEYS, (int(x) for x in out)))

    def hits(self): return self._stats()["hits"]
    def misses(self): return self._stats()["misses"]
    def evictions(self): return self._stats()["evictions"]
    def reinserts(self): return self._stats()["reinserts"]
    def size(self): return self._stats()["size"]
    def max_size(self): return self._nominal_max if self._nominal_max is not None else self._stats()["max_size"]


def S3FIFOCache(max_size, ghost_size, num_policy, num_value, device=0):
    """py_wrapper.cc:222-248 — the single-shard cache."""
    return ShardedS3FIFOCache(max_size, 1, ghost_size, num_policy, num_value, device)
