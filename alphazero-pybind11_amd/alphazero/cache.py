"""The device-side S3-FIFO position caches (azmi_cache_*)."""
import ctypes as C

import numpy as np

from . import _args
from ._capi import lib

_KEY_DTYPES = ("torch.int64", "torch.uint64")      # a key is 64 bits of storage; the sign is nobody's business
_ROW_DTYPES = ("torch.int32", "torch.uint32")
_F32 = ("torch.float32",)


def _stream_handle(stream, device):
    """-> the raw HIP stream of a call: `stream` (a torch.cuda.Stream, a raw handle or None = torch's current one on `device`)"""
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    return C.c_void_p(getattr(stream, "cuda_stream", stream))


def _on_stream(stream, device):
    """-> (a context that makes the call's stream torch's current one, so that the outputs the call allocates and clears are
    ordered on it; the raw handle)"""
    import torch
    if stream is None:
        s = torch.cuda.current_stream(device)
    elif hasattr(stream, "cuda_stream"):
        s = stream
    else:
        s = torch.cuda.ExternalStream(int(stream), device=device)
    return torch.cuda.stream(s), C.c_void_p(s.cuda_stream)


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

    def insert_many(self, hashes, policies, values, rows=None, row_count=None, stream=None):
        """numpy / sequence arguments: the host-staged insert, as ever.  A CUDA tensor of keys (int64 or uint64, contiguous [n])
        takes the device path (azmi_cache_insert_rows): policies [n, num_policy] and values [n, num_value] are float32 CUDA tensors,
        the launches are enqueued on `stream` (default: torch's current one) and nothing waits.  rows (int32 [m], CUDA) lists the
        rows to insert, in that order - the state insert_many(keys[rows], p[rows], v[rows]) leaves; row_count (one int32 on the
        device, read there) cuts the list short; without rows every row goes in, in order.  Host and device arguments do not mix."""
        if not _args.is_device_tensor(hashes):
            for name, x in (("policies", policies), ("values", values), ("rows", rows), ("row_count", row_count)):
                if _args.is_device_tensor(x):
                    raise RuntimeError(f"insert_many: {name} is a CUDA tensor but hashes is a host array (host and device arguments do not mix)")
            if rows is not None or row_count is not None:
                raise RuntimeError("insert_many: rows / row_count belong to the device path (a CUDA tensor of hashes)")
            h = np.ascontiguousarray(hashes, np.uint64)
            p = np.ascontiguousarray(policies, np.float32).reshape(len(h), self._np)
            v = np.ascontiguousarray(values, np.float32).reshape(len(h), self._nv)
            if lib.azmi_cache_insert_many(self._h, h.ctypes.data, p.ctypes.data, v.ctypes.data, len(h)) != 0:
                raise RuntimeError(lib.azmi_cache_last_error().decode())
            return
        dev = self._args[3]
        h = _args.device_tensor(hashes, "insert_many", "hashes", _KEY_DTYPES, (None,), dev)
        n = h.shape[0]
        p = _args.device_tensor(policies, "insert_many", "policies", _F32, (n, self._np), dev)
        v = _args.device_tensor(values, "insert_many", "values", _F32, (n, self._nv), dev)
        n_max = n
        if rows is not None:
            rows = _args.device_tensor(rows, "insert_many", "rows", _ROW_DTYPES, (None,), dev)
            n_max = rows.shape[0]
        if row_count is not None:
            row_count = _args.device_tensor(row_count, "insert_many", "row_count", _ROW_DTYPES, (1,), dev)
        if lib.azmi_cache_insert_rows(self._h, h.data_ptr(), p.data_ptr(), v.data_ptr(), None if rows is None else rows.data_ptr(),
                                      None if row_count is None else row_count.data_ptr(), n_max, _stream_handle(stream, dev)) != 0:
            raise RuntimeError(lib.azmi_cache_last_error().decode())

    def insert(self, hash, policy, value):
        self.insert_many([hash], [policy], [value])

    def find_many(self, hashes, stream=None):
        """-> (hit bool [n], p [n, num_policy], v [n, num_value]); the rows of a miss are zero.  numpy / sequence keys: numpy arrays,
        host-staged, as ever.  A CUDA tensor of keys (int64 or uint64, contiguous [n]): CUDA tensors, enqueued on `stream`
        (default: torch's current one), nothing waits (find_rows without the miss list)."""
        if not _args.is_device_tensor(hashes):
            h = np.ascontiguousarray(hashes, np.uint64)
            hit = np.zeros(len(h), np.uint8)
            p = np.zeros((len(h), self._np), np.float32)
            v = np.zeros((len(h), self._nv), np.float32)
            if lib.azmi_cache_find_many(self._h, h.ctypes.data, len(h), hit.ctypes.data, p.ctypes.data, v.ctypes.data) != 0:
                raise RuntimeError(lib.azmi_cache_last_error().decode())
            return hit.astype(bool), p, v
        return self._find_device("find_many", hashes, stream, None, None, False)[:3]

    def find_rows(self, keys, stream=None, p_out=None, v_out=None):
        """The device probe with its miss list (azmi_cache_find_rows): keys is a CUDA tensor (int64 or uint64, contiguous [n]) ->
        (hit bool [n], p [n, num_policy], v [n, num_value], miss_rows int32 [n], miss_count int32 [1]), all CUDA tensors.
        miss_rows[:miss_count] are the rows that missed, ascending - the order is a prefix over `hit`, the same on every run; the
        count stays on the device (HipLeafNet.forward_rows and insert_many(rows=, row_count=) read it there).  p_out / v_out:
        float32 CUDA tensors to write the hits' rows into; the rows of a miss are left as they are (new tensors: zero)."""
        return self._find_device("find_rows", keys, stream, p_out, v_out, True)

    def _find_device(self, what, keys, stream, p_out, v_out, compact):
        import torch
        dev = self._args[3]
        h = _args.device_tensor(keys, what, "hashes" if what == "find_many" else "keys", _KEY_DTYPES, (None,), dev)
        n = h.shape[0]
        ctx, handle = _on_stream(stream, dev)
        with ctx:
            p = torch.zeros((n, self._np), dtype=torch.float32, device=h.device) if p_out is None else \
                _args.device_tensor(p_out, what, "p_out", _F32, (n, self._np), dev)
            v = torch.zeros((n, self._nv), dtype=torch.float32, device=h.device) if v_out is None else \
                _args.device_tensor(v_out, what, "v_out", _F32, (n, self._nv), dev)
            hit = torch.zeros(n, dtype=torch.uint8, device=h.device)
            rows = torch.zeros(n, dtype=torch.int32, device=h.device) if compact else None
            count = torch.zeros(1, dtype=torch.int32, device=h.device) if compact else None
            if lib.azmi_cache_find_rows(self._h, h.data_ptr(), n, hit.data_ptr(), p.data_ptr(), v.data_ptr(), rows.data_ptr() if compact else None,
                                        count.data_ptr() if compact else None, handle) != 0:
                raise RuntimeError(lib.azmi_cache_last_error().decode())
        return hit.view(torch.bool), p, v, rows, count

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


def cached_forward(net, cache, canonical, keys, v_out=None, pi_out=None, stream=None):
    """cache_utils.cached_inference for a batch on the device (azmi_net_forward_cached): probe the cache with `keys`, run `net`
    (a HipLeafNet) on the rows that missed, insert their answers - three steps enqueued on one stream (default: torch's current
    one) with nothing read back.  canonical [n, C, H, W] float32 and keys [n] (int64 or uint64) are contiguous CUDA tensors
    -> (v [n, P+1], pi [n, M], hit bool [n]): a hit's row holds the cached bits, a miss's row the net's.  v_out / pi_out:
    float32 CUDA tensors to write into.  The cache's num_policy / num_value must be the net's M / P + 1.
    A key that occurs several times in one batch and is not in the cache yet is a miss every time: every such row is evaluated,
    the first one is inserted and the others are recognised as present (the reference, one position at a time, would hit from
    the second on).  One cache is used from one stream at a time."""
    import torch
    dev = cache._args[3]
    k = _args.device_tensor(keys, "cached_forward", "keys", _KEY_DTYPES, (None,), dev)
    n = k.shape[0]
    if not _args.is_tensor(canonical) or canonical.dim() < 1:
        raise RuntimeError(f"cached_forward: canonical must be a CUDA tensor [{n}, C, H, W], got {type(canonical).__name__}")
    c = _args.device_tensor(canonical, "cached_forward", "canonical", _F32, (n,) + (None,) * (canonical.dim() - 1), dev)
    v = None if v_out is None else _args.device_tensor(v_out, "cached_forward", "v_out", _F32, (n, cache._nv), dev)
    pi = None if pi_out is None else _args.device_tensor(pi_out, "cached_forward", "pi_out", _F32, (n, cache._np), dev)
    ctx, handle = _on_stream(stream, dev)
    with ctx:
        if v is None:
            v = torch.empty((n, cache._nv), dtype=torch.float32, device=k.device)
        if pi is None:
            pi = torch.empty((n, cache._np), dtype=torch.float32, device=k.device)
        hit = torch.zeros(n, dtype=torch.uint8, device=k.device)
        if lib.azmi_net_forward_cached(net._h, cache._h, c.data_ptr(), k.data_ptr(), n, v.data_ptr(), pi.data_ptr(), hit.data_ptr(), handle) != 0:
            raise RuntimeError(lib.azmi_cache_last_error().decode())
    return v, pi, hit.view(torch.bool)
