"""Native round and pipeline drivers over PlayManager engines, plus the debug probes and the tracy stubs."""
import ctypes as C

import numpy as np

from ._capi import lib, check


def _engine_arrays(pms, streams):
    """-> (engine handles, their streams, count) as the native round drivers take them; every engine remembers its stream"""
    k = len(pms)
    arr_pm = (C.c_void_p * k)(*[pm._h for pm in pms])
    arr_st = (C.c_void_p * k)(*[C.c_void_p(int(s)) for s in streams])
    for pm, s in zip(pms, streams):
        pm._last_stream = C.c_void_p(int(s))
    return arr_pm, arr_st, k


def _net_handles(nets):
    """one net handle per model group (None = a group without a net)"""
    return (C.c_void_p * len(nets))(*[None if n is None else n._h for n in nets])


def run_rounds(pms, net, rounds, streams):
    """azmi_run_rounds: native round driver over several engines (one stream each) sharing one HipLeafNet."""
    arr_pm, arr_st, k = _engine_arrays(pms, streams)
    check(lib.azmi_run_rounds(arr_pm, net._h, k, int(rounds), arr_st))


def run_rounds_groups(pms, nets, rounds, streams):
    """azmi_run_rounds_groups: `nets[g]` (HipLeafNet or None) evaluates the leaves of model group g."""
    arr_pm, arr_st, k = _engine_arrays(pms, streams)
    check(lib.azmi_run_rounds_groups(arr_pm, _net_handles(nets), len(nets), k, int(rounds), arr_st))


def pipeline_supported(pm, net):
    """azmi_pipeline_supported: True when azmi_run_pipeline can drive this engine with this net (the Connect4 engine with plain
    PUCT seats, one model group, NN seats and a bf16 Connect4-family HipLeafNet - or `net=None` for an engine whose seats all use
    EvalType.RANDOM: the tree side alone -, at most 16384 concurrent games)."""
    return bool(lib.azmi_pipeline_supported(pm._h, None if net is None else net._h))


def pipeline_supported_groups(pm, nets):
    """azmi_pipeline_supported_groups: True when azmi_run_pipeline_groups can drive this engine with nets[g] behind model group g
    (None = a group of RANDOM seats)."""
    return bool(lib.azmi_pipeline_supported_groups(pm._h, _net_handles(nets), len(nets)))


_PIPE_KEYS = ("tiles", "tile_boards", "last_epoch_sims", "tree_wgs_started", "net_wgs_started", "last_epoch_inserts", "net_wgs", "tree_wgs",
              "tree_latest_start_us", "net_latest_start_us", "net_kernel_us", "tree_kernel_us", "epochs", "host_enqueue_us", "calibration_rounds",
              "answer_table_hits")


def _pipe_stats(out):
    d = dict(zip(_PIPE_KEYS, (int(x) for x in out)))
    # (slot 14 carries two 32-bit counts: the calibration launches of this call, and the requests the net side has given up on and
    # the boundary has sent again since the engine was created - PipeCtl::lost_total)
    d["lost_total"] = d["calibration_rounds"] >> 32
    d["freezes"] = (d["calibration_rounds"] >> 8) & 0xFFFFFF      # polling wavefronts that stood still for > 2 ms since creation (credited, not errors)
    d["calibration_rounds"] &= 0xFF
    return d


def _pipeline_call(pm, stream, call):
    """the stream, the counter buffer and the read-out of one pipeline call: call(stream, out) -> status"""
    st = pm._stream_arg(stream)
    out = (C.c_uint64 * 16)()
    check(call(st, out))
    return _pipe_stats(out)


def run_pipeline(pm, net, epochs, sims_per_epoch, stream=None):
    """azmi_run_pipeline: `epochs` epochs of the asynchronous tree / net pipeline on one engine (persistent tree wavefronts and
    net workgroups side by side; moves, game ends and cache inserts between epochs).  Synchronous.  Returns a dict of
    pipeline counters: net tiles run and boards in them since the pipeline was created, simulations / insert-log entries of
    the last epoch, workgroups launched and started, kernel and host-enqueue times of this call."""
    return _pipeline_call(pm, stream, lambda st, out: lib.azmi_run_pipeline(
        pm._h, None if net is None else net._h, int(epochs), int(sims_per_epoch), st, out))


def run_pipeline_groups(pm, nets, epochs, sims_per_epoch, stream=None):
    """azmi_run_pipeline_groups: run_pipeline with one net per model group (play_past: the new model behind group 0, the past one
    behind group 1; None = the reference's RandPlayer)."""
    return _pipeline_call(pm, stream, lambda st, out: lib.azmi_run_pipeline_groups(
        pm._h, _net_handles(nets), len(nets), int(epochs), int(sims_per_epoch), st, out))


def pipeline_log_duplicates(pm):
    """azmi_debug_pipe_log_dupes: (answers consumed in the last epoch, of those asked for more than once, of those within 4096 log
    entries of their twin) - what inserting at answer time / coalescing requests in flight would save."""
    out = (C.c_uint64 * 3)()
    check(lib.azmi_debug_pipe_log_dupes(pm._h, out))
    return int(out[0]), int(out[1]), int(out[2])


def rng_probe(kind, seed, n, param=0.0, reps=1, device=0):
    """azmi_rng_probe: kind in {"pcg32","shuffle","uniform","gamma","gamma_fresh"}."""
    kinds = {"pcg32": 0, "shuffle": 1, "uniform": 2, "gamma": 3, "gamma_fresh": 4}
    k = kinds[kind]
    dtype = np.uint32 if k < 2 else np.float32
    out = np.zeros(n * (reps if k == 1 else 1), dtype)
    check(lib.azmi_rng_probe(device, k, seed, param, n, reps, out.ctypes.data))
    return out.reshape(reps, n) if k == 1 else out


def _cache_check(rc):
    if rc != 0:
        raise RuntimeError(lib.azmi_cache_last_error().decode("utf-8", "replace") or f"azmi error {rc}")


def cache_find_group(cache, group_lanes, hashes):
    """azmi_debug_cache_find_group: ShardedS3FIFOCache.find_many with the probe of a `group_lanes`-lane group (8 or 64, the
    engines' GM::GROUP) -> (hit, policy, value)."""
    h = np.ascontiguousarray(hashes, np.uint64)
    hit = np.zeros(len(h), np.uint8)
    p = np.zeros((len(h), cache._np), np.float32)
    v = np.zeros((len(h), cache._nv), np.float32)
    _cache_check(lib.azmi_debug_cache_find_group(cache._h, int(group_lanes), h.ctypes.data, len(h), hit.ctypes.data, p.ctypes.data, v.ctypes.data))
    return hit.astype(bool), p, v


def cache_insert_locked(cache, hashes, policies, values, waves):
    """azmi_debug_cache_insert_locked: the pipeline's locked insert (one wavefront per entry, `waves` wavefronts in one kernel) of
    host rows -> the number of entries whose shard lock was not had (0 unless something is wrong)."""
    h = np.ascontiguousarray(hashes, np.uint64)
    p = np.ascontiguousarray(policies, np.float32).reshape(len(h), cache._np)
    v = np.ascontiguousarray(values, np.float32).reshape(len(h), cache._nv)
    failed = C.c_uint32(0)
    _cache_check(lib.azmi_debug_cache_insert_locked(cache._h, h.ctypes.data, p.ctypes.data, v.ctypes.data, len(h), int(waves), C.byref(failed)))
    return int(failed.value)


# Tracy stubs — py_wrapper.cc:772-787: must exist even as no-ops
def tracy_is_enabled():
    return False


def tracy_frame_mark():
    return None


def _tracy_zone_begin(name, file, line):
    return None


def _tracy_zone_end():
    return None


def _tracy_set_thread_name(name):
    return None
