"""The resample plan and gather at the size of one headline run's samples after the mirror (for the record: DESIGN.md 8.5).
    python scripts/resample_probe.py [rows]          (default 4 Mi Connect4 rows: canonical 672 B, v 12 B, pi 28 B per row)
Times azmi_resample_plan (host clock: the call ends in its one synchronisation) and, with device events, per row array:
the gather (alphazero.resample_rows), a device-to-device hipMemcpy of the bytes the gather writes, and the torch one-liner
x[torch.repeat_interleave(torch.arange(n), copies)]; then azmi_resample_gather itself on preallocated outputs, once with the
three arrays in ONE call (n_arrays = 3) and as three calls of one array.  The contenders of a comparison alternate: every
repetition times each of them once, a timed sample being INNER back-to-back calls between two events.  Rates are traffic rates:
bytes read plus bytes written over the time (the gather reads n rows and writes rows_out, a copy reads and writes the same
bytes, the one-liner reads and writes rows_out rows plus its index).  Two warm-up rounds, then the median of REPS.  Not a test,
not part of bench.py."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
import alphazero as az  # noqa: E402
import torch  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4 << 20
WARM, REPS, INNER = 2, 21, 8
DEV = torch.device("cuda", 0)


def hip_memcpy():
    """hipMemcpyAsync of the runtime this process already uses, or None"""
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            fn = C.CDLL(name).hipMemcpyAsync
        except (OSError, AttributeError):
            continue
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        return fn
    return None


def alternate_ms(fns):
    """-> per contender [median, minimum, maximum] ms per call; the contenders take turns inside every repetition"""
    for _ in range(WARM):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / INNER)
    return [[round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)] for t in times]


def host_ms(fn):
    for _ in range(WARM):
        fn()
    times = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def raw_gather(copies, offsets, xs, outs, stream):
    """one azmi_resample_gather call over the arrays xs -> outs"""
    k = len(xs)
    ins = (C.c_void_p * k)(*[x.data_ptr() for x in xs])
    dst = (C.c_void_p * k)(*[o.data_ptr() for o in outs])
    rb = (C.c_uint32 * k)(*[x[0].numel() * 4 for x in xs])

    def call():
        rc = az.lib.azmi_resample_gather(copies.data_ptr(), offsets.data_ptr(), N, k, ins, dst, rb, 0, stream)
        assert rc == 0, az.lib.azmi_samples_last_error().decode()
    return call


if __name__ == "__main__":
    gen = torch.Generator(device=DEV).manual_seed(20261020)
    arrays = {"canonical": torch.rand((N, 4, 6, 7), device=DEV, generator=gen), "v": torch.rand((N, 3), device=DEV, generator=gen),
              "pi": torch.rand((N, 7), device=DEV, generator=gen)}
    loss = torch.rand(N, dtype=torch.float64, device=DEV, generator=gen)
    copies, offsets, rows_out, total = az.resample_plan(loss, 7)
    med, lo, hi = host_ms(lambda: az.resample_plan(loss, 7))
    print(json.dumps({"what": "resample_plan", "rows": N, "rows_out": rows_out, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                      "ms_max": round(hi, 4), "loss_bytes_per_s": round(N * 8 / (med * 1e-3), 0)}), flush=True)
    memcpy = hip_memcpy()
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    copies64 = copies.to(torch.int64)
    rate = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e9, 1)
    for name, x in arrays.items():
        row = x[0].numel() * 4
        ours = az.resample_rows(copies, offsets, x, rows_out=rows_out)[0]
        theirs = x[torch.repeat_interleave(torch.arange(N, device=DEV), copies64)]
        assert torch.equal(ours, theirs), name
        del theirs
        dst = torch.empty_like(ours)
        nbytes = rows_out * row
        copy = (lambda: memcpy(dst.data_ptr(), ours.data_ptr(), nbytes, 3, stream)) if memcpy is not None else (lambda: dst.copy_(ours))      # 3: device to device
        g, m, t = alternate_ms([lambda: az.resample_rows(copies, offsets, x, rows_out=rows_out), copy,
                                lambda: x[torch.repeat_interleave(torch.arange(N, device=DEV), copies64)]])
        assert torch.equal(dst, ours)
        del dst, ours
        print(json.dumps({"what": "gather", "array": name, "row_bytes": row, "rows": N, "rows_out": rows_out,
                          "gather_ms": g, "gather_GB_per_s": rate((N + rows_out) * row, g[0]),
                          "copy": "hipMemcpyAsync device-to-device" if memcpy is not None else "Tensor.copy_",
                          "copy_ms": m, "copy_GB_per_s": rate(2 * nbytes, m[0]),
                          "torch_one_liner_ms": t, "torch_one_liner_GB_per_s": rate(2 * nbytes + rows_out * 8, t[0])}), flush=True)
    xs = list(arrays.values())
    outs = [torch.zeros((rows_out,) + tuple(x.shape[1:]), dtype=torch.float32, device=DEV) for x in xs]
    joint = raw_gather(copies, offsets, xs, outs, stream)
    singles = [raw_gather(copies, offsets, [x], [o], stream) for x, o in zip(xs, outs)]
    j_ms, s_ms = alternate_ms([joint, lambda: [f() for f in singles]])
    for x, o in zip(xs, outs):
        assert torch.equal(o, az.resample_rows(copies, offsets, x, rows_out=rows_out)[0])
    print(json.dumps({"what": "azmi_resample_gather, three arrays, preallocated outputs", "one_call_n_arrays_3_ms": j_ms,
                      "three_calls_n_arrays_1_ms": s_ms}), flush=True)
