"""The measurement behind profiles/cache_rows.txt: rows/s of the cache's device-pointer entries against the
host-staged numpy entries on the same cache shape, and cached_forward against net.forward, on one MI355X.
    python profiles/cache_rows_measure.py [out.txt]
Method: every shape is warmed up first; a sample is one call (device path: between two events on the stream; host path: a host
clock around the call, which ends in its own device synchronise); `REPEATS` samples per figure, device and host samples
alternating; the figure is the median, the spread min .. max.  The cache is refilled to the same state before every insert sample
outside the timed part."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
N = 65536
REPEATS = 15


def main():
    import torch
    import alphazero as az
    from alphazero import torch_net
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    dev = torch.device("cuda", 0)

    def say(line):
        print(line, file=out, flush=True)
        if out is not sys.stdout:
            print(line, flush=True)

    def device_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        return a.elapsed_time(b)

    def host_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter(); fn(); torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def report(name, rows, samples):
        s = np.sort(np.asarray(samples))
        med = float(np.median(s))
        say(f"{name:44s} median {med:9.3f} ms  min {s[0]:9.3f}  max {s[-1]:9.3f}  -> {rows / med / 1e3:10.2f} M rows/s  ({len(s)} samples)")
        return med

    rng = np.random.default_rng(1)
    keys = rng.integers(1, 1 << 62, size=2 * N, dtype=np.uint64)
    pol = rng.random((2 * N, 7), dtype=np.float32); val = rng.random((2 * N, 3), dtype=np.float32)
    dk = torch.from_numpy(keys.view(np.int64)).to(dev); dp = torch.from_numpy(pol).to(dev); dv = torch.from_numpy(val).to(dev)
    say(f"cache ShardedS3FIFOCache.for_engine(1 << 22, 7, 3), n = {N} rows per call, {REPEATS} samples per figure, torch {torch.__version__}, "
        f"{torch.cuda.get_device_name(0)}")

    # ---- find: the first N keys are present, probed on both paths -----------------------------------------------------------------
    cache = az.ShardedS3FIFOCache.for_engine(1 << 22, 7, 3)
    cache.insert_many(keys[:N], pol[:N], val[:N])
    for _ in range(3):
        cache.find_rows(dk[:N]); cache.find_many(dk[:N]); cache.find_many(keys[:N])
    d_rows, d_many, h_many = [], [], []
    for _ in range(REPEATS):
        d_rows.append(device_ms(lambda: cache.find_rows(dk[:N])))
        d_many.append(device_ms(lambda: cache.find_many(dk[:N])))
        h_many.append(host_ms(lambda: cache.find_many(keys[:N])))
    report("find_rows (device, with the miss list)", N, d_rows)
    report("find_many (device keys, no miss list)", N, d_many)
    report("find_many (numpy, host-staged)", N, h_many)
    half = torch.cat([dk[: N // 2], dk[N: N + N // 2]]).contiguous()
    for _ in range(3):
        cache.find_rows(half)
    report("find_rows (device, half of the keys absent)", N, [device_ms(lambda: cache.find_rows(half)) for _ in range(REPEATS)])

    # ---- insert: N new keys into a cache that holds the first N ----------------------------------------------------------------------
    d_ins, h_ins = [], []
    for i in range(REPEATS + 2):
        for path in ("device", "host"):
            c = az.ShardedS3FIFOCache.for_engine(1 << 22, 7, 3)
            c.insert_many(keys[:N], pol[:N], val[:N])
            torch.cuda.synchronize()
            if path == "device":
                ms = device_ms(lambda: c.insert_many(dk[N:], dp[N:], dv[N:]))
            else:
                ms = host_ms(lambda: c.insert_many(keys[N:], pol[N:], val[N:]))
            if i >= 2:
                (d_ins if path == "device" else h_ins).append(ms)
            del c
    report("insert_many (device rows)", N, d_ins)
    report("insert_many (numpy, host-staged)", N, h_ins)

    # ---- cached_forward with the 6b64c Connect4 net at 0 %, 50 %, 100 % hits against net.forward alone ----------------------------------
    spec = torch_net.connect4_spec()
    net = az.HipLeafNet(torch_net.random_init(spec, seed=3), spec)
    x = (torch.rand((2 * N, 4, 6, 7), device=dev) < 0.2).float().contiguous()
    v = torch.empty((N, 3), device=dev); pi = torch.empty((N, 7), device=dev)
    for _ in range(3):
        net.forward(x[:N], v, pi)
    fwd = [device_ms(lambda: net.forward(x[:N], v, pi)) for _ in range(REPEATS)]
    report("net.forward alone (6b64c Connect4, bf16)", N, fwd)
    mixed_x = torch.cat([x[: N // 2], x[N: N + N // 2]]).contiguous()
    for share, kx, kk in ((0, x[N:], dk[N:]), (50, mixed_x, half), (100, x[:N], dk[:N])):
        samples = []
        for i in range(REPEATS + 2):
            c = az.ShardedS3FIFOCache.for_engine(1 << 22, 7, 3)
            az.cached_forward(net, c, x[:N], dk[:N], v_out=v, pi_out=pi)      # the first N keys are present
            torch.cuda.synchronize()
            ms = device_ms(lambda: az.cached_forward(net, c, kx, kk, v_out=v, pi_out=pi))
            if i >= 2:
                samples.append(ms)
            del c
        report(f"cached_forward, {share:3d} % hits", N, samples)


if __name__ == "__main__":
    main()
