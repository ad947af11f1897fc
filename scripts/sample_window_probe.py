"""Times the window gather against torch.index_select and select_top against torch.topk on one GPU.  The
contenders of a comparison alternate inside every repetition; a timed sample is `inner` back-to-back calls between two device
events; two warm-up rounds, then the median, the fastest and the slowest of `reps` samples, per call.

    python scripts/sample_window_probe.py [--rows 1048576] [--keys 4194304] [--k 1048576] [--reps 21]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def compare(contenders, reps, inner):
    samples = {name: [] for name in contenders}
    for rep in range(reps + 2):
        for name, fn in contenders.items():
            t = timed(fn, inner)
            if rep >= 2:
                samples[name].append(t)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--floats", type=int, default=168)
    ap.add_argument("--keys", type=int, default=1 << 22)
    ap.add_argument("--k", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    import torch
    import alphazero as az
    from alphazero import samples
    import sample_window_ref as ref
    dev = torch.device("cuda", 0)

    # the gather: 1 Mi rows of 168 floats in 16 segments, one pass in one batch
    n, f = args.rows, args.floats
    whole = torch.randn(n, f, device=dev)
    cuts = [n * s // 16 for s in range(17)]
    segs = [whole[lo:hi] for lo, hi in zip(cuts, cuts[1:])]
    rows_list = [int(s.shape[0]) for s in segs]
    perm = torch.from_numpy(ref.permutation(n, 7, 0)).to(dev)
    got = samples._window_gather(segs, rows_list, None, 7, 0, 0, n, None)
    assert torch.equal(got, whole.index_select(0, perm))
    by_index = lambda: samples._window_gather(segs, rows_list, perm, 0, 0, 0, n, None)
    assert torch.equal(by_index(), got)
    out = torch.empty_like(whole)
    res = compare({"window_gather (perm computed)": lambda: samples._window_gather(segs, rows_list, None, 7, 0, 0, n, None),
                   "window_gather (index list)": by_index,
                   "torch.index_select": lambda: torch.index_select(whole, 0, perm, out=out),
                   "copy_ of the same bytes": lambda: out.copy_(whole)}, args.reps, 8)
    traffic = 2.0 * n * f * 4
    print(f"gather: {n} rows x {f} float32 ({traffic / 1e9:.3f} GB read + written)")
    for name, (med, lo, hi) in res.items():
        print(f"  {name:32s} {med:8.4f} ms ({lo:.4f} - {hi:.4f})  {traffic / med / 1e6:8.1f} GB/s  {traffic / med / 1e6 / 8000:.1%} of 8 TB/s")

    # the selection: the k largest of `keys` reservoir keys
    m, k = args.keys, args.k
    iters = torch.randint(0, 200, (m,), dtype=torch.int32, device=dev)
    keys = az.reservoir_keys(iters, 200, 0.98, 11)
    index, _ = az.select_top(keys, k)
    top = torch.topk(keys, k, sorted=False).indices
    assert torch.equal(index, torch.sort(top).values)      # (distinct keys: the sets agree)
    res = compare({"select_top": lambda: az.select_top(keys, k),
                   "torch.topk (unsorted)": lambda: torch.topk(keys, k, sorted=False),
                   "torch.topk + sort of the indices": lambda: torch.sort(torch.topk(keys, k, sorted=False).indices),
                   "reservoir_keys": lambda: az.reservoir_keys(iters, 200, 0.98, 11)}, args.reps, 4)
    print(f"selection: k = {k} of {m} float64 keys")
    for name, (med, lo, hi) in res.items():
        print(f"  {name:32s} {med:8.4f} ms ({lo:.4f} - {hi:.4f})")


if __name__ == "__main__":
    main()
