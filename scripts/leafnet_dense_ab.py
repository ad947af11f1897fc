"""Rows/s of the reference-default dense Connect4 net (4 planes, growth 12, 4 blocks, 5x5): what a user would otherwise run on the
same card - torch_net.LeafNet(connect4_dense_spec()).cuda().process(x, amp_dtype=torch.bfloat16), the reference's
NNWrapper.process under autocast - against the fp32 tier and the bf16 matrix-core tile of HipLeafNet.

Per batch size: a warm-up, then `--launches` forwards between two events; the three contenders alternate `--repeats` times in
one process and the median of each is reported.  Usage: python scripts/leafnet_dense_ab.py [--out profiles/leafnet_dense_ab.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))

import torch  # noqa: E402

import alphazero as az  # noqa: E402
from alphazero import torch_net  # noqa: E402


def timed(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096, 32768])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    spec = torch_net.connect4_dense_spec()
    net = torch_net.random_init(spec, seed=3)
    tnet = torch_net.random_init(spec, seed=3).cuda()
    contenders = {"torch bf16 autocast": None, "hip fp32": az.HipLeafNet(net, precision="fp32"), "hip bf16 tile": az.HipLeafNet(net, precision="bf16")}
    lines = ["batch  " + "  ".join(f"{n:>22}" for n in contenders) + "    tile / torch   (rows/s, median of %d x %d launches)" % (a.repeats, a.launches)]
    for batch in a.batches:
        x = (torch.rand((batch,) + tuple(spec.in_shape), device="cuda", generator=torch.Generator("cuda").manual_seed(1)) < 0.3).float()
        v = torch.empty((batch, 3), device="cuda")
        pi = torch.empty((batch, 7), device="cuda")
        fns = {n: ((lambda: tnet.process(x, amp_dtype=torch.bfloat16)) if h is None else (lambda h=h: h.forward(x, v, pi))) for n, h in contenders.items()}
        for fn in fns.values():
            for _ in range(5):
                fn()
        secs = {n: [] for n in fns}
        for _ in range(a.repeats):
            for n, fn in fns.items():
                secs[n].append(timed(fn, a.launches))
        rate = {n: batch / statistics.median(s) for n, s in secs.items()}
        lines.append(f"{batch:>5}  " + "  ".join(f"{rate[n]:>22,.0f}" for n in contenders) + f"    {rate['hip bf16 tile'] / rate['torch bf16 autocast']:.2f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
