"""Rows/s of the dense StarGambit net of tests/golden/nn_sg_dense_4x16_k3.npz (36 planes, 13x13, growth 16, 4 blocks, 3x3, spatial head
+ 19 global actions): the bf16 matrix-core tile of csrc/leafnet_dense_sp.h against the fp32 tier (what the parent commit ran these
nets on; csrc/leafnet_f32.hip is unchanged) and against torch_net.LeafNet(..).cuda().process(x, amp_dtype=torch.bfloat16), the
reference's NNWrapper.process under autocast, on the same card.

The method of scripts/leafnet_dense_ab.py: per batch size a warm-up, then `--launches` forwards between two events; the three
contenders alternate `--repeats` times in one process; the median of each and the spread of its repeats are reported.
Usage: python scripts/leafnet_dense_sp_ab.py [--out profiles/leafnet_dense_sp_ab.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import alphazero as az  # noqa: E402
from leafnet_dense_ab import timed  # noqa: E402
import leafnet_dense_ref as dr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[184, 1024, 4096])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import copy
    net = dr.fixture("sg_dense")[0]
    spec = net.spec
    tnet = copy.deepcopy(net).cuda()
    contenders = {"torch bf16 autocast": None, "hip fp32": az.HipLeafNet(net, precision="fp32"), "hip bf16 tile": az.HipLeafNet(net, precision="bf16")}
    lines = ["batch  " + "  ".join(f"{n:>30}" for n in contenders) + "    tile / fp32  tile / torch   (rows/s, median of %d x %d launches; +- = (max - min) / median of the repeats)"
             % (a.repeats, a.launches)]
    for batch in a.batches:
        x = (torch.rand((batch,) + tuple(spec.in_shape), device="cuda", generator=torch.Generator("cuda").manual_seed(1)) < 0.3).float()
        v = torch.empty((batch, 3), device="cuda")
        pi = torch.empty((batch, spec.num_moves), device="cuda")
        fns = {n: ((lambda: tnet.process(x, amp_dtype=torch.bfloat16)) if h is None else (lambda h=h: h.forward(x, v, pi))) for n, h in contenders.items()}
        for fn in fns.values():
            for _ in range(5):
                fn()
        secs = {n: [] for n in fns}
        for _ in range(a.repeats):
            for n, fn in fns.items():
                secs[n].append(timed(fn, a.launches))
        med = {n: statistics.median(s) for n, s in secs.items()}
        cell = {n: f"{batch / med[n]:,.0f} +-{100 * (max(secs[n]) - min(secs[n])) / med[n]:.1f}%" for n in contenders}
        lines.append(f"{batch:>5}  " + "  ".join(f"{cell[n]:>30}" for n in contenders) +
                     f"    {med['hip fp32'] / med['hip bf16 tile']:.2f}x        {med['torch bf16 autocast'] / med['hip bf16 tile']:.2f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
