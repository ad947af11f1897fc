"""Rows/s of the layer-norm instance of the dense Connect4 tile (trunk_norm="layer": k_leafnet_dense<true>) on the reference-default
net (4 planes, growth 12, 4 blocks, 5x5) against two yardsticks: the batch-norm tile on the same net (k_leafnet_dense<false>, the
kernel scripts/leafnet_dense_ab.py times) and torch's bf16 autocast of the same layer net on the card.  The method is that of
scripts/leafnet_dense_ab.py: per batch size a warm-up, then `--launches` forwards between two events; the contenders alternate
`--repeats` times in one process; the median of each is reported, and the spread (min .. max over the repeats) of the two tiles.
Usage: python scripts/leafnet_dense_layer_ab.py [--out profiles/leafnet_dense_layer_ab.txt]
"""
import argparse
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import alphazero as az  # noqa: E402
from alphazero import torch_net  # noqa: E402
from leafnet_dense_ab import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096, 32768])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    spec = torch_net.connect4_dense_spec()
    lspec = dataclasses.replace(spec, trunk_norm="layer")
    tnet = torch_net.random_init(lspec, seed=3).cuda()
    contenders = {"torch bf16 autocast (layer)": None,
                  "batch tile": az.HipLeafNet(torch_net.random_init(spec, seed=3), precision="bf16"),
                  "layer tile": az.HipLeafNet(torch_net.random_init(lspec, seed=3), precision="bf16")}
    lines = ["batch  " + "  ".join(f"{n:>28}" for n in contenders) + "   layer / batch   layer / torch   spread batch tile      spread layer tile"
             "   (rows/s, median of %d x %d launches)" % (a.repeats, a.launches)]
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
        spread = {n: "%.3g .. %.3g" % (batch / max(s), batch / min(s)) for n, s in secs.items()}
        lines.append(f"{batch:>5}  " + "  ".join(f"{rate[n]:>28,.0f}" for n in contenders) +
                     f"   {rate['layer tile'] / rate['batch tile']:>13.3f}   {rate['layer tile'] / rate['torch bf16 autocast (layer)']:>12.2f}x"
                     f"   {spread['batch tile']:>20}   {spread['layer tile']:>20}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
