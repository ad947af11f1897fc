"""Seconds per hand-off of a trained model to self-play: HipLeafNet(net_on_gpu) - state_dict to the host, the fold in numpy, a new
blob and a new net object: what there was before refresh and the yardstick - against hip.refresh(net_on_gpu) followed by one
stream synchronisation (kernels fold and lay out the image on the device, in place).  The 6 x 64 Connect4 ResNet net on both
tiers and the reference-default dense net.

Per net: one warm-up of each side (the first refresh allocates its staging image), then the two alternate `--repeats` times in one
process, each timed by a host clock around work that ends in a device synchronise; the median of each is reported.
Usage: python scripts/leafnet_refresh_ab.py [--out profiles/leafnet_refresh_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))

import torch  # noqa: E402

import alphazero as az  # noqa: E402
from alphazero import torch_net  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nets = [("connect4 6b64c", torch_net.connect4_spec(), "bf16"), ("connect4 6b64c", torch_net.connect4_spec(), "bf16x3"),
            ("connect4 dense 4x12 k5", torch_net.connect4_dense_spec(), "bf16")]
    lines = [f"{'net':<24} {'tier':<7} {'image bytes':>11}  {'HipLeafNet(net) ms':>18}  {'refresh + sync ms':>17}  {'ratio':>7}   (median of {a.repeats} alternating repeats)"]
    for name, spec, precision in nets:
        model = torch_net.random_init(spec, seed=3).cuda()
        hip = az.HipLeafNet(model, precision=precision)
        timed(lambda: hip.refresh(model))                      # warm-up: allocates the table, scratch and staging image
        timed(lambda: az.HipLeafNet(model, precision=precision))
        build, refresh = [], []
        for _ in range(a.repeats):
            build.append(timed(lambda: az.HipLeafNet(model, precision=precision))[0])
            refresh.append(timed(lambda: hip.refresh(model))[0])
        assert hip.blob() == az.HipLeafNet(model, precision=precision)._blob, "the refreshed image is not the folded one"
        b, r = statistics.median(build) * 1e3, statistics.median(refresh) * 1e3
        lines.append(f"{name:<24} {precision:<7} {len(hip.blob()):>11}  {b:>18.3f}  {r:>17.3f}  {b / r:>6.0f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
