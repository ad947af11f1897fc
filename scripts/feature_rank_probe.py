"""effective_rank and feature_rank against torch's float32 SVD on the same device features (for the record: DESIGN.md 8.5.3).
    python scripts/feature_rank_probe.py
Three measurements.  (1) effective_rank over 512 positions of the Connect4 6b64c net on the fp32 tier - trunk, pooling, Gram,
record - against the reference's tail on the same pooled features: centre, torch.linalg.svdvals in float32, the ratio, one .item()
(neural_net.py:867-873).  (2), (3) feature_rank alone at (512, 64) and (65536, 128) against that tail.  The two contenders alternate
inside every repetition; a timed sample is INNER back-to-back calls between two host clock readings, each call ending in its own
host synchronisation (the record of feature_rank, the .item() of the torch tail): what a caller of either waits for.  Two warm-up
rounds, then the median of REPS with the range, per call.  The Gram kernel's own time is a matter of
`rocprofv3 --kernel-trace --stats` over this script in a run of its own; its floor is the larger of `gram_flop` (2 n 64^2 per
upper-triangle tile pair) at the float64 vector rate and `feature_bytes` (4 n C) at the HBM rate.  Not a test, not part of bench.py."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
import alphazero as az  # noqa: E402
import torch  # noqa: E402
from alphazero import torch_net  # noqa: E402

WARM, REPS, INNER = 2, 15, 8
DEV = torch.device("cuda", 0)


def alternate_us(fns):
    """-> per contender [median, minimum, maximum] microseconds per call; the contenders take turns inside every repetition"""
    for _ in range(WARM):
        for fn in fns:
            for _ in range(INNER):
                fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(INNER):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e6 / INNER)
    return [[round(statistics.median(t), 1), round(min(t), 1), round(max(t), 1)] for t in times]


def svd_tail(feats):
    """neural_net.py:867-873 on float32 device features"""
    f = feats - feats.mean(dim=0, keepdim=True)
    s2 = torch.linalg.svdvals(f) ** 2
    denom = (s2 * s2).sum()
    if denom.item() == 0:
        return 1.0
    return float(((s2.sum() ** 2) / denom).item())


if __name__ == "__main__":
    gen = torch.Generator(device=DEV).manual_seed(20261021)
    spec = torch_net.connect4_spec()
    net = az.HipLeafNet(torch_net.random_init(spec, seed=3), precision="fp32")
    boards = (torch.rand((512,) + tuple(spec.in_shape), device=DEV, generator=gen) < 0.2).float().contiguous()
    feats = net.trunk_features(boards)
    ours, theirs = az.effective_rank(boards, net), svd_tail(feats)
    e_us, t_us = alternate_us([lambda: az.effective_rank(boards, net), lambda: svd_tail(net.trunk_features(boards))])
    print(json.dumps({"what": "effective_rank, Connect4 6b64c fp32 tier, 512 positions, against trunk_features + the float32 SVD tail",
                      "effective_rank": ours, "svd_tail_float32": theirs, "effective_rank_us": e_us, "trunk_plus_svd_tail_us": t_us}), flush=True)
    for n, c in ((512, 64), (65536, 128)):
        f = (torch.randn((n, c), device=DEV, generator=gen) * (torch.rand(c, device=DEV, generator=gen) + 0.2)).contiguous()
        ours, theirs = az.feature_rank(f)["rank"], svd_tail(f)
        g_us, s_us = alternate_us([lambda: az.feature_rank(f), lambda: svd_tail(f)])
        tiles = (c + 63) // 64
        flop = 2 * n * 64 * 64 * (tiles * (tiles + 1) // 2)
        print(json.dumps({"what": "feature_rank against the float32 SVD tail", "n": n, "C": c, "rank": ours, "svd_tail_float32": theirs,
                          "feature_rank_us": g_us, "svd_tail_us": s_us, "gram_flop": flop, "feature_bytes": 4 * n * c}), flush=True)
