"""One k_sample_metrics launch against the two k_sample_loss launches iteration_losses makes on the same rows (for the record:
DESIGN.md 8.5).
    python scripts/sample_metrics_probe.py [rows]          (default 65536 rows: one chunk of eval_metrics)
Two shapes: Connect4 (M = 7, V = 3) and the unified StarGambit policy width (M = StarGambitUnifiedGS.NUM_MOVES(), V = 3), the
latter with sparse targets (about 24 positive entries a row: what a search over the legal moves leaves) and with dense ones (70 %
positive: the worst case, every positive entry costs four float64 logarithms and a division).  The two
contenders alternate inside every repetition; a timed sample is INNER back-to-back calls of azmi_sample_metrics (or of the pair of
azmi_sample_loss calls) on preallocated outputs between two device events; two warm-up rounds, then the median of REPS, per
call.  At this size a call is a few microseconds of kernel behind a launch, so the event figure is the rate at which the launches
drain, not the kernel alone: run the script under `rocprofv3 --kernel-trace --stats` for the kernels' own times.  Bytes: both
contenders read 4 (M + V) bytes of targets and 4 (M + V) of probabilities per row; the losses write 16 bytes per row, the metrics
13 * 8 + 8.  Not a test, not part of bench.py."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
import alphazero as az  # noqa: E402
import torch  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
WARM, REPS, INNER = 2, 21, 64
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
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / INNER)
    return [[round(statistics.median(t), 3), round(min(t), 3), round(max(t), 3)] for t in times]


def rows_like(n, width, gen):
    x = torch.rand((n, width), device=DEV, generator=gen)
    return (x / x.sum(dim=1, keepdim=True)).contiguous()


if __name__ == "__main__":
    gen = torch.Generator(device=DEV).manual_seed(20261020)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    SG = az.StarGambitUnifiedGS.NUM_MOVES()
    for game, M, V, positive in (("connect4", az.Connect4GS.NUM_MOVES(), 3, 0.7), ("stargambit_unified, sparse targets", SG, 3, 24.0 / SG),
                                 ("stargambit_unified, dense targets", SG, 3, 0.7)):
        t, p, tv, pv = rows_like(N, M, gen), rows_like(N, M, gen), rows_like(N, V, gen), rows_like(N, V, gen)
        t[torch.rand((N, M), device=DEV, generator=gen) >= positive] = 0.0      # targets hold zeros: illegal and unvisited moves
        cols = torch.empty((13, N), dtype=torch.float64, device=DEV)
        mcts, net = torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
        loss_pi, loss_v = torch.empty(N, dtype=torch.float64, device=DEV), torch.empty(N, dtype=torch.float64, device=DEV)

        def metrics():
            rc = az.lib.azmi_sample_metrics(t.data_ptr(), p.data_ptr(), tv.data_ptr(), pv.data_ptr(), N, M, V, 1.5, cols.data_ptr(), N, mcts.data_ptr(),
                                            net.data_ptr(), 0, stream)
            assert rc == 0, az.lib.azmi_samples_last_error().decode()

        def losses():
            rc = az.lib.azmi_sample_loss(t.data_ptr(), p.data_ptr(), N, M, 1.0, loss_pi.data_ptr(), 0, stream)
            rc = rc or az.lib.azmi_sample_loss(tv.data_ptr(), pv.data_ptr(), N, V, 1.5, loss_v.data_ptr(), 0, stream)
            assert rc == 0, az.lib.azmi_samples_last_error().decode()

        m_us, l_us = alternate_us([metrics, losses])
        assert torch.equal(cols[0], loss_pi) and torch.equal(cols[1], loss_v)      # the same bits, at the size timed
        read = N * 8 * (M + V)
        print(json.dumps({"what": "k_sample_metrics against two k_sample_loss", "game": game, "rows": N, "M": M, "V": V, "positive_targets": round(float((t > 0).float().mean()), 4),
                          "metrics_us": m_us, "metrics_bytes_read": read, "metrics_bytes_written": N * (13 * 8 + 8),
                          "losses_us": l_us, "losses_bytes_read": read, "losses_bytes_written": N * 16}), flush=True)
