"""What `MCTSBatch(..., descents_per_step=L)` buys, on one GPU: steps, net rows, host reads and wall time of

  search   1024 Connect4 positions x 120 visits with the 6b64c bf16 net and a 200 k-entry position cache (frozen_eval's shape),
           `cold` (a fresh cache) and `warm` (the same positions again behind a reset, the cache kept)
  play     256 whole Connect4 games through play(100, net, cache, temp=1.0, max_moves=42), a fresh cache per run

for L in 1, 4, 16 (--ls).  Warm-up first; then the L values alternate in one process, --reps runs each; every time is taken
around a device synchronise; median (min - max) is reported, one JSON line per workload and L.  The answers of every L must equal
those of L = 1 (visit counts / move logs): `same` in the line.
  python scripts/search_batch_descents.py [--workload search|play|both] [--ls 1,4,16] [--reps R] [--n N] [--visits V] [--pkg DIR]
--pkg DIR imports the `alphazero` package from DIR (another build of the project, e.g. the parent commit's, beside its own
libazmi.so).  A package without descents_per_step runs L = 1 only and reports host_reads as null."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def positions(az, n, rng, plies):
    out = []
    while len(out) < n:
        gs = az.Connect4GS()
        ok = True
        for _ in range(int(rng.integers(0, plies + 1))):
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            if gs.scores() is not None:
                ok = False
                break
        if ok:
            out.append(gs)
    return out


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


def delta(a, b):
    return {k: b[k] - a[k] for k in ("launches", "net_calls", "steps")} | {
        "net_rows": b["evaluator_leaves"], "simulations": b["simulations"], "terminal_leaves": b["terminal_leaves"],
        "host_reads": b["host_reads"] - a["host_reads"] if "host_reads" in b else None}


def timed(mb, fn):
    import torch
    torch.cuda.synchronize()
    s0 = mb.stats()
    t0 = time.perf_counter()
    fn()
    mb.synchronize()
    dt = time.perf_counter() - t0
    return dt, delta(s0, mb.stats())


def batch(az, n, max_sims, seeds, L, has_dl):
    kw = dict(descents_per_step=L) if has_dl else {}
    return az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=max_sims, seeds=seeds, **kw)


def measure_search(az, net, n, visits, ls, reps, has_dl):
    states = positions(az, n, np.random.default_rng(1), 12)
    seeds = [1 + i for i in range(n)]
    mbs = {L: batch(az, n, visits, seeds, L, has_dl) for L in ls}
    cold, warm, st_cold, st_warm, counts = ({L: [] for L in ls} for _ in range(5))

    def one(L, record):
        mb = mbs[L]
        cache = az.ShardedS3FIFOCache.for_engine(200_000, 7, 3)
        mb.reset(states)
        dt, st = timed(mb, lambda: mb.search(visits, net=net, cache=cache))
        c = mb.counts()
        mb.reset(states)
        dt2, st2 = timed(mb, lambda: mb.search(visits, net=net, cache=cache))
        same = bool(np.array_equal(c, mb.counts()))
        if record:
            cold[L].append(dt); warm[L].append(dt2); st_cold[L] = st; st_warm[L] = st2; counts[L] = (c, same)

    for L in ls:
        one(L, False)                 # warm-up: code objects, the net's scratch
    for _ in range(reps):
        for L in ls:
            one(L, True)
    for L in ls:
        same = bool(np.array_equal(counts[L][0], counts[ls[0]][0])) and counts[L][1]
        print(json.dumps(dict(workload="search", positions=n, visits=visits, descents_per_step=L, same=same,
                              cold_s=summary(cold[L]), cold=st_cold[L], warm_s=summary(warm[L]), warm=st_warm[L])), flush=True)


def measure_play(az, net, n, visits, max_moves, ls, reps, has_dl):
    states = positions(az, n, np.random.default_rng(2), 6)
    seeds = [1 + i for i in range(n)]
    mbs = {L: batch(az, n, visits * max_moves, seeds, L, has_dl) for L in ls}
    times, stats, logs = ({L: [] for L in ls} for _ in range(3))

    def one(L, record):
        mb = mbs[L]
        cache = az.ShardedS3FIFOCache.for_engine(200_000, 7, 3)
        mb.reset(states)
        dt, st = timed(mb, lambda: mb.play(visits, net=net, cache=cache, temp=1.0, max_moves=max_moves))
        if record:
            times[L].append(dt); stats[L] = st; logs[L] = mb.move_logs()

    for L in ls:
        one(L, False)
    for _ in range(reps):
        for L in ls:
            one(L, True)
    for L in ls:
        same = all(np.array_equal(a, b) for a, b in zip(logs[L], logs[ls[0]]))
        print(json.dumps(dict(workload="play", games=n, visits=visits, max_moves=max_moves, descents_per_step=L, same=same,
                              moves_played=int(sum(len(x) for x in logs[L])), wall_s=summary(times[L]), **stats[L])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=["search", "play", "both"])
    ap.add_argument("--ls", default="1,4,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=0, help="positions / games (default: 1024 / 256)")
    ap.add_argument("--visits", type=int, default=0, help="default: 120 (search), 100 (play)")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "alphazero-pybind11_amd"))
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import alphazero as az
    from alphazero import torch_net
    has_dl = "descents_per_step" in inspect.signature(az.MCTSBatch.__init__).parameters
    ls = [int(x) for x in args.ls.split(",")] if has_dl else [1]
    spec = torch_net.connect4_spec()
    net = az.HipLeafNet(torch_net.random_init(spec, seed=0), spec, precision="bf16")
    print(json.dumps(dict(package=os.path.basename(os.path.abspath(args.pkg)),descents_per_step_supported=has_dl, ls=ls, reps=args.reps)), flush=True)
    if args.workload in ("search", "both"):
        measure_search(az, net, args.n or 1024, args.visits or 120, ls, args.reps, has_dl)
    if args.workload in ("play", "both"):
        measure_play(az, net, args.n or 256, args.visits or 100, 42, ls, args.reps, has_dl)


if __name__ == "__main__":
    main()
