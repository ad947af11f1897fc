"""Batched position search against the loop it replaces, on one GPU.

  (a) MCTSBatch.search(visits, net): N trees in one arena, everything on the device
  (b) the reference-shaped loop (frozen_eval.py:594-647 written against this module): N stand-alone MCTS objects, find_leaf on
      each, the leaves' planes stacked into ONE net.process per step, process_result on each

for Connect4 (N positions x VISITS, the 6b64c bf16 net) and Tawlbwrdd (the configs/tawlbwrdd.yaml net).  Warm-up first, then
the two versions alternate in one process; every time is taken around a device synchronise; median and spread are printed.
  python scripts/search_batch_speed.py [--game connect4|tawlbwrdd|both] [--n N] [--visits V] [--reps R] [--loop-reps L]
                                       [--leaves-per-step K]
One JSON line per game on stdout.  --leaves-per-step K > 1 times (a) with K leaves of every tree in flight per step (WU-UCT: a
different search, so (b) is not run beside it); every line carries the steps, the time per step and the rows per net call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))


def positions(az, Game, n, rng, plies):
    """n non-terminal positions: random legal prefixes (legality from the rules kernels' valid masks)."""
    out = []
    while len(out) < n:
        gs = Game()
        ok = True
        for _ in range(int(rng.integers(0, plies + 1))):
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            if gs.scores() is not None:
                ok = False
                break
        if ok:
            out.append(gs)
    return out


def run_batch(az, mb, states, seeds, visits, net):
    import torch
    mb.reset(states, seeds=seeds)
    torch.cuda.synchronize()
    l0 = mb.stats()
    t0 = time.perf_counter()
    mb.search(visits, net=net)
    mb.synchronize()
    dt = time.perf_counter() - t0
    l1 = mb.stats()
    run_batch.last = dict(steps=l1["steps"] - l0["steps"], evaluator_leaves=l1["evaluator_leaves"])
    return dt, l1["launches"] - l0["launches"], l1["net_calls"] - l0["net_calls"], mb.counts()


def run_loop(az, Game, states, seeds, visits, net, cpuct):
    """The parent commit's only way to do this job.  Object creation is not timed."""
    import torch
    P, M, chw = Game._info()
    dev = torch.device("cuda", 0)
    trees = [az.MCTS(cpuct, P, M, game=Game, seed=int(s), max_simulations=visits) for s in seeds]
    dummy_v, dummy_pi = np.full(P + 1, 1.0 / (P + 1), np.float32), np.full(M, 1.0 / M, np.float32)
    torch.cuda.synchronize()
    calls = 0
    t0 = time.perf_counter()
    for _ in range(visits):
        leaves = [m.find_leaf(gs) for m, gs in zip(trees, states)]
        live = [i for i, leaf in enumerate(leaves) if leaf.scores() is None]
        calls += 2 * len(trees)                                   # find_leaf + the leaf's replay (scores, planes)
        if live:
            batch = torch.from_numpy(np.stack([leaves[i].canonicalized() for i in live])).to(dev)
            v, pi = net.process(batch)
            v, pi = v.cpu().numpy(), pi.cpu().numpy()
            calls += 1
        row = {i: r for r, i in enumerate(live)}
        for i, (m, gs) in enumerate(zip(trees, states)):
            if i in row:
                m.process_result(gs, v[row[i]], pi[row[i]])
            else:
                m.process_result(gs, dummy_v, dummy_pi)
            calls += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, calls, np.stack([m.counts() for m in trees])


def measure(az, name, n, visits, reps, loop_reps, leaves_per_step=1):
    from alphazero import torch_net
    Game, spec, plies = {"connect4": (az.Connect4GS, torch_net.connect4_spec(), 12),
                         "tawlbwrdd": (az.TawlbwrddGS, torch_net.tawlbwrdd_spec(), 6)}[name]
    net = az.HipLeafNet(torch_net.random_init(spec, seed=0), spec, precision="bf16")
    rng = np.random.default_rng(1)
    states = positions(az, Game, n, rng, plies)
    seeds = [1 + i for i in range(n)]
    mb = az.MCTSBatch(Game, n, 1.25, max_simulations=visits, seeds=seeds, leaves_per_step=leaves_per_step)
    if leaves_per_step > 1:
        loop_reps = 0
    run_batch(az, mb, states, seeds, visits, net)                  # warm-up (code objects, the net's scratch)
    a, b, launches, net_calls, loop_calls, same = [], [], 0, 0, 0, True
    order = ["a", "b"] * loop_reps + ["a"] * max(0, reps - loop_reps)
    for which in order:
        if which == "a":
            dt, launches, net_calls, counts_a = run_batch(az, mb, states, seeds, visits, net)
            a.append(dt)
        else:
            dt, loop_calls, counts_b = run_loop(az, Game, states, seeds, visits, net, 1.25)
            b.append(dt)
            same = same and bool(np.array_equal(counts_a, counts_b))
    rec = dict(game=name, positions=n, visits=visits,
               batch_s=dict(median=statistics.median(a), min=min(a), max=max(a), runs=len(a)),
               batch_launches=launches, batch_net_calls=net_calls, leaves_per_step=leaves_per_step, steps=run_batch.last["steps"],
               step_us=dict(median=1e6 * statistics.median(a) / run_batch.last["steps"], min=1e6 * min(a) / run_batch.last["steps"],
                            max=1e6 * max(a) / run_batch.last["steps"]),
               rows_per_net_call=run_batch.last["evaluator_leaves"] / max(1, net_calls))
    if b:
        rec.update(loop_s=dict(median=statistics.median(b), min=min(b), max=max(b), runs=len(b)), loop_device_calls=loop_calls,
                   ratio=statistics.median(b) / statistics.median(a), same_counts=same)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="both")
    ap.add_argument("--n", type=int, default=0, help="positions (default: 1024 Connect4, 256 Tawlbwrdd)")
    ap.add_argument("--visits", type=int, default=120)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=2, help="runs of the stand-alone-object loop (minutes each at full size; 0 = skip)")
    ap.add_argument("--leaves-per-step", type=int, default=1, help="K leaves of every tree in flight per step (1 = the plain search)")
    args = ap.parse_args()
    import alphazero as az
    for name in (["connect4", "tawlbwrdd"] if args.game == "both" else [args.game]):
        measure(az, name, args.n or (1024 if name == "connect4" else 256), args.visits, args.reps, args.loop_reps, args.leaves_per_step)


if __name__ == "__main__":
    main()
