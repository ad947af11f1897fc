"""Batched position search against the loop it replaces, on one GPU.

  (a) MCTSBatch.search(visits, net): N trees in one arena, everything on the device
  (b) the reference-shaped loop (frozen_eval.py:594-647 written against this module): N stand-alone MCTS objects, find_leaf on
      each, the leaves' planes stacked into ONE net.process per step, process_result on each

for Connect4 (N positions x VISITS, the 6b64c bf16 net) and Tawlbwrdd (the configs/tawlbwrdd.yaml net).  Warm-up first, then
the two versions alternate in one process; every time is taken around a device synchronise; median and spread are printed.
  python scripts/search_batch_speed.py [--game connect4|tawlbwrdd|both] [--n N] [--visits V] [--reps R] [--loop-reps L]
                                       [--leaves-per-step K] [--play MOVES] [--evaluator net|playout] [--sweep C0,C1,...]
One JSON line per game on stdout.  --leaves-per-step K > 1 times (a) with K leaves of every tree in flight per step (WU-UCT: a
different search, so (b) is not run beside it); every line carries the steps, the time per step and the rows per net call.

--play MOVES times walking games instead of one search: (a) MCTSBatch.play(visits, net, max_moves=MOVES) - MOVES x (search, pick,
update_roots) enqueued in one call - against (b) the same trees as stand-alone MCTS objects stepped from Python: one net.process
per step, then pick_move(probs(1.0)) and update_root per object per move.  The equal-answers check compares the move logs of the
two versions (defaults: 256 Connect4 positions x 64 visits x 8 moves with --play 8, 32 Tawlbwrdd positions x 64 visits x 4 moves
with --play 4).

--evaluator playout times the PLAYOUT evaluator instead of the net: (a) MCTSBatch.search(visits, evaluator="playout") - the
rollouts on the device - against (b) the loop it replaces (mcts_analysis.py:649): the same trees as MCTS objects stepped from
Python, one playout_eval_batch(leaves, seeds) per step, with the seeds of (a) (MCTSBatch.rollout_seed), so that the counts of every
pair are compared.  With --leaves-per-step K > 1 (b) is the batched object calls, every leaf's playout_eval answered at once.
Without --n / --visits it runs the four workloads of DESIGN.md 8.3: Connect4 1024 x 120, Connect4 16 x 1600 at K = 1 and K = 8,
Tawlbwrdd 64 x 64.

--sweep c0,c1,... times a visit sweep on one set of trees (the inner loop of mcts_analysis.py:run_analysis): (a) one
MCTSBatch.search_to(max, net, checkpoints=(c0, c1, ...)) plus checkpoints() - the snapshots recorded on the device on the way -
against (b) what the batch offered before: per checkpoint search(delta, net), then counts(), probs(1.0), root_values() and
root_q_values().  The snapshots of (a) must equal the read-outs of (b).  The same line carries the cost of the target rule itself:
search_to(max) without checkpoints against search(max), alternating."""
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


def run_playout_batch(az, mb, states, seeds, visits):
    import torch
    mb.reset(states, seeds=seeds)
    torch.cuda.synchronize()
    l0 = mb.stats()
    t0 = time.perf_counter()
    mb.search(visits, evaluator="playout")
    mb.synchronize()
    dt = time.perf_counter() - t0
    l1 = mb.stats()
    return dt, l1["launches"] - l0["launches"], l1["steps"] - l0["steps"], l1["evaluator_leaves"], mb.counts()


def run_playout_loop(az, Game, states, seeds, rs, visits, cpuct, K):
    """The loop the device rollouts replace: MCTS objects stepped from Python, one playout_eval_batch per step (K == 1); K > 1: the
    batched object calls with every leaf's playout_eval answered at once, in descent order.  Object creation is not timed."""
    import torch
    P, M, chw = Game._info()
    trees = [az.MCTS(cpuct, P, M, game=Game, seed=int(s), max_simulations=visits) for s in seeds]
    dummy_v, dummy_pi = np.full(P + 1, 1.0 / (P + 1), np.float32), np.full(M, 1.0 / M, np.float32)
    j = [0] * len(trees)
    seed_of = az.MCTSBatch.rollout_seed
    torch.cuda.synchronize()
    calls = 0
    t0 = time.perf_counter()
    if K == 1:
        for _ in range(visits):
            leaves = [m.find_leaf(gs) for m, gs in zip(trees, states)]
            live = [i for i, leaf in enumerate(leaves) if leaf.scores() is None]
            calls += 2 * len(trees)
            if live:
                v, pi = az.playout_eval_batch([leaves[i] for i in live], [seed_of(rs[i], j[i]) for i in live])
                calls += 1
            row = {i: r for r, i in enumerate(live)}
            for i, (m, gs) in enumerate(zip(trees, states)):
                if i in row:
                    m.process_result(gs, v[row[i]], pi[row[i]]); j[i] += 1
                else:
                    m.process_result(gs, dummy_v, dummy_pi)
                calls += 1
    else:
        for left in range(visits, 0, -K):
            for i, (m, gs) in enumerate(zip(trees, states)):
                for k in range(min(K, left)):
                    leaf = m.find_leaf_batched(gs)
                    v, pi = (dummy_v, dummy_pi) if leaf.scores() is not None else az.playout_eval(leaf, seed=seed_of(rs[i], j[i]))
                    j[i] += leaf.scores() is None
                    m.process_result_batched(gs, k, v, pi)
                    calls += 4
                m.reset_batch()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, calls, np.stack([m.counts() for m in trees])


def measure_playout(az, name, n, visits, reps, loop_reps, K):
    Game, plies = {"connect4": (az.Connect4GS, 12), "tawlbwrdd": (az.TawlbwrddGS, 6)}[name]
    rng = np.random.default_rng(1)
    states = positions(az, Game, n, rng, plies)
    seeds = [1 + i for i in range(n)]
    mb = az.MCTSBatch(Game, n, 1.25, max_simulations=visits, seeds=seeds, leaves_per_step=K)
    run_playout_batch(az, mb, states, seeds, visits)               # warm-up
    rs = [int(x) for x in mb.rollout_seeds()]
    a, b, launches, steps, rollouts, loop_calls, same = [], [], 0, 1, 0, 0, True
    for which in ["a", "b"] * loop_reps + ["a"] * max(0, reps - loop_reps):
        if which == "a":
            dt, launches, steps, rollouts, counts_a = run_playout_batch(az, mb, states, seeds, visits)
            a.append(dt)
        else:
            dt, loop_calls, counts_b = run_playout_loop(az, Game, states, seeds, rs, visits, 1.25, K)
            b.append(dt)
            same = same and bool(np.array_equal(counts_a, counts_b))
    rec = dict(mode="playout", game=name, positions=n, visits=visits, leaves_per_step=K,
               batch_s=dict(median=statistics.median(a), min=min(a), max=max(a), runs=len(a)),
               batch_launches=launches, steps=steps, rollouts=rollouts, step_us=1e6 * statistics.median(a) / steps)
    if b:
        rec.update(loop_s=dict(median=statistics.median(b), min=min(b), max=max(b), runs=len(b)), loop_device_calls=loop_calls,
                   ratio=statistics.median(b) / statistics.median(a), same_counts=same)
    print(json.dumps(rec), flush=True)


def run_play_batch(az, mb, states, seeds, visits, net, moves):
    import torch
    mb.reset(states, seeds=seeds)
    torch.cuda.synchronize()
    l0 = mb.stats()
    t0 = time.perf_counter()
    mb.play(visits, net=net, max_moves=moves)
    mb.synchronize()
    dt = time.perf_counter() - t0
    l1 = mb.stats()
    return dt, l1["launches"] - l0["launches"], l1["net_calls"] - l0["net_calls"], [l.tolist() for l in mb.move_logs()]


def run_play_loop(az, Game, states, seeds, visits, net, cpuct, moves):
    """The loop play() replaces: the trees as stand-alone objects, one net.process per step, update_root per object per move."""
    import torch
    P, M, chw = Game._info()
    dev = torch.device("cuda", 0)
    trees = [az.MCTS(cpuct, P, M, game=Game, seed=int(s), max_simulations=visits * moves) for s in seeds]
    gss = [g.copy() for g in states]
    logs = [[] for _ in trees]
    dummy_v, dummy_pi = np.full(P + 1, 1.0 / (P + 1), np.float32), np.full(M, 1.0 / M, np.float32)
    live = list(range(len(trees)))
    torch.cuda.synchronize()
    calls = 0
    t0 = time.perf_counter()
    for _ in range(moves):
        for _ in range(visits):
            leaves = {i: trees[i].find_leaf(gss[i]) for i in live}
            need = [i for i in live if leaves[i].scores() is None]
            calls += 2 * len(live)
            if need:
                batch = torch.from_numpy(np.stack([leaves[i].canonicalized() for i in need])).to(dev)
                v, pi = net.process(batch)
                v, pi = v.cpu().numpy(), pi.cpu().numpy()
                calls += 1
            row = {i: r for r, i in enumerate(need)}
            for i in live:
                if i in row:
                    trees[i].process_result(gss[i], v[row[i]], pi[row[i]])
                else:
                    trees[i].process_result(gss[i], dummy_v, dummy_pi)
                calls += 1
        for i in live:
            mv = trees[i].pick_move(trees[i].probs(1.0))
            trees[i].update_root(gss[i], mv)
            gss[i].play_move(mv)
            logs[i].append(mv)
            calls += 4                                            # probs, pick_move, update_root, the successor's replay (scores)
        live = [i for i in live if gss[i].scores() is None]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, calls, logs


def measure_play(az, name, n, visits, reps, loop_reps, moves):
    from alphazero import torch_net
    Game, spec, plies = {"connect4": (az.Connect4GS, torch_net.connect4_spec(), 12),
                         "tawlbwrdd": (az.TawlbwrddGS, torch_net.tawlbwrdd_spec(), 6)}[name]
    net = az.HipLeafNet(torch_net.random_init(spec, seed=0), spec, precision="bf16")
    rng = np.random.default_rng(1)
    states = positions(az, Game, n, rng, plies)
    seeds = [1 + i for i in range(n)]
    # Connect4's flat arena: every move's search counts; the wide games compact behind update_roots
    mb = az.MCTSBatch(Game, n, 1.25, max_simulations=visits * moves if name == "connect4" else visits, seeds=seeds)
    run_play_batch(az, mb, states, seeds, visits, net, moves)      # warm-up
    a, b, launches, net_calls, loop_calls, same = [], [], 0, 0, 0, True
    for which in ["a", "b"] * loop_reps + ["a"] * max(0, reps - loop_reps):
        if which == "a":
            dt, launches, net_calls, logs_a = run_play_batch(az, mb, states, seeds, visits, net, moves)
            a.append(dt)
        else:
            dt, loop_calls, logs_b = run_play_loop(az, Game, states, seeds, visits, net, 1.25, moves)
            b.append(dt)
            same = same and logs_a == logs_b
    rec = dict(mode="play", game=name, positions=n, visits=visits, moves=moves,
               batch_s=dict(median=statistics.median(a), min=min(a), max=max(a), runs=len(a)),
               batch_launches=launches, batch_net_calls=net_calls, finished=int(mb.finished().sum()))
    if b:
        rec.update(loop_s=dict(median=statistics.median(b), min=min(b), max=max(b), runs=len(b)), loop_device_calls=loop_calls,
                   ratio=statistics.median(b) / statistics.median(a), same_move_logs=same)
    print(json.dumps(rec), flush=True)


def run_sweep_to(az, mb, states, seeds, cps, net):
    import torch
    mb.reset(states, seeds=seeds)
    torch.cuda.synchronize()
    l0 = mb.stats()["launches"]
    t0 = time.perf_counter()
    mb.search_to(cps[-1], net=net, checkpoints=cps)
    snap = mb.checkpoints()
    dt = time.perf_counter() - t0
    return dt, mb.stats()["launches"] - l0, snap


def run_sweep_loop(az, mb, states, seeds, cps, net):
    """The sweep without search_to: every checkpoint ends the enqueued run, four read-outs and four copies each."""
    import torch
    mb.reset(states, seeds=seeds)
    torch.cuda.synchronize()
    l0 = mb.stats()["launches"]
    t0 = time.perf_counter()
    prev, rows = 0, []
    for c in cps:
        mb.search(c - prev, net=net)
        rows.append((mb.counts(), mb.probs(1.0), mb.root_values(), mb.root_q_values()))
        prev = c
    dt = time.perf_counter() - t0
    snap = {k: np.stack([r[i] for r in rows], axis=1) for i, k in enumerate(("counts", "probs", "root_values", "root_q_values"))}
    return dt, mb.stats()["launches"] - l0, snap


def run_plain(az, mb, states, seeds, visits, net, to):
    import torch
    mb.reset(states, seeds=seeds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if to:
        mb.search_to(visits, net=net)
    else:
        mb.search(visits, net=net)
    mb.synchronize()
    return time.perf_counter() - t0


def measure_sweep(az, name, n, cps, reps):
    from alphazero import torch_net
    Game, spec, plies = {"connect4": (az.Connect4GS, torch_net.connect4_spec(), 12),
                         "tawlbwrdd": (az.TawlbwrddGS, torch_net.tawlbwrdd_spec(), 6)}[name]
    net = az.HipLeafNet(torch_net.random_init(spec, seed=0), spec, precision="bf16")
    rng = np.random.default_rng(1)
    states = positions(az, Game, n, rng, plies)
    seeds = [1 + i for i in range(n)]
    mb = az.MCTSBatch(Game, n, 1.25, max_simulations=cps[-1], seeds=seeds)
    stats = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x), runs=len(x))
    rec = dict(mode="sweep", game=name, positions=n, checkpoints=list(cps))
    run_plain(az, mb, states, seeds, cps[-1], net, False)          # warm-up (code objects, the net's scratch)
    run_sweep_to(az, mb, states, seeds, cps, net)
    a, b, s_plain, s_to, la, lb, same = [], [], [], [], 0, 0, True
    for _ in range(reps):
        s_plain.append(run_plain(az, mb, states, seeds, cps[-1], net, False))
        s_to.append(run_plain(az, mb, states, seeds, cps[-1], net, True))
        dt, la, snap_a = run_sweep_to(az, mb, states, seeds, cps, net)
        a.append(dt)
        dt, lb, snap_b = run_sweep_loop(az, mb, states, seeds, cps, net)
        b.append(dt)
        same = same and bool(snap_a["taken"].all()) and all(np.array_equal(snap_a[k], snap_b[k]) for k in snap_b)
    rec.update(search_s=stats(s_plain), search_to_s=stats(s_to), search_to_over_search=statistics.median(s_to) / statistics.median(s_plain),
               sweep_to_s=stats(a), sweep_loop_s=stats(b), ratio=statistics.median(b) / statistics.median(a), sweep_to_launches=la,
               sweep_loop_launches=lb, same_snapshots=same)
    print(json.dumps(rec), flush=True)


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
    ap.add_argument("--n", type=int, default=0, help="positions (default: 1024 Connect4, 256 Tawlbwrdd; with --play 256 and 32)")
    ap.add_argument("--visits", type=int, default=0, help="default: 120, with --play 64")
    ap.add_argument("--play", type=int, default=0, metavar="MOVES", help="time MCTSBatch.play over MOVES moves against the object loop")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=2, help="runs of the stand-alone-object loop (minutes each at full size; 0 = skip)")
    ap.add_argument("--leaves-per-step", type=int, default=1, help="K leaves of every tree in flight per step (1 = the plain search)")
    ap.add_argument("--evaluator", default="net", choices=["net", "playout"], help="playout: rollouts on the device against the playout_eval_batch loop")
    ap.add_argument("--sweep", default="", metavar="C0,C1,...", help="time search_to(max, checkpoints) + checkpoints() against per-checkpoint search + read-outs")
    args = ap.parse_args()
    import alphazero as az
    if args.sweep:
        cps = tuple(int(x) for x in args.sweep.split(","))
        for name in (["connect4", "tawlbwrdd"] if args.game == "both" else [args.game]):
            measure_sweep(az, name, args.n or (1024 if name == "connect4" else 256), cps, args.reps)
        return
    if args.evaluator == "playout":
        if args.play:
            ap.error("--evaluator playout times search(), not --play")
        if args.n or args.visits:
            for name in (["connect4", "tawlbwrdd"] if args.game == "both" else [args.game]):
                measure_playout(az, name, args.n or 64, args.visits or 64, args.reps, args.loop_reps, args.leaves_per_step)
            return
        for name, n, visits, K in (("connect4", 1024, 120, 1), ("connect4", 16, 1600, 1), ("connect4", 16, 1600, 8), ("tawlbwrdd", 64, 64, 1)):
            if args.game in ("both", name):
                measure_playout(az, name, n, visits, args.reps, args.loop_reps, K)
        return
    for name in (["connect4", "tawlbwrdd"] if args.game == "both" else [args.game]):
        if args.play:
            measure_play(az, name, args.n or (256 if name == "connect4" else 32), args.visits or 64, args.reps, args.loop_reps, args.play)
            continue
        measure(az, name, args.n or (1024 if name == "connect4" else 256), args.visits or 120, args.reps, args.loop_reps, args.leaves_per_step)


if __name__ == "__main__":
    main()
