"""build_opening_tree against the per-node host loop it replaces, Connect4 with the 6b64c fixture net (for the record: DESIGN.md 8.4).
    python scripts/opening_tree_timing.py [sims] [min_reach]
Both sides build the same tree in the same process: node b is searched with the tree seed node_seed(seed, b), the batched side on
one MCTSBatch, the loop with one stand-alone alphazero.MCTS per node (find_leaf / net / process_result per simulation) plus
GameState.play_move / scores() per child.  A warm-up call of each first, then the median of five runs each."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
import alphazero as az  # noqa: E402
import torch  # noqa: E402
from alphazero import torch_net  # noqa: E402

SIMS = int(sys.argv[1]) if len(sys.argv) > 1 else 64
MIN_REACH = float(sys.argv[2]) if len(sys.argv) > 2 else 0.01
SEED = 0


def fixture_net():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "nn_connect4_6b64c.npz"))
    net = torch_net.LeafNet(torch_net.connect4_spec())
    net.load_state_dict({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")})
    return az.HipLeafNet(net.eval())


def apply_temperature(probs, temperature):
    if temperature == 0:
        out = np.zeros_like(probs); out[np.argmax(probs)] = 1.0
        return out
    if temperature == 1.0:
        return probs
    scaled = np.power(probs + 1e-10, 1.0 / temperature)
    return scaled / scaled.sum()


def host_loop(net):
    """opening_analysis.py build_tree in BFS order, one MCTS object per node -> node count"""
    dev = torch.device("cuda", 0)
    nodes = [(az.Connect4GS(), 0, 1.0)]
    b = 0
    while b < len(nodes):
        gs, depth, reach = nodes[b]
        az.hash_game_state(gs)
        if gs.scores() is None:
            m = az.MCTS(1.25, 2, 7, seed=az.node_seed(SEED, b), max_simulations=SIMS)
            for _ in range(SIMS):
                leaf = m.find_leaf(gs)
                v, pi = net.process(torch.from_numpy(leaf.canonicalized()[None]).to(dev))
                m.process_result(gs, v[0].cpu().numpy(), pi[0].cpu().numpy(), False)
            counts = np.asarray(m.counts(), np.float64)
            samp = apply_temperature(counts / counts.sum(), az.temperature_at_depth(depth))
            for a in range(7):
                if samp[a] > 0 and reach * samp[a] >= MIN_REACH:
                    child = gs.copy()
                    child.play_move(a)
                    nodes.append((child, depth + 1, reach * float(samp[a])))
        b += 1
    return len(nodes)


def batched(net):
    return az.build_opening_tree(az.Connect4GS, az.Connect4GS(), SIMS, net=net, min_reach=MIN_REACH, seed=SEED)


def median_of_five(fn, net):
    fn(net)      # warm-up
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = fn(net)
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


if __name__ == "__main__":
    net = fixture_net()
    tb, tree = median_of_five(batched, net)
    tl, n_loop = median_of_five(host_loop, net)
    print(f"sims {SIMS}, min_reach {MIN_REACH}: build_opening_tree {len(tree)} nodes, {tree.stats['levels']} levels, "
          f"{tree.stats['chunks']} chunks, median {tb:.3f} s; per-node loop {n_loop} nodes, median {tl:.3f} s; ratio {tl / tb:.1f}")
