"""-m gpu: the root read-outs of the device search - probs / probs_pruned at every temperature, pick_move, root_value,
root_q_values, the root entropy - and the prior normalisation and backup inside process_result, on trees grown with the scripted
sharp evaluators of tests/mcts_readout_ref.py: the stand-alone `MCTS` object call by call against the oracle, then `MCTSBatch`
with the same inputs.  Every comparison is equality of bits (NaN entries: NaN on both sides); tests/test_oracle_readouts.py
holds the oracle itself to a plain restatement at the same inputs and shows its vectors finite there, so nothing is skipped."""
import numpy as np
import pytest

import mcts_readout_ref as ref
from mcts_readout_ref import TEMPS, same_bits

pytestmark = pytest.mark.gpu

CONFIGS = {
    "puct": dict(cpuct=1.25),
    "noise": dict(cpuct=1.25, epsilon=0.25, root_policy_temp=1.25, shaped_dirichlet=True, root_fpu_zero=True),
}
SIMS, PLIES = 24, 4
GAMES = ["Connect4GS", "BrandubhGS", "TawlbwrddGS", "StarGambitUnifiedGS"]


@pytest.fixture(scope="module")
def az():
    import alphazero
    return alphazero


def _games(az, oracle, name):
    """(device game state, oracle game state, keyword arguments of az.MCTS, of oracle.Mcts) at the opening position"""
    if name == "StarGambitUnifiedGS":
        return az.StarGambitUnifiedGS(0), oracle.Game.sg_unified(0), dict(game=az.StarGambitUnifiedGS, relative_values=True), dict(relative_values=True)
    Game = getattr(az, name)
    gid = dict(Connect4GS=oracle.GAME_CONNECT4, BrandubhGS=oracle.GAME_BRANDUBH, TawlbwrddGS=oracle.GAME_TAWLBWRDD)[name]
    return Game(), oracle.Game(gid), ({} if name == "Connect4GS" else dict(game=Game, max_simulations=400)), {}


def _stream(m):
    """position of the object's pcg32 stream, through the root-children hook"""
    import alphazero
    u = m._query(alphazero.Query.ROOT_CHILDREN)[1]
    return int(u[1]) | (int(u[2]) << 32)


def _compare_readouts(m, o, what, picks=True):
    """every read-out of the device object `m` against the oracle `o`; -> the moves picked from probs(t), in TEMPS order"""
    assert np.array_equal(m.counts(), o.counts()), what
    assert same_bits(m.root_q_values(), o.root_q()), what
    assert same_bits(m.root_value(), o.root_value()), f"{what}: root_value {m.root_value()} vs {o.root_value()}"
    assert m.depth() == o.depth() and m.root_n() == o.root_n(), what
    assert same_bits([m.normalized_root_entropy()], [o.entropy()]), f"{what}: entropy {m.normalized_root_entropy()!r} vs {o.entropy()!r}"
    assert same_bits([m.avg_leaf_depth()], [o.avg_leaf_depth()]), f"{what}: avg_leaf_depth {m.avg_leaf_depth()!r} vs {o.avg_leaf_depth()!r}"
    assert np.array_equal(m.principal_variation(5), o.principal_variation(5)), what
    moves = []
    for t in TEMPS:
        for pruned in (False, True):
            fn = "probs_pruned" if pruned else "probs"
            got = m.probs_pruned(t) if pruned else m.probs(t)
            want = o.probs(t, pruned=pruned)
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert same_bits(got, want), f"{what}: {fn}({t}) differs at moves {bad[:8]}: {got[bad[:8]]!r} vs {want[bad[:8]]!r}"
            if picks:
                mv = m.pick_move(got)
                assert mv == o.pick_move(want), f"{what}: pick_move({fn}({t}))"
                if not pruned:
                    moves.append(mv)
    if picks:
        assert _stream(m) == o.rng_state(), f"{what}: the streams are at different positions after the picks"
    return moves


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("name", GAMES)
def test_object_readouts_with_sharp_evaluators(az, oracle, name, cfg):
    """24 simulations per ply, 4 plies with update_root in between, the scripted sharp evaluator: every value vector
    process_result returns and, after every ply, every read-out at every temperature equal the oracle's."""
    gs, og, dkw, okw = _games(az, oracle, name)
    kw = dict(CONFIGS[cfg]); cpuct = kw.pop("cpuct")
    noise = kw.get("epsilon", 0) > 0
    M = og.num_moves()
    m = az.MCTS(cpuct, 2, M, seed=31, **dkw, **kw)
    o = oracle.Mcts(cpuct, 2, M, seed=31, **okw, **kw)
    if name == "TawlbwrddGS":
        assert int(og.valid().sum()) > 64, "the wavefront engine's child loops must take a second pass"
    for ply in range(PLIES):
        for sim in range(SIMS):
            leaf = m.find_leaf(gs); oleaf = o.find_leaf(og)
            canon = oleaf.canonical()
            assert np.array_equal(leaf.canonicalized(), canon), f"ply {ply}, simulation {sim}: another leaf than the oracle's"
            if oleaf.scores() is not None:
                v, pi = np.full(3, 1 / 3, np.float32), np.zeros(M, np.float32)
            else:
                v, pi = ref.sharp_eval(canon, oleaf.valid())
            out = m.process_result(gs, v.copy(), pi, noise)
            assert same_bits(out, o.process_result(v.copy(), pi, noise)), f"ply {ply}, simulation {sim}: the backed-up value"
        if name == "TawlbwrddGS" and ply == 0:
            assert len(o.root_children()[0]) > 64
        moves = _compare_readouts(m, o, f"{name}/{cfg} ply {ply}")
        move = moves[(ply + 1) % len(TEMPS)]                 # the pick from probs(1), probs(2), probs(0.5), probs(0.2)
        m.update_root(gs, move); o.update_root(og, move)
        gs.play_move(move); og.play(move)
        assert og.scores() is None
        if noise:
            m.apply_root_policy_temp(); o.apply_root_policy_temp()
            if o.root_n() > 0:
                m.add_root_noise(); o.add_root_noise()


@pytest.mark.parametrize("name", GAMES)
def test_object_readouts_of_shallow_roots(az, oracle, name):
    """fresh objects, the uniform evaluator, 0 / 1 / 2 / k + 1 simulations: no children (whatever the oracle gives, NaN
    included, is the answer; pick_move of such a vector throws in the reference and is not called), the prior branch
    (count_sum == 0: pow at t != 0, none at t == 0, probs_pruned falls through to probs), one visited child, and every child
    visited once, where the temp == 0 branches split evenly over the k tied moves."""
    gs, og, dkw, okw = _games(az, oracle, name)
    M = og.num_moves()
    k = int(og.valid().sum())
    for sims in (0, 1, 2, k + 1):
        m = az.MCTS(1.25, 2, M, seed=7, **dkw)
        o = oracle.Mcts(1.25, 2, M, seed=7, **okw)
        for sim in range(sims):
            leaf = m.find_leaf(gs); oleaf = o.find_leaf(og)
            if sim < 3:
                assert np.array_equal(leaf.canonicalized(), oleaf.canonical())
            v, pi = oracle.dumb_eval(oleaf)
            assert same_bits(m.process_result(gs, v.copy(), pi), o.process_result(v.copy(), pi))
        _compare_readouts(m, o, f"{name} after {sims} simulations", picks=sims > 0)
        if sims == k + 1:
            assert (o.counts()[og.valid() == 1] == 1).all()
            even = np.where(og.valid() == 1, np.float32(1.0 / k), np.float32(0))
            assert np.array_equal(m.probs(0.0), even) and np.array_equal(m.probs_pruned(0.0), even)


# ---- MCTSBatch with the same inputs ------------------------------------------------------------------------------------------
def _start_positions(az, oracle, name, n):
    """n openings: tree i stands i % 4 fixed moves into the game"""
    out = []
    for i in range(n):
        gs, og, _, _ = _games(az, oracle, name)
        for j in range(i % 4):
            legal = np.flatnonzero(og.valid())
            mv = int(legal[(5 * i + 3 * j) % legal.size])
            gs.play_move(mv); og.play(mv)
        assert og.scores() is None
        out.append((gs, og))
    return out


@pytest.mark.parametrize("name,n,K", [("Connect4GS", 1, 1), ("Connect4GS", 9, 1), ("Connect4GS", 65, 1), ("Connect4GS", 9, 3),
                                      ("BrandubhGS", 1, 1), ("BrandubhGS", 9, 1), ("BrandubhGS", 65, 1), ("BrandubhGS", 9, 3)])
def test_batch_readouts_with_sharp_evaluators(az, oracle, name, n, K):
    """find_leaves / process_results with the scripted evaluator (the oracle beside every tree supplies each leaf's legal-move
    mask); probs(t), probs_pruned(t) and pick_moves(t) at every temperature equal, per tree, the stand-alone object with the
    tree's seed fed the same rows, and the oracle.  9 lane groups do not fit one wavefront, 65 trees not one workgroup of
    the wide kernels; K = 3: leaves_per_step."""
    Game = getattr(az, name)
    M = Game.NUM_MOVES()
    cpuct, kw = 1.25, dict(fpu_reduction=0.25)
    seeds = [900 + 13 * i for i in range(n)]
    starts = _start_positions(az, oracle, name, n)
    mb = az.MCTSBatch(Game, n, cpuct, max_simulations=SIMS, seeds=seeds, leaves_per_step=K, **kw)
    mb.reset([g for g, _ in starts])
    extra = {} if name == "Connect4GS" else dict(game=Game)
    ms = [az.MCTS(cpuct, 2, M, seed=seeds[i], max_simulations=SIMS, **extra, **kw) for i in range(n)]
    os_ = [oracle.Mcts(cpuct, 2, M, seed=seeds[i], **kw) for i in range(n)]
    for _ in range(SIMS // K):
        canon, idx = mb.find_leaves(numpy=True)
        rows = []                                             # (tree, descent, v, pi) in row order
        for t in range(n):
            for k in range(K):
                oleaf = os_[t].find_leaf(starts[t][1]) if K == 1 else os_[t].find_leaf_batched(starts[t][1])
                if K == 1:
                    ms[t].find_leaf(starts[t][0])
                else:
                    ms[t].find_leaf_batched(starts[t][0])
                if oleaf.scores() is not None:                # backed up at once, no row
                    v, pi = np.full(3, 1 / 3, np.float32), np.full(M, 1 / M, np.float32)
                    if K == 1:
                        os_[t].process_result(v.copy(), pi); ms[t].process_result(starts[t][0], v.copy(), pi)
                    else:
                        os_[t].process_result_batched(k, v.copy(), pi); ms[t].process_result_batched(starts[t][0], k, v.copy(), pi)
                    continue
                c = oleaf.canonical()
                assert np.array_equal(canon[len(rows)], c), f"tree {t}, descent {k}: another leaf than the oracle's"
                v, pi = ref.sharp_eval(c, oleaf.valid())
                rows.append((t, k, v, pi))
        assert idx.tolist() == [r[0] for r in rows]
        V = np.stack([r[2] for r in rows]) if rows else np.zeros((0, 3), np.float32)
        PI = np.stack([r[3] for r in rows]) if rows else np.zeros((0, M), np.float32)
        mb.process_results(V, PI)
        for t, k, v, pi in rows:
            if K == 1:
                a = ms[t].process_result(starts[t][0], v.copy(), pi); b = os_[t].process_result(v.copy(), pi)
            else:
                a = ms[t].process_result_batched(starts[t][0], k, v.copy(), pi); b = os_[t].process_result_batched(k, v.copy(), pi)
            assert same_bits(a, b), f"tree {t}: the backed-up value"
        if K > 1:
            for t in range(n):
                ms[t].reset_batch(); os_[t].reset_batch()
    assert np.array_equal(mb.counts(), np.stack([o.counts() for o in os_]))
    for t in TEMPS:
        for pruned in (False, True):
            fn = "probs_pruned" if pruned else "probs"
            got = mb.probs_pruned(t) if pruned else mb.probs(t)
            for i in range(n):
                one = ms[i].probs_pruned(t) if pruned else ms[i].probs(t)
                assert same_bits(got[i], one), f"tree {i}: {fn}({t}) differs from the stand-alone object"
                assert same_bits(got[i], os_[i].probs(t, pruned=pruned)), f"tree {i}: {fn}({t}) differs from the oracle"
        picked = mb.pick_moves(t)
        for i in range(n):
            assert int(picked[i]) == ms[i].pick_move(ms[i].probs(t)), f"tree {i}: pick_moves({t}) differs from the stand-alone object"
            assert int(picked[i]) == os_[i].pick_move(os_[i].probs(t)), f"tree {i}: pick_moves({t}) differs from the oracle"
    for i in (0, n - 1):
        assert _stream(ms[i]) == os_[i].rng_state()
