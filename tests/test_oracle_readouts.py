"""The oracle's root read-outs against the plain restatement of tests/mcts_readout_ref.py, on trees grown with the scripted
sharp evaluators, at every temperature the device tests use: bit for bit.  This pins the checker at inputs it has not been
asked about (sharp priors, zero priors, saturated q, small temperatures) before tests/test_gpu_mcts_readouts.py holds the
device to it.  No GPU."""
import numpy as np
import pytest

import mcts_readout_ref as ref
from mcts_readout_ref import TEMPS, same_bits

CONFIGS = {
    "puct": dict(cpuct=1.25),
    "noise": dict(cpuct=1.25, epsilon=0.25, root_policy_temp=1.25, shaped_dirichlet=True, root_fpu_zero=True),
}
SIMS, PLIES = 24, 4


def _root(o, cpuct):
    mv, n, q, pol, d = o.root_children_full()
    rv, rd, rn = o.root_node()
    assert rn == o.root_n()
    return ref.Root(mv, n, q, pol, d, rn, rv, rd, cpuct, o.P, o.M)


def _check_readouts(o, cpuct, what, finite):
    """every read-out of the oracle equals the restatement's; `finite`: the oracle-alone condition of the device tests - at
    every temperature of at least 0.05 every vector is finite and sums to 1 within 1e-5"""
    r = _root(o, cpuct)
    assert np.array_equal(o.counts(), ref.counts(r)), what
    assert same_bits(o.root_q(), ref.root_q(r)), what
    assert same_bits(o.root_value(), ref.root_value(r)), what
    assert same_bits([o.entropy()], [ref.normalized_root_entropy(r)]), what
    vectors = []
    for t in TEMPS:
        for pruned in (False, True):
            got = o.probs(t, pruned=pruned)
            want = (ref.probs_pruned if pruned else ref.probs)(r, t)
            assert same_bits(got, want), f"{what}: {'probs_pruned' if pruned else 'probs'}({t}): {got[got != want]} vs {want[got != want]}"
            if finite:
                assert np.isfinite(got).all(), f"{what}: temp {t}, pruned {pruned}: a non-finite entry"
                assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-5, f"{what}: temp {t}, pruned {pruned}: sum {got.sum()}"
            vectors.append((t, pruned, got))
    return vectors


def _check_picks(o, vectors, what):
    moves = []
    for t, pruned, p in vectors:
        mv = o.pick_move(p)
        assert mv == ref.pick_move(p, o.last_uniform()), f"{what}: pick_move at temp {t}, pruned {pruned}"
        assert p[mv] > 0
        moves.append(mv)
    return moves


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("game", ["connect4", "brandubh"])
def test_oracle_readouts_equal_the_restatement(oracle, game, cfg):
    gid = dict(connect4=oracle.GAME_CONNECT4, brandubh=oracle.GAME_BRANDUBH)[game]
    kw = dict(CONFIGS[cfg]); cpuct = kw.pop("cpuct")
    noise = kw.get("epsilon", 0) > 0
    og = oracle.Game(gid)
    o = oracle.Mcts(cpuct, 2, og.num_moves(), seed=31, **kw)
    seen_patterns = set()
    for ply in range(PLIES):
        for _ in range(SIMS):
            leaf = o.find_leaf(og)
            if leaf.scores() is not None:
                v, pi = np.full(3, 1 / 3, np.float32), np.zeros(o.M, np.float32)
            else:
                canon = leaf.canonical()
                v, pi = ref.sharp_eval(canon, leaf.valid())
                seen_patterns.add(ref._stable_hash(canon) % len(ref.POLICY_PATTERNS))
            o.process_result(v, pi, noise)
        vectors = _check_readouts(o, cpuct, f"{game}/{cfg} ply {ply}", finite=True)
        moves = _check_picks(o, vectors, f"{game}/{cfg} ply {ply}")
        move = moves[2 * ((ply + 1) % len(TEMPS))]          # the pick from probs(1), probs(2), probs(0.5), probs(0.2)
        o.update_root(og, move); og.play(move)
        assert og.scores() is None
        if noise:
            o.apply_root_policy_temp()
            if o.root_n() > 0:
                o.add_root_noise()
        # the reused root before any new simulation is a read-out state of its own
        _check_readouts(o, cpuct, f"{game}/{cfg} reused root after ply {ply}", finite=o.root_n() > 0)
    assert len(seen_patterns) == len(ref.POLICY_PATTERNS), "the scripted evaluator did not reach every policy pattern"


@pytest.mark.parametrize("game", ["connect4", "brandubh"])
def test_oracle_shallow_roots_equal_the_restatement(oracle, game):
    """0, 1, 2 and k + 1 simulations with the uniform evaluator: no children (NaN vectors), the prior branch, one visited child,
    every child visited once (all counts tie)"""
    gid = dict(connect4=oracle.GAME_CONNECT4, brandubh=oracle.GAME_BRANDUBH)[game]
    og = oracle.Game(gid)
    k = int(og.valid().sum())
    for sims in (0, 1, 2, k + 1):
        o = oracle.Mcts(1.25, 2, og.num_moves(), seed=7)
        for _ in range(sims):
            leaf = o.find_leaf(og)
            v, pi = oracle.dumb_eval(leaf)
            o.process_result(v, pi)
        vectors = _check_readouts(o, 1.25, f"{game} after {sims} simulations", finite=sims > 0)
        if sims == 0:
            assert all(np.isnan(p).all() for _, _, p in vectors)       # 0 / 0 everywhere: nothing to pick from
            continue
        _check_picks(o, vectors, f"{game} after {sims} simulations")
        if sims == k + 1:
            assert (o.counts()[og.valid() == 1] == 1).all()
            for t, pruned, p in vectors:
                if t == 0.0:
                    assert np.array_equal(p, np.where(og.valid() == 1, np.float32(1.0 / k), np.float32(0))), (pruned, p)


def test_sharp_eval_patterns():
    """the evaluator is a pure function and gives the rows it promises"""
    canon = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    valid = np.array([1, 0, 1, 1, 0, 1, 1], np.uint8)
    a = ref.sharp_eval(canon, valid); b = ref.sharp_eval(canon.copy(), valid.copy())
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    rows = {p: ref.sharp_eval(canon, valid, policy_pattern=p)[1] for p in ref.POLICY_PATTERNS}
    legal = valid == 1
    assert sorted(rows["one_hot"].tolist()) == [0] * 6 + [1] and rows["one_hot"][~legal].sum() == 0
    assert sorted(rows["peak_and_dust"][legal].tolist()) == [np.float32(1e-30)] * 4 + [np.float32(0.999)]
    assert 2 <= int((rows["half_zero"][legal] == 0).sum()) <= 3 and rows["half_zero"][legal].sum() == pytest.approx(1.0)
    assert rows["mass_on_illegal"][~legal].sum() == pytest.approx(0.9) and rows["mass_on_illegal"][legal].sum() == pytest.approx(0.1)
    assert rows["sums_to_3p7"].sum() == pytest.approx(3.7) and rows["sums_to_3p7"][~legal].sum() == 0
    d = rows["denormals"][legal]
    tiny = np.finfo(np.float32).tiny
    assert int((d == 0.5).sum()) == 1 and int(((d > 0) & (d < tiny)).sum()) == 4
    assert {tuple(ref.sharp_eval(canon, valid, value_pattern=i)[0]) for i in range(4)} == set(ref.VALUE_PATTERNS)
