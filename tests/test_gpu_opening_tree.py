"""-m gpu: `MCTSBatch.expand_frontier` (azmi_search_expand / azmi_search_frontier) and `alphazero.build_opening_tree`: the
reference's opening_analysis.py build_tree (:261-355) level by level on the device.

The comparison side of a frontier is a float64 numpy restatement of evaluate_node (:233-257), play.py's apply_temperature
(:256-266) and the entropy / reach lines (:328-346), fed with the same batch's counts(), root_values() and
gumbel_improved_policies(); the children are GameState copies with play_move, hash_game_state, current_player and scores().

Exactness: with temp in {0, 1} raw_pi, sampling_pi, child_reach and the kept set are bit-identical to numpy; key, player, variant,
terminal, scores, parent and the action order always are.  For other temperatures the device's pow / log are not numpy's, so the
kept set must equal numpy's for every move with |reach * p - min_reach| > 1e-9 * min_reach, and every test asserts that no move
of its inputs lies inside that band (min_reach = 0.0437 and the seeds below: the band is empty).

Tolerance on sampling_pi, entropy and child_reach for those temperatures: the largest relative deviation from numpy over the
inputs of this file, measured on an MI355X, is 1.04e-15 (sampling_pi 1.04e-15, entropy 1.03e-15, child_reach 3.7e-16).  The bound is
64 times that, 6.7e-14 (never looser than 1e-10): the order of the lane-strided sums of up to 2662 terms.  The last test prints
the figures of the run (-s)."""
import random

import numpy as np
import pytest

from test_gpu_search_batch import _c4_at, _c4_states, _drive_alone, az  # noqa: F401
from test_gpu_search_batch_play import _C4_LAST_CELL, _C4_WIN_IN_ONE

pytestmark = pytest.mark.gpu

MIN_REACH = 0.0437
WIDE_MIN_REACH = 0.0137
BAND = 1e-9
MEASURED = 1.04e-15
TOL = min(64 * MEASURED, 1e-10)
TEMPS = (0.0, 1.0, 0.37, 2.5)
WORST = {"sampling_pi": 0.0, "entropy": 0.0, "child_reach": 0.0}


def _apply_temperature(probs, temperature):      # play.py:256-266
    if temperature == 0:
        result = np.zeros_like(probs)
        result[np.argmax(probs)] = 1.0
        return result
    elif temperature == 1.0:
        return probs
    scaled = np.power(probs + 1e-10, 1.0 / temperature)
    return scaled / scaled.sum()


def _raw_pi(counts, valids, gp=None):      # opening_analysis.py:233-257
    raw_pi = None
    if gp is not None:
        ip = np.asarray(gp, dtype=np.float64)
        if ip.sum() > 0:
            raw_pi = ip / ip.sum()
    if raw_pi is None:
        counts = np.asarray(counts, dtype=np.float64)
        total = counts.sum()
        if total <= 0:
            valids = np.asarray(valids, dtype=np.float64)
            raw_pi = valids / valids.sum() if valids.sum() > 0 else counts
        else:
            raw_pi = counts / total
    return raw_pi


def _close(what, got, want, where):
    """|got - want| <= TOL * |want| entry by entry (0 where want is 0); the largest relative deviation is kept for the header's figure"""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    assert np.array_equal(got == 0, want == 0), f"{where}: {what}: zeros differ"
    nz = want != 0
    worst = float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0
    WORST[what] = max(WORST[what], worst)
    assert worst <= TOL, f"{where}: {what} deviates from numpy by {worst:.3g} (bound {TOL:.3g})"


def _children(az, gs, actions):
    """the comparison side of the records of one root: GameState copies with play_move"""
    out = []
    for a in actions:
        c = gs.copy()
        c.play_move(int(a))
        sc = c.scores()
        out.append((az.hash_game_state(c), c.current_player(), c.get_variant_id(), sc is not None,
                    (np.zeros(3, np.float32) if sc is None else np.asarray(sc, np.float32)).tolist()))
    return out


def _check_frontier(az, mb, fr, reach, temps, min_reach, gumbel=False, children=_children):
    """fr = mb.expand_frontier(reach, temps, min_reach) against numpy on the batch's own read-outs -> total records"""
    n = len(mb)
    M = fr["raw_pi"].shape[1]
    states, finished = mb.states(), mb.finished()
    counts, rv = mb.counts(), mb.root_values()
    gp = mb.gumbel_improved_policies() if gumbel else None
    temps = np.broadcast_to(np.asarray(temps, np.float64), (n,))
    assert fr["first_child"][0] == 0 and fr["first_child"].dtype == np.uint32 and fr["raw_pi"].dtype == np.float64
    r = 0
    for i in range(n):
        gs = states[i]
        assert fr["first_child"][i] == r, f"tree {i}"
        if finished[i] or reach[i] == 0:
            assert fr["kind"][i] == 2 and fr["key"][i] == 0 and not fr["raw_pi"][i].any() and not fr["sampling_pi"][i].any()
            assert fr["entropy"][i] == 0 and not fr["value"][i].any()
            continue
        assert fr["key"][i] == az.hash_game_state(gs), f"tree {i}"
        sc = gs.scores()
        if sc is not None:
            assert fr["kind"][i] == 1 and np.array_equal(fr["value"][i], np.asarray(sc, np.float64))
            assert not fr["raw_pi"][i].any() and not fr["sampling_pi"][i].any() and fr["entropy"][i] == 0
            continue
        assert fr["kind"][i] == 0
        valids = gs.valid_moves()
        raw = _raw_pi(counts[i], valids, None if gp is None else gp[i])
        samp = _apply_temperature(raw, temps[i])
        safe = samp[samp > 0]
        entropy = float(-np.sum(safe * np.log(safe))) if safe.size > 0 else 0.0
        assert np.array_equal(fr["raw_pi"][i], raw), f"tree {i}: raw_pi"
        assert np.array_equal(fr["value"][i], np.asarray(rv[i], np.float64)), f"tree {i}: value"
        exact = temps[i] in (0.0, 1.0)
        if exact:
            assert np.array_equal(fr["sampling_pi"][i], samp), f"tree {i}: sampling_pi"
        else:
            _close("sampling_pi", fr["sampling_pi"][i], samp, f"tree {i}")
        _close("entropy", fr["entropy"][i], entropy, f"tree {i}")      # (log is the device's for every temperature)
        cr = reach[i] * samp
        if not exact:
            assert not np.any((samp > 0) & (np.abs(cr - min_reach) <= BAND * min_reach)), f"tree {i}: a move lies inside the band"
        kept = np.flatnonzero((samp > 0) & (cr >= min_reach) & (valids != 0))
        k = len(kept)
        assert fr["first_child"][i + 1] == r + k, f"tree {i}: {fr['first_child'][i + 1] - r} kept, numpy keeps {k}"
        assert fr["action"][r: r + k].tolist() == kept.tolist() and (fr["parent"][r: r + k] == i).all(), f"tree {i}"
        if exact:
            assert np.array_equal(fr["child_reach"][r: r + k], cr[kept]), f"tree {i}: child_reach"
        elif k:
            _close("child_reach", fr["child_reach"][r: r + k], cr[kept], f"tree {i}")
        got = list(zip(fr["child_key"][r: r + k].tolist(), fr["child_player"][r: r + k].tolist(), fr["child_variant"][r: r + k].tolist(),
                       fr["child_terminal"][r: r + k].tolist(), fr["child_scores"][r: r + k].tolist()))
        assert got == children(az, gs, kept), f"tree {i}: records"
        r += k
    assert fr["first_child"][n] == r and all(len(fr[k]) == r for k in ("parent", "action", "child_reach", "child_key", "child_player",
                                                                         "child_variant", "child_terminal", "child_scores"))
    return r


def _c4_children_by_replay(az, gs, actions):
    """the same records from one batched rules replay (hash_game_state / current_player / scores of GameState come from it)"""
    if not len(actions):
        return []
    moves = -np.ones((len(actions), len(gs._moves) + 2), np.int32)
    for j, a in enumerate(actions):
        moves[j, : len(gs._moves) + 1] = gs._moves + [int(a)]
    out = az.game_replay(type(gs), moves)
    assert (out["status"] == 0).all()
    return [(int(out["key"][j]), int(out["player"][j]), -1, bool(out["scores"][j][0] >= 0),
             (out["scores"][j] if out["scores"][j][0] >= 0 else np.zeros(3, np.float32)).tolist()) for j in range(len(actions))]


# ---- 1. shapes: one tree, a few, past one workgroup's 32 trees -------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 33])
def test_connect4_frontier_is_the_numpy_restatement(az, n):
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=24, seeds=[4100 + 7 * i for i in range(n)])
    mb.reset(_c4_states(az, n, seed=90 + n))
    mb.search(24)
    reach = np.random.default_rng(n).uniform(0.05, 1.0, n)
    temps = [TEMPS[(i + n) % 4] for i in range(n)]
    l0 = mb.stats()["launches"]
    fr = mb.expand_frontier(reach, temps, MIN_REACH)
    assert mb.stats()["launches"] - l0 == 3, "policies, scan, records: three launches whatever n is"
    assert _check_frontier(az, mb, fr, reach, temps, MIN_REACH) > 0


def test_connect4_1030_trees_cross_the_scan_boundary(az):
    """n = 1030: k_frontier_scan takes two trees per thread and the records cross the 1024 boundary; 8 random visits"""
    n = 1030
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=8, seeds=[77000 + i for i in range(n)])
    mb.reset(_c4_states(az, n, seed=5, max_len=8))
    mb.search(8)
    reach = np.random.default_rng(2).uniform(0.05, 1.0, n)
    temps = [TEMPS[i % 4] for i in range(n)]
    l0 = mb.stats()["launches"]
    fr = mb.expand_frontier(reach, temps, MIN_REACH)
    assert mb.stats()["launches"] - l0 == 3
    total = _check_frontier(az, mb, fr, reach, temps, MIN_REACH, children=_c4_children_by_replay)
    assert total > 1024 and fr["parent"][1023] <= fr["parent"][1024] and np.all(np.diff(fr["parent"].astype(np.int64)) >= 0)


# ---- 2. the wide games: one wavefront per tree -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,evaluator", [("BrandubhGS", "random"), ("TawlbwrddGS", "playout"), ("StarGambitUnifiedGS", "random")])
def test_wide_game_frontier(az, name, evaluator):
    """n = 2.  Tawlbwrdd: M = 2662, 42 moves per lane in the per-tree scan.  StarGambit unified: the variant field, and several
    actions per turn (the player to move is unchanged after a move).  64 visits over dozens of root moves leave most
    children one visit, p = 1 / 64: the threshold of these games sits below that."""
    Game = getattr(az, name)
    random.seed(11)      # an unpinned StarGambit object draws its variant from Python's `random`
    start = [Game(-1, [0.25] * 4) if name == "StarGambitUnifiedGS" else Game() for _ in range(2)]
    first = int(np.flatnonzero(start[1].valid_moves())[3])
    start[1].play_move(first)
    mb = az.MCTSBatch(Game, 2, 1.25, max_simulations=64, seeds=[31, 32])
    mb.reset(start)
    mb.search(64, evaluator=evaluator)
    reach, temps = [1.0, 0.6], [1.0, 0.37]
    l0 = mb.stats()["launches"]
    fr = mb.expand_frontier(reach, temps, WIDE_MIN_REACH)
    assert mb.stats()["launches"] - l0 == 3
    assert _check_frontier(az, mb, fr, reach, temps, WIDE_MIN_REACH) > 0
    if name == "StarGambitUnifiedGS":
        assert set(fr["child_variant"].tolist()) <= {0, 1, 2, 3} and fr["child_variant"][0] == start[0].get_variant_id()
    else:
        assert set(fr["child_variant"].tolist()) == {-1}
    again = mb.expand_frontier(reach, [0.0, 2.5], WIDE_MIN_REACH)      # the other two temperature branches on the same searches
    _check_frontier(az, mb, again, reach, [0.0, 2.5], WIDE_MIN_REACH)


# ---- 3. placed positions -------------------------------------------------------------------------------------------------------
def test_placed_connect4_positions(az):
    """tree 0: one move from a win (a terminal child with scores); 1: a full column (an illegal move with p > 0 under temp 2.5);
    2: a terminal root (kind 1); 3: finished by a move played on the batch (kind 2); 4: reach 0 (kind 2); 5: one descent only
    (uniform over the legal moves); 6, 7: temp 0 and 0.37"""
    n = 8
    full = (3, 3, 3, 3, 3, 3)
    states = [_c4_at(az, p) for p in [_C4_WIN_IN_ONE, full, _C4_WIN_IN_ONE + (0,), _C4_LAST_CELL, (2, 4), full, (3, 3, 2), (1, 6, 3, 6)]]
    assert states[2].scores() is not None
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=64, seeds=[500 + i for i in range(n)])
    mb.reset(states)
    last = int(np.flatnonzero(states[3].valid_moves())[0])
    mb.update_roots([-1, -1, -1, last, -1, -1, -1, -1])
    assert mb.finished().tolist() == [False, False, False, True, False, False, False, False]
    mb.search_to([24, 24, 24, 24, 24, 1, 24, 24])
    assert mb.counts()[5].sum() == 0, "one descent only expands the root"
    reach = [1.0, 0.9, 0.5, 0.7, 0.0, 0.8, 0.3, 1.0]
    temps = [1.0, 2.5, 1.0, 1.0, 1.0, 1.0, 0.0, 0.37]
    fr = mb.expand_frontier(reach, temps, MIN_REACH)
    _check_frontier(az, mb, fr, reach, temps, MIN_REACH)
    assert fr["kind"].tolist() == [0, 0, 1, 2, 2, 0, 0, 0]
    assert fr["value"][2].tolist() == [1.0, 0.0, 0.0]
    lo, hi = fr["first_child"][0], fr["first_child"][1]
    win = np.flatnonzero(fr["action"][lo:hi] == 0)
    assert len(win) == 1 and fr["child_terminal"][lo + win[0]] and fr["child_scores"][lo + win[0]].tolist() == [1.0, 0.0, 0.0]
    assert not fr["child_terminal"][lo:hi][fr["action"][lo:hi] != 0].any()
    assert fr["sampling_pi"][1][3] > 0 and fr["raw_pi"][1][3] == 0, "the `+ 1e-10` gives the full column a tiny mass"
    uniform = fr["raw_pi"][5]
    assert uniform[3] == 0 and np.array_equal(uniform[[0, 1, 2, 4, 5, 6]], np.full(6, 1.0 / 6.0))
    assert np.count_nonzero(fr["sampling_pi"][6]) == 1 and fr["first_child"][7] - fr["first_child"][6] == 1
    # a threshold low enough for the full column's mass: the move is illegal, so it is not kept
    low = 1e-7
    assert 0.9 * fr["sampling_pi"][1][3] >= low
    fr2 = mb.expand_frontier(reach, temps, low)
    _check_frontier(az, mb, fr2, reach, temps, low)
    lo, hi = fr2["first_child"][1], fr2["first_child"][2]
    assert 3 not in fr2["action"][lo:hi].tolist() and hi - lo == 6
    # a min_reach that keeps nothing
    none = mb.expand_frontier(reach, temps, 2.0)
    assert none["first_child"].tolist() == [0] * (n + 1) and len(none["parent"]) == 0 and none["child_scores"].shape == (0, 3)
    assert np.array_equal(none["sampling_pi"], fr["sampling_pi"]) and np.array_equal(none["kind"], fr["kind"])


def test_gumbel_batch_uses_the_improved_policy(az):
    n = 4
    mb = az.MCTSBatch(az.Connect4GS, n, 2.0, gumbel_enabled=True, gumbel_m=4, max_simulations=16, seeds=[900 + 5 * i for i in range(n)])
    mb.reset([_c4_at(az, p) for p in [(), (3, 3, 2), (1, 6, 3, 6, 4, 2, 2), (2, 4)]])
    mb.search(16)
    reach, temps = [1.0, 0.5, 0.8, 0.6], [1.0, 1.0, 0.0, 0.37]
    fr = mb.expand_frontier(reach, temps, MIN_REACH)
    _check_frontier(az, mb, fr, reach, temps, MIN_REACH, gumbel=True)
    gp = mb.gumbel_improved_policies().astype(np.float64)
    assert np.array_equal(fr["raw_pi"][0], gp[0] / gp[0].sum())
    counts = mb.counts()[0].astype(np.float64)
    assert not np.array_equal(fr["raw_pi"][0], counts / counts.sum()), "not the visit counts"


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------
def test_overflow_names_both_numbers_and_the_batch_stays_usable(az):
    n = 5
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=64, seeds=[60 + i for i in range(n)])
    mb.reset(_c4_states(az, n, seed=3))
    mb.search(24)
    reach = [1.0] * n
    full = mb.expand_frontier(reach, 1.0, MIN_REACH)
    total = len(full["parent"])
    assert total > 1
    with pytest.raises(RuntimeError, match=rf"keep {total} children, max_children = {total - 1}"):
        mb.expand_frontier(reach, 1.0, MIN_REACH, max_children=total - 1)
    exact = mb.expand_frontier(reach, 1.0, MIN_REACH, max_children=total)      # exactly enough room
    assert all(np.array_equal(full[k], exact[k]) for k in full)
    mb.search(24)                                                              # still usable
    more = mb.expand_frontier(reach, 1.0, MIN_REACH, max_children=10 * total)  # and the record buffers regrow
    _check_frontier(az, mb, more, reach, 1.0, MIN_REACH)
    canon, idx = mb.find_leaves(numpy=True)
    with pytest.raises(RuntimeError, match="expand_frontier: a find_leaves step is pending"):
        mb.expand_frontier(reach, 1.0, MIN_REACH)
    mb.process_results(np.full((len(idx), 3), 1 / 3, np.float32), np.full((len(idx), 7), 1 / 7, np.float32))
    _check_frontier(az, mb, mb.expand_frontier(reach, 1.0, MIN_REACH), reach, 1.0, MIN_REACH)


def test_frontier_before_any_expand_is_a_state_error(az):
    from alphazero import _capi
    mb = az.MCTSBatch(az.Connect4GS, 2, 1.25, max_simulations=8, seeds=[1, 2])
    mb.reset([az.Connect4GS(), az.Connect4GS()])
    assert _capi.lib.azmi_search_frontier(mb._h, *([None] * 15)) == -5
    assert "no expand_frontier call" in _capi.lib.azmi_last_error().decode()
    unready = az.MCTSBatch(az.Connect4GS, 2, 1.25, max_simulations=8)
    with pytest.raises(RuntimeError, match="call reset first"):
        unready.expand_frontier([1.0, 1.0], 1.0, 0.01)


# ---- 5. an expand in between changes nothing ------------------------------------------------------------------------------------
def test_a_batch_that_never_expands_is_untouched(az):
    def run(expand):
        mb = az.MCTSBatch(az.Connect4GS, 6, 1.25, fpu_reduction=0.25, max_simulations=40, seeds=[800 + i for i in range(6)])
        mb.reset(_c4_states(az, 6, seed=17))
        mb.search(20)
        if expand:
            mb.expand_frontier([1.0] * 6, [0.0, 1.0, 0.37, 2.5, 1.0, 1.0], MIN_REACH)
        mb.search(20)
        mb.pick_moves(1.0)
        return mb, dict(counts=mb.counts(), q=mb.root_q_values(), rv=mb.root_values(), p=mb.probs(1.0), n=mb.root_ns(), d=mb.depths())
    a, ra = run(False)
    b, rb = run(True)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    sa, sb = a.stats(), b.stats()
    assert sb["launches"] - sa["launches"] == 3 and all(sa[k] == sb[k] for k in sa if k != "launches")


# ---- 6. build_opening_tree ------------------------------------------------------------------------------------------------------
def _reference_tree(az, start, sims, min_reach, seed, start_temp=1.0, final_temp=0.2, half_life=10):
    """opening_analysis.py build_tree with one stand-alone MCTS(seed = node_seed(seed, b)) per node, visited in BFS order"""
    nodes = [dict(state=start.copy(), depth=0, reach=1.0, parent=-1, action=-1)]
    b = 0
    while b < len(nodes):
        nd = nodes[b]
        gs = nd["state"]
        nd["hash"] = az.hash_game_state(gs)
        sc = gs.scores()
        if sc is not None:
            nd.update(terminal=True, value=np.asarray(sc, np.float64), raw_pi=np.zeros(0), sampling_pi=np.zeros(0), entropy=0.0)
            b += 1
            continue
        m = az.MCTS(1.25, 2, 7, seed=az.node_seed(seed, b), max_simulations=sims)
        _drive_alone(az, m, gs, sims)
        raw = _raw_pi(m.counts(), gs.valid_moves())
        samp = _apply_temperature(raw, az.temperature_at_depth(nd["depth"], start_temp, final_temp, half_life))
        safe = samp[samp > 0]
        nd.update(terminal=False, value=np.asarray(m.root_value(), np.float64), raw_pi=raw, sampling_pi=samp,
                  entropy=float(-np.sum(safe * np.log(safe))) if safe.size > 0 else 0.0)
        for a in range(len(samp)):
            p = float(samp[a])
            if p <= 0.0:
                continue
            cr = nd["reach"] * p
            assert abs(cr - min_reach) > BAND * min_reach, f"node {b}, move {a}: inside the band"
            if cr < min_reach:
                continue
            child = gs.copy()
            child.play_move(a)
            nodes.append(dict(state=child, depth=nd["depth"] + 1, reach=cr, parent=b, action=a))
        b += 1
    return nodes


@pytest.fixture(scope="module")
def c4_tree(az):
    return az.build_opening_tree(az.Connect4GS, az.Connect4GS(), 24, evaluator="random", min_reach=0.02, batch=8, seed=5)


def test_connect4_tree_equals_the_reference_recursion(az, c4_tree):
    tree = c4_tree
    ref = _reference_tree(az, az.Connect4GS(), 24, 0.02, 5)
    assert len(tree) == len(ref) and len(tree) > 16
    assert tree.parent.tolist() == [nd["parent"] for nd in ref] and tree.incoming_action.tolist() == [nd["action"] for nd in ref]
    assert tree.depth.tolist() == [nd["depth"] for nd in ref] and tree.state_hash.tolist() == [nd["hash"] for nd in ref]
    assert tree.is_terminal.tolist() == [nd["terminal"] for nd in ref]
    for b, nd in enumerate(ref):
        assert abs(tree.reach_prob[b] - nd["reach"]) <= TOL * nd["reach"] * (nd["depth"] + 1), b
        assert np.array_equal(tree.value[b], nd["value"]), b
        if nd["terminal"]:
            assert not tree.searched[b] and tree.entropy[b] == 0
            continue
        assert np.array_equal(tree.raw_pi[b], nd["raw_pi"]), b
        assert np.allclose(tree.sampling_pi[b], nd["sampling_pi"], rtol=TOL, atol=0), b
        assert abs(tree.entropy[b] - nd["entropy"]) <= TOL * abs(nd["entropy"]), b
        assert az.hash_game_state(tree.state(b)) == nd["hash"] and tree.state(b)._moves == nd["state"]._moves
    levels = int(tree.depth[tree.searched].max()) + 1
    chunks = sum(-(-int(np.sum(tree.searched & (tree.depth == d))) // 8) for d in range(levels))
    assert tree.stats == dict(levels=levels, chunks=chunks, host_reads=chunks) and chunks > levels, "levels span several chunks"
    # children: neighbours in ascending action order
    for b in range(len(tree)):
        first, count = tree.children[b]
        kids = np.flatnonzero(tree.parent == b)
        assert count == len(kids) and (count == 0 or kids.tolist() == list(range(first, first + count)))
        assert np.all(np.diff(tree.incoming_action[kids]) > 0)
    # the nested view carries the reference TreeNode's fields
    root = tree.nodes()
    assert root.incoming_action is None and root.depth == 0 and root.reach_prob == 1.0 and not root.is_terminal
    assert sorted(root.children) == tree.incoming_action[tree.parent == 0].tolist()
    kid = root.children[min(root.children)]
    assert kid.depth == 1 and kid.state_hash == int(tree.state_hash[1]) and kid.state._moves == [kid.incoming_action]
    count = lambda nd: 1 + sum(count(c) for c in nd.children.values())      # noqa: E731
    assert count(root) == len(tree)


def test_the_tree_does_not_depend_on_chunking(az, c4_tree):
    other = az.build_opening_tree(az.Connect4GS, az.Connect4GS(), 24, evaluator="random", min_reach=0.02, batch=64, seed=5)
    for k in ("parent", "depth", "incoming_action", "reach_prob", "state_hash", "is_terminal", "searched", "entropy", "value", "raw_pi",
              "sampling_pi", "children"):
        assert np.array_equal(getattr(other, k), getattr(c4_tree, k)), k
    assert other.stats["chunks"] < c4_tree.stats["chunks"] and other.stats["levels"] == c4_tree.stats["levels"]


def test_brandubh_playout_tree_stops_at_max_depth(az):
    """64 rollouts over dozens of root moves, sharpened by a temperature of 0.3 so that a few moves carry the mass two plies deep"""
    tree = az.build_opening_tree(az.BrandubhGS, az.BrandubhGS(), 64, evaluator="playout", min_reach=WIDE_MIN_REACH, batch=4, seed=9, max_depth=2,
                                 start_temp=0.3, final_temp=0.3)
    assert tree.depth.max() == 2 and tree.stats["levels"] == 2 and len(tree) > 3
    edge = tree.depth == 2
    assert not tree.searched[edge].any() and not tree.is_terminal[edge].any() and not tree.value[edge].any()
    assert tree.searched[tree.depth < 2].all()
    for b in (0, 1, len(tree) - 1):
        assert int(tree.state_hash[b]) == az.hash_game_state(tree.state(b))
    for b in np.flatnonzero(tree.searched):
        first, count = tree.children[b]
        kids = slice(first, first + count)
        assert np.array_equal(tree.reach_prob[kids], tree.reach_prob[b] * tree.sampling_pi[b][tree.incoming_action[kids]])
        assert np.all(tree.reach_prob[kids] >= WIDE_MIN_REACH)


def test_a_net_and_a_shared_cache_one_read_per_chunk(az):
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    net = az.HipLeafNet(torch_net.random_init(spec, seed=3), spec)
    cache = az.ShardedS3FIFOCache.for_engine(1 << 12, 7, 3)
    tree = az.build_opening_tree(az.Connect4GS, az.Connect4GS(), 16, net=net, cache=cache, min_reach=0.1, batch=8, seed=1)
    assert len(tree) > 1 and tree.stats["host_reads"] == tree.stats["chunks"] >= tree.stats["levels"]
    assert abs(tree.sampling_pi[0].sum() - 1.0) < 1e-12 and tree.searched[0]


def test_readme_opening_tree_snippet():
    import alphazero
    tree = alphazero.build_opening_tree(alphazero.Connect4GS, alphazero.Connect4GS(), 32, evaluator="random", min_reach=0.05, batch=64)
    line = [0]
    while tree.children[line[-1]][1]:                          # follow the likeliest move from the start position
        first, count = tree.children[line[-1]]
        line.append(first + int(np.argmax(tree.reach_prob[first: first + count])))
    assert len(tree) > 1 and tree.depth[line].tolist() == list(range(len(line)))
    assert tree.state(line[-1])._moves == tree.incoming_action[line[1:]].tolist()


def test_zz_report_the_measured_deviation():
    """the figure of the header: printed with -s; nothing above exceeded the bound"""
    print("opening tree: largest relative deviation from numpy:", WORST, "bound", TOL)
    assert max(WORST.values()) <= TOL
