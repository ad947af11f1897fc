"""-m gpu: `alphazero.MCTSBatch(..., descents_per_step=L)`: a tree goes on descending inside a step while its leaves need no
evaluator (terminal, RANDOM, cache hit).  The contract: tree i makes the same find_leaf / process_result calls as with L = 1,
so every read-out and the tree's stream position equal the L = 1 batch bit for bit (np.array_equal), and a search needs
fewer steps.  The L = 1 batch itself is pinned to the stand-alone object and the oracle by tests/test_gpu_search_batch*.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_search_batch import _c4_at, _c4_states, _drive_alone, az, c4_net  # noqa: F401

pytestmark = pytest.mark.gpu

N, VISITS = 37, 48          # one full 32-slot workgroup of the Connect4 kernels and a partial one
LS = (2, 8, 64)             # 64 > VISITS: the whole search fits one step where no leaf needs the evaluator

# Connect4: columns 0-5 full without a four (cell (row, col) belongs to player (row + col // 2) % 2), column 6 empty
_C4_ONE_COLUMN = (0,) * 6 + (1,) * 6 + (4,) + (2,) * 6 + (3,) * 6 + (4,) * 5 + (5,) * 6
_C4_SPECIAL = [(), (3, 3, 2), (1, 6, 3, 6, 4, 2, 2), (0, 1, 0, 1, 0, 1), _C4_ONE_COLUMN, _C4_ONE_COLUMN + (6,) * 3,
               _C4_ONE_COLUMN + (6,) * 4]

# Connect4 positions in which EVERY legal move ends the game (a win or the full board), with 1, 1, 3, 2, 4 and 5 legal moves:
# found by random play with the rules of _c4_wins; the test checks them with Connect4GS
_C4_ALL_TERMINAL = [
    _C4_ONE_COLUMN + (6,) * 5,
    (1, 0, 4, 2, 2, 6, 5, 3, 6, 3, 6, 4, 2, 3, 4, 5, 6, 1, 0, 2, 4, 6, 6, 2, 0, 5, 1, 0, 1, 4, 3, 2, 1, 3, 4, 5, 5, 0, 3, 1, 0),
    (5, 1, 3, 4, 3, 3, 0, 5, 5, 4, 0, 5, 3, 0, 3, 1, 0, 6, 1, 4, 5, 6, 5, 0, 6, 3, 6, 0, 6, 1, 4, 1, 1, 2),
    (3, 4, 4, 3, 3, 3, 6, 6, 2, 0, 6, 1, 4, 4, 5, 6, 2, 2, 1, 2, 4, 6, 2, 4, 3, 3, 0, 1, 1, 6, 0, 2, 0, 1, 1, 5),
    (4, 0, 0, 0, 6, 4, 6, 2, 3, 5, 0, 6, 4, 2, 4, 3, 4, 3, 6, 3, 1, 4, 0, 0, 6, 6, 2),
    (5, 5, 1, 4, 1, 6, 3, 1, 2, 1, 4, 0, 1, 4, 0, 4, 1, 3, 0, 0, 0, 6, 6, 6, 0, 5, 3, 4, 2, 5, 3),
]

KINDS = ("random", "net", "net+cache", "playout", "gumbel")


def _positions(az):
    """start positions, mid-game positions, positions two or three plies from the end of the game"""
    states = [_c4_at(az, p) for p in _C4_SPECIAL] + _c4_states(az, N - len(_C4_SPECIAL), seed=7, max_len=30)
    assert len(states) == N and all(g.scores() is None for g in states)
    assert 42 - len(_C4_SPECIAL[-1]) == 2 and 42 - len(_C4_SPECIAL[-2]) == 3
    return states


def _search_kw(az, kind, net, num_moves=7):
    if kind == "random":
        return dict(evaluator="random")
    if kind == "playout":
        return dict(evaluator="playout")
    if kind == "net+cache":
        return dict(net=net, cache=az.ShardedS3FIFOCache.for_engine(1 << 10, num_moves, 3))      # small: entries are evicted
    return dict(net=net)


def _readout(mb):
    out = dict(counts=mb.counts(), rv=mb.root_values(), q=mb.root_q_values(), p1=mb.probs(1.0), root_n=mb.root_ns(), depth=mb.depths())
    out["moves"] = mb.pick_moves(1.0)       # drawn from every tree's own stream: proves the stream position
    return out


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs in trees {np.flatnonzero((np.asarray(a[k]) != np.asarray(b[k])).reshape(len(a[k]), -1).any(1)).tolist()}"


def _c4_search(az, kind, L, net):
    seeds = [4000 + 13 * i for i in range(N)]
    kw = dict(gumbel_enabled=True, gumbel_m=4) if kind == "gumbel" else dict(fpu_reduction=0.25, epsilon=0.25)
    mb = az.MCTSBatch(az.Connect4GS, N, 2.0 if kind == "gumbel" else 1.25, max_simulations=VISITS + 8, seeds=seeds, descents_per_step=L, **kw)
    assert mb.descents_per_step == L and mb.leaves_per_step == 1
    mb.reset(_positions(az))
    s0 = mb.stats()
    mb.search(VISITS, root_noise=kind != "gumbel", **_search_kw(az, kind, net))
    s1 = mb.stats()
    out = _readout(mb)
    assert out["depth"].tolist() == [VISITS] * N
    return out, {k: s1[k] - s0[k] for k in s1}, mb


@pytest.fixture(scope="module")
def c4_reference(az, c4_net):
    """the L = 1 batch of every evaluator, searched once and left unchanged"""
    memo = {}

    def get(kind):
        if kind not in memo:
            memo[kind] = _c4_search(az, kind, 1, c4_net)[:2]
        return memo[kind]
    return get


# ---- 1. Connect4: every evaluator, every L, bit for bit the L = 1 batch -----------------------------------------------------------
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("kind", KINDS)
def test_connect4_equals_one_descent_per_step(az, c4_net, c4_reference, kind, L):
    want, d1 = c4_reference(kind)
    got, d, _ = _c4_search(az, kind, L, c4_net)
    _assert_same(want, got, f"{kind}, L = {L}")
    assert d1["steps"] == VISITS and d1["host_reads"] == 0
    assert d["simulations"] == d1["simulations"] == N * VISITS and d["terminal_leaves"] == d1["terminal_leaves"]
    assert -(-VISITS // L) <= d["steps"] <= VISITS
    if kind == "random":
        # every leaf is immediate: exactly ceil(visits / L) steps of one launch each (+ the counter launch), nothing read
        assert d["steps"] == -(-VISITS // L) and d["host_reads"] == 0 and d["launches"] == d["steps"] + 1 and d["net_calls"] == 0
    else:
        assert 1 <= d["host_reads"] <= 1 + int(np.ceil(np.log2(VISITS)))
    if kind in ("net", "playout", "gumbel"):      # no cache: the same leaves reach the evaluator
        assert d["evaluator_leaves"] == d1["evaluator_leaves"]
    assert d["terminal_leaves"] > 0               # the late positions did end descents in terminal nodes


def test_random_against_the_stand_alone_object(az):
    """three of the trees (a start position, a mid-game one, one three plies from the end) against alphazero.MCTS driven call by call"""
    got, _, _ = _c4_search(az, "random", 8, None)
    states = _positions(az)
    for i in (0, 5, 20):
        m = az.MCTS(1.25, 2, 7, game=az.Connect4GS, seed=4000 + 13 * i, max_simulations=VISITS + 8, fpu_reduction=0.25, epsilon=0.25)
        _drive_alone(az, m, states[i], VISITS, noise=True)
        assert np.array_equal(got["counts"][i], m.counts()) and np.array_equal(got["q"][i], m.root_q_values()), f"tree {i}"
        assert np.array_equal(got["rv"][i], m.root_value()) and np.array_equal(got["p1"][i], m.probs(1.0)), f"tree {i}"
        assert int(got["root_n"][i]) == m.root_n() and int(got["depth"][i]) == m.depth() == VISITS
        assert int(got["moves"][i]) == m.pick_move(m.probs(1.0)), f"tree {i}: the stream is elsewhere"


# ---- 2. the wavefront-per-tree engine -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brandubh(az):
    from alphazero import torch_net
    spec = torch_net.brandubh_spec()
    net = az.HipLeafNet(torch_net.random_init(spec, seed=4), spec)
    rng = np.random.default_rng(11)
    states, gs = [], az.BrandubhGS()
    for _ in range(5):
        states.append(gs.copy())
        for _ in range(2):
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            assert gs.scores() is None
    memo = {}

    def search(kind, L):
        if (kind, L) not in memo:
            mb = az.MCTSBatch(az.BrandubhGS, 5, 1.25, fpu_reduction=0.25, max_simulations=32, seeds=[31 + i for i in range(5)], descents_per_step=L)
            mb.reset(states)
            s0 = mb.stats()
            mb.search(24, **_search_kw(az, kind, net, az.BrandubhGS.NUM_MOVES()))
            s1 = mb.stats()
            memo[kind, L] = (_readout(mb), {k: s1[k] - s0[k] for k in s1})
        return memo[kind, L]
    return search


@pytest.mark.parametrize("L", (4, 32))
@pytest.mark.parametrize("kind", ("random", "playout", "net", "net+cache"))
def test_brandubh_equals_one_descent_per_step(az, brandubh, kind, L):
    want, d1 = brandubh(kind, 1)
    got, d = brandubh(kind, L)
    _assert_same(want, got, f"Brandubh, {kind}, L = {L}")
    assert want["depth"].tolist() == [24] * 5 and d["simulations"] == d1["simulations"] == 5 * 24
    assert d1["steps"] == 24 and d1["host_reads"] == 0
    if kind == "random":
        assert d["steps"] == -(-24 // L) and d["host_reads"] == 0
    else:
        assert -(-24 // L) <= d["steps"] <= 24 and 1 <= d["host_reads"] <= 1 + int(np.ceil(np.log2(24)))


# ---- 3. step counts ------------------------------------------------------------------------------------------------------------------
def test_all_terminal_positions_take_two_steps(az, c4_net):
    """every legal move of every root ends the game: with the net and L >= visits a search is the root's row, then visits - 1
    terminal descents in ONE step"""
    visits = 24
    states = [_c4_at(az, p) for p in _C4_ALL_TERMINAL]
    n = len(states)
    for g in states:
        assert g.scores() is None
        for mv in np.flatnonzero(g.valid_moves()):
            h = g.copy(); h.play_move(int(mv))
            assert h.scores() is not None
    outs = []
    for L in (1, 32):
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=visits, seeds=list(range(n)), descents_per_step=L)
        mb.reset(states)
        s0 = mb.stats()
        mb.search(visits, net=c4_net)
        outs.append(_readout(mb))
        s1 = mb.stats()
        d = {k: s1[k] - s0[k] for k in s1}
        assert d["terminal_leaves"] == n * (visits - 1) and d["evaluator_leaves"] == n and d["simulations"] == n * visits
        if L > 1:
            assert d["steps"] == 2 and d["net_calls"] == 2 and d["host_reads"] == 2
    _assert_same(outs[0], outs[1], "all-terminal positions")


def test_whole_games_take_fewer_steps(az, c4_net):
    n, visits, max_moves = 9, 16, 42
    states = _c4_states(az, n, seed=3, max_len=6)
    res = []
    for L in (1, 8):
        cache = az.ShardedS3FIFOCache.for_engine(1 << 12, 7, 3)
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits * max_moves, seeds=[600 + i for i in range(n)],
                          descents_per_step=L)
        mb.reset(states)
        mb.play(visits, net=c4_net, cache=cache, temp=1.0, max_moves=max_moves)
        res.append((mb.move_logs(), mb.finished(), mb.final_scores(), mb.stats()))
    (logs1, fin1, fs1, st1), (logs8, fin8, fs8, st8) = res
    assert all(np.array_equal(a, b) for a, b in zip(logs1, logs8)) and len(logs1) == len(logs8) == n
    assert fin1.all() and np.array_equal(fin1, fin8) and np.array_equal(fs1, fs8)
    assert st1["simulations"] == st8["simulations"] and st1["terminal_leaves"] == st8["terminal_leaves"]
    assert st1["steps"] == visits * max_moves and st8["steps"] < st1["steps"]
    assert st1["host_reads"] == 0 and 0 < st8["host_reads"] <= max_moves * (1 + int(np.ceil(np.log2(visits))))


# ---- 4. what is out of scope raises by name, and the batch goes on ----------------------------------------------------------------------
def test_named_errors_leave_the_batch_usable(az, c4_reference):
    from alphazero import _capi
    from alphazero.mcts import _ENGINE_STREAM
    lib = _capi.lib
    with pytest.raises(RuntimeError, match=r"descents_per_step = 8 with leaves_per_step = 2"):
        az.MCTSBatch(az.Connect4GS, N, 1.25, max_simulations=VISITS, descents_per_step=8, leaves_per_step=2)
    seeds = [4000 + 13 * i for i in range(N)]
    mb = az.MCTSBatch(az.Connect4GS, N, 1.25, fpu_reduction=0.25, epsilon=0.25, max_simulations=VISITS + 8, seeds=seeds, descents_per_step=8)
    mb.reset(_positions(az))
    l0 = mb.stats()
    with pytest.raises(RuntimeError, match=r"search_to with descents_per_step = 8"):
        mb.search_to(12)
    with pytest.raises(RuntimeError, match=r"find_leaves with descents_per_step = 8"):
        mb.find_leaves()
    # the library's own checks, behind the Python ones
    pc, pt, nr = C.c_void_p(), C.c_void_p(), C.c_uint32()
    assert lib.azmi_search_find_leaves(mb._h, _ENGINE_STREAM, C.byref(pc), C.byref(pt), C.byref(nr)) == -1      # AZMI_ERR_INVALID
    assert "find_leaves with descents_per_step = 8" in lib.azmi_last_error().decode()
    tg = np.full(N, 12, np.uint32)
    assert lib.azmi_search_run_to(mb._h, 1, None, None, tg.ctypes.data, None, 0, 1.0, 0, 0, _ENGINE_STREAM) == -1
    assert "search_to with descents_per_step = 8" in lib.azmi_last_error().decode()
    assert lib.azmi_search_set_leaves_per_step(mb._h, 2) == -1
    assert "leaves_per_step = 2 with descents_per_step = 8" in lib.azmi_last_error().decode()
    assert mb.stats() == l0, "a refused call launches nothing"
    mb.search(VISITS, root_noise=True, evaluator="random")
    assert lib.azmi_search_set_descents_per_step(mb._h, 4) == -5                                                  # AZMI_ERR_STATE
    assert "the trees have been searched" in lib.azmi_last_error().decode()
    _assert_same(c4_reference("random")[0], _readout(mb), "after the refused calls")
