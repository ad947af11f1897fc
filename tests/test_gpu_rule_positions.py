"""-m gpu: the device rules (csrc/dev_games.h) at the placed positions of tests/rule_positions.py, bit for bit against the
oracle: one batched game_replay(..., init=...) per game and family, before and after the follow-up move; then the positions
one move from a win, the draw, a stalemate or encirclement as ROOTS of MCTSBatch and of the stand-alone MCTS object, whose
terminal-leaf paths the parity tests from the opening do not reach.  tests/test_rule_positions.py (CPU) shows that every
family has the behaviour it is named for.

The wide-game engine (PlayManager) has no start-position entry - it starts every game from the game's initial position - so
its child generation is reached here only through the rules it shares with these kernels."""
import numpy as np
import pytest

import rule_positions as rp
from test_gpu_search_batch import _assert_tree_equals, _drive_alone, _readout, _readout_one
from test_rule_positions import c4_game, dense_follow_up, tafl_game

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def az():
    import alphazero
    return alphazero


# ---- replay ----------------------------------------------------------------------------------------------------------------
def _rows(cases, image, make, illegal=False):
    """-> (images, moves [n, L], oracle games, names, want_status): per case one row at the position and, with a follow-up, one
    behind it.  `illegal`: the LAST follow-up move is refused: the row keeps the position in front of it, status -1."""
    images, moves, games, names, status = [], [], [], [], []
    for case in cases:
        name, board, player, turn, follow = case
        img = image(board, player, turn)
        images.append(img); moves.append([]); games.append(make(case)); names.append(name); status.append(0)
        if follow:
            g = make(case)
            for m in follow[:-1] if illegal else follow:
                g.play(m)
            images.append(img); moves.append(list(follow)); games.append(g); names.append(name + " + " + str(follow)); status.append(-1 if illegal else 0)
    width = max(1, max(len(m) for m in moves))
    mv = -np.ones((len(moves), width), np.int32)
    for i, m in enumerate(moves):
        mv[i, :len(m)] = m
    return images, mv, games, names, np.array(status, np.int32)


def _compare(out, games, names, want_status, exact_keys):
    assert np.array_equal(out["status"], want_status), [names[i] for i in np.flatnonzero(out["status"] != want_status)][:5]
    seen = {}
    for r, (g, name) in enumerate(zip(games, names)):
        assert np.array_equal(out["valid"][r], g.valid()), name
        sc = g.scores()
        assert np.array_equal(out["scores"][r], np.full_like(out["scores"][r], -1) if sc is None else sc), (name, out["scores"][r], sc)
        canon = g.canonical()
        assert np.array_equal(out["canonical"][r], canon), name
        assert out["player"][r] == g.player() and out["turn"][r] == g.turn(), name
        if exact_keys:
            assert int(out["key"][r]) == g.key(), name
        else:                # equal device keys exactly when canonical tensor and player are equal
            ident = (canon.tobytes(), g.player())
            assert seen.setdefault(("k", int(out["key"][r])), ident) == ident, name
            assert seen.setdefault(("i", ident), int(out["key"][r])) == int(out["key"][r]), name


def _c4_replay(az, oracle, cases, illegal=False):
    images, mv, games, names, status = _rows(cases, lambda b, p, t: az.Connect4GS(b, p, t)._init, lambda c: c4_game(oracle, c), illegal)
    _compare(az.game_replay(az.Connect4GS, mv, init=images), games, names, status, exact_keys=True)
    return len(names)


def _tafl_replay(az, oracle, spec, cases, illegal=False):
    Game = getattr(az, spec.name)
    images, mv, games, names, status = _rows(cases, Game._image, lambda c: tafl_game(oracle, spec, c), illegal)
    _compare(az.game_replay(Game, mv, init=images), games, names, status, exact_keys=False)
    return len(names)


def test_connect4_placed_positions(az, oracle):
    fam = rp.by_family(rp.c4_all())
    assert set(fam) == {"line", "wrap", "full", "lastdraw", "lastwin", "oneopen", "nearwin"}
    for name, cases in fam.items():
        assert _c4_replay(az, oracle, cases) >= len(cases), name


def test_connect4_full_column_is_refused_and_the_other_rows_stand(az, oracle):
    legal = rp.c4_one_open()[:20]
    bad = rp.c4_illegal()
    images, mv, games, names, status = _rows(bad, lambda b, p, t: az.Connect4GS(b, p, t)._init, lambda c: c4_game(oracle, c), illegal=True)
    i2, mv2, g2, n2, s2 = _rows(legal, lambda b, p, t: az.Connect4GS(b, p, t)._init, lambda c: c4_game(oracle, c))
    order = np.random.default_rng(3).permutation(len(names) + len(n2))           # refused and legal rows interleaved
    every = [(images + i2)[j] for j in order]
    out = az.game_replay(az.Connect4GS, np.concatenate([mv, mv2])[order], init=every)
    assert (out["status"] == -1).sum() == len(bad)
    _compare(out, [(games + g2)[j] for j in order], [(names + n2)[j] for j in order], np.concatenate([status, s2])[order], exact_keys=True)


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_tafl_slides(az, oracle, spec):
    for name, cases in rp.by_family(rp.tafl_slides(spec)).items():
        assert _tafl_replay(az, oracle, spec, cases) == len(cases), name


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_tafl_captures_kings_and_endings(az, oracle, spec):
    cases = rp.tafl_captures(spec) + rp.tafl_kings(spec) + rp.tafl_boxed(spec) + rp.tafl_forced(spec) + rp.tafl_last_turn(spec)
    cases += rp.tafl_repetition(spec)
    if spec.special:
        cases += rp.tafl_special_squares(spec)
    if spec.strong_king:
        cases += rp.tafl_encirclement(spec)
    fam = rp.by_family(cases)
    assert {"capture0", "capture1", "capture2", "capture3", "kingcap1", "kingwin", "boxed", "forced", "lastturn", "repetition"} <= set(fam)
    for name, group in fam.items():
        assert _tafl_replay(az, oracle, spec, group) >= len(group), name


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_tafl_illegal_moves_are_refused_and_the_other_rows_stand(az, oracle, spec):
    Game = getattr(az, spec.name)
    make = lambda c: tafl_game(oracle, spec, c)
    bad = rp.tafl_illegal(spec)
    legal = rp.tafl_forced(spec) + rp.tafl_last_turn(spec)
    images, mv, games, names, status = _rows(bad, Game._image, make, illegal=True)
    i2, mv2, g2, n2, s2 = _rows(legal, Game._image, make)
    order = np.random.default_rng(4).permutation(len(names) + len(n2))
    out = az.game_replay(Game, np.concatenate([mv, mv2])[order], init=[(images + i2)[j] for j in order])
    assert (out["status"] == -1).sum() == len(bad)
    _compare(out, [(games + g2)[j] for j in order], [(names + n2)[j] for j in order], np.concatenate([status, s2])[order], exact_keys=False)


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_tafl_dense_boards(az, oracle, spec):
    """the seeded dense family, each position followed by one legal move drawn from the oracle's valid() (the same draw as in
    test_rule_positions.test_dense_family_shares, which holds the capture and terminal shares above their floors)"""
    rng = np.random.default_rng(1)
    cases = []
    for case in rp.tafl_dense(spec):
        _, m = dense_follow_up(oracle, spec, case, rng)
        cases.append(case[:4] + (None if m is None else [m],))
    assert _tafl_replay(az, oracle, spec, cases) > len(cases)


# ---- the search consumers ------------------------------------------------------------------------------------------------------
def _take(cases, family, k, with_moves=False):
    got = [c for c in cases if rp.family(c[0]) == family and (c[4] or not with_moves)]
    step = max(1, len(got) // k)
    return got[::step][:k]


def c4_roots():
    cases = rp.c4_all()
    return _take(cases, "nearwin", 12) + _take(cases, "lastwin", 4) + _take(cases, "lastdraw", 6) + _take(cases, "oneopen", 10)


def tafl_roots(oracle, spec):
    """one move from a win for either side, from the draw, a forced move, next to encirclement, dense boards: 32 running roots"""
    placed = rp.tafl_kings(spec) + rp.tafl_forced(spec) + rp.tafl_last_turn(spec) + rp.tafl_captures(spec)
    roots = _take(placed, "kingcap1", 5) + _take(placed, "kingwin", 5) + _take(placed, "lastturn", 3) + _take(placed, "lastturn-win", 1)
    roots += _take(placed, "forced", 4) + _take(placed, "capture2", 2)
    if spec.strong_king:
        roots += _take(rp.tafl_encirclement(spec), "gap", 4, with_moves=True)
    dense = [c for c in rp.tafl_dense(spec) if int(c[0].split("/")[1][0]) >= 3 and tafl_game(oracle, spec, c).scores() is None
             and tafl_game(oracle, spec, c).valid().any()]
    roots += dense[: 32 - len(roots)]
    assert len(roots) == 32 and all(tafl_game(oracle, spec, c).scores() is None for c in roots)
    return roots


def _search_roots(az, oracle, Game, states, ogames, what, visits=64):
    n, M = len(states), Game.NUM_MOVES()
    seeds = [700 + 13 * i for i in range(n)]
    kw = dict(fpu_reduction=0.25)
    mb = az.MCTSBatch(Game, n, 1.25, max_simulations=visits, seeds=seeds, **kw)
    mb.reset(states)
    mb.search(visits, evaluator="random")
    out = _readout(mb)
    assert out["depth"].tolist() == [visits] * n
    terminal_leaves = mb.stats()["terminal_leaves"]
    for i in range(n):
        o = oracle.Mcts(1.25, 2, M, seed=seeds[i], **kw)
        o.search_dumb(ogames[i], visits)
        assert np.array_equal(out["counts"][i], o.counts()), f"{what}: root {i}: counts"
        assert np.array_equal(out["rv"][i], o.root_value()), f"{what}: root {i}: root value"
        assert np.array_equal(out["q"][i], o.root_q()), f"{what}: root {i}: root q"
        m = az.MCTS(1.25, 2, M, game=Game, seed=seeds[i], max_simulations=visits, **kw)
        _drive_alone(az, m, states[i], visits)
        _assert_tree_equals(out, i, _readout_one(m), what)
    return terminal_leaves


def test_connect4_placed_roots_in_the_search(az, oracle):
    roots = c4_roots()
    assert len(roots) == 32
    states = [az.Connect4GS(b, p, t) for _, b, p, t, _ in roots]
    terminal = _search_roots(az, oracle, az.Connect4GS, states, [c4_game(oracle, c) for c in roots], "Connect4GS")
    # the 10 lastwin / lastdraw roots have one legal move and it ends the game: every visit behind the root's own expansion
    # (and, at most, one for the child's) ends on a terminal leaf
    assert terminal >= 10 * 62


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_tafl_placed_roots_in_the_search(az, oracle, spec):
    Game = getattr(az, spec.name)
    roots = tafl_roots(oracle, spec)
    states = [Game.from_board(b, p, t) for _, b, p, t, _ in roots]
    terminal = _search_roots(az, oracle, Game, states, [tafl_game(oracle, spec, c) for c in roots], spec.name)
    assert terminal > 0
