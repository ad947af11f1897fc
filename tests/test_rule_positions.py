"""CPU: every family of tests/rule_positions.py shows, on the oracle, the behaviour it is named for - a family that
silently tests nothing would make the device comparison of tests/test_gpu_rule_positions.py empty.  The oracle is pinned to
the reference (tests/test_oracle_pinned.py); where tafl_cases.py holds the reference's own answer for a position of the same
kind, the oracle is held to it here next to the family."""
import numpy as np
import pytest

import rule_positions as rp
import tafl_cases as tc

WIN = {0: [1, 0, 0], 1: [0, 1, 0], 2: [0, 0, 1]}


def c4_game(oracle, case):
    return oracle.Game.connect4_from_board(case[1], case[2], case[3])


def tafl_game(oracle, spec, case):
    return oracle.Game.tafl_from_board(spec.game_id, case[1], case[2], turn=case[3], max_turns=spec.max_turns)


def play_legal(game, moves):
    for m in moves or ():
        assert game.valid()[m] == 1, m
        game.play(m)
    return game


def score(game):
    s = game.scores()
    return None if s is None else s.tolist()


def pieces(game):
    return int(game.canonical()[:3].sum())


# ---- Connect4 ----------------------------------------------------------------------------------------------------------
def test_connect4_families(oracle):
    fam = rp.by_family(rp.c4_all() + rp.c4_illegal())
    assert len(fam["line"]) == 4 * 69 and len(fam["wrap"]) >= 2 * (5 + 3 + 3) and len(fam["full"]) >= 8
    assert len({c[1].tobytes() for c in fam["full"]}) == len(fam["full"])
    for case in fam["line"]:
        owner = int(case[0].split("-p")[1][0])
        assert score(c4_game(oracle, case)) == WIN[owner], case[0]
        assert rp.c4_has_four(case[1][owner]) and not rp.c4_has_four(case[1][1 - owner])
        if "embedded" in case[0]:                          # gravity, and stone counts of alternate play
            filled = case[1].sum(0)
            assert (np.diff(filled, axis=0) >= 0).all() and case[1][0].sum() - case[1][1].sum() == (1 if owner == 0 else 0), case[0]
    for case in fam["wrap"]:
        g = c4_game(oracle, case)
        assert score(g) is None and case[1].sum() == 4, case[0]
    assert {c[0].split("/")[1].split("-")[0] for c in fam["wrap"]} == {"row", "diag", "anti"}
    for case in fam["full"]:
        g = c4_game(oracle, case)
        assert score(g) == WIN[2] and not g.valid().any() and case[1].sum() == 42, case[0]
    for name, want in (("lastdraw", WIN[2]), ("lastwin", WIN[1])):
        assert len(fam[name]) >= 8
        for case in fam[name]:
            g = c4_game(oracle, case)
            assert score(g) is None and case[1].sum() == 41 and g.valid().sum() == 1, case[0]
            assert score(play_legal(g, case[4])) == want, case[0]
    for case in fam["oneopen"]:
        g = c4_game(oracle, case)
        assert score(g) is None and g.valid().sum() == 1, case[0]
        play_legal(g, case[4])
    for case in fam["illegal"]:
        g = c4_game(oracle, case)
        assert g.valid()[case[4][0]] == 0, case[0]
    for case in fam["nearwin"]:
        g = c4_game(oracle, case)
        assert score(g) is None and case[1][0].sum() - case[1][1].sum() == case[2], case[0]
        assert score(play_legal(g, case[4])) == WIN[case[2]], case[0]
    assert {c[2] for c in fam["nearwin"]} == {0, 1}
    print({k: len(v) for k, v in fam.items()})


# ---- Tafl family ---------------------------------------------------------------------------------------------------------
def _mover_moves(spec, game, h, w):
    return int(game.valid()[(h * spec.N + w) * 2 * spec.N:][: 2 * spec.N].sum())


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_slides(oracle, spec):
    fam = rp.by_family(rp.tafl_slides(spec))
    lone = {}
    for case in fam["slide0"]:
        kind, sq = case[0].split("/")[1].split("@")
        h, w = map(int, sq.split(","))
        lone[kind, h, w] = _mover_moves(spec, tafl_game(oracle, spec, case), h, w)
    band = {0, spec.T - 1, spec.T, spec.T + 1, spec.N - 1}
    assert {(h, w) for _, h, w in lone} == {(h, w) for h in range(spec.N) for w in range(spec.N) if h in band or w in band}
    assert max(lone.values()) == 2 * (spec.N - 1)
    blocked_on = set()
    for name in ("slide1", "slide2"):
        assert len(fam[name]) >= 400
        for case in fam[name]:
            head, *blockers = case[0].split("/")[1].split("|")
            kind, sq = head.split("@")
            h, w = map(int, sq.split(","))
            got = _mover_moves(spec, tafl_game(oracle, spec, case), h, w)
            assert got < lone[kind, h, w], case[0]        # every blocker stands on a ray of the mover and shortens it
            for s in blockers:
                bh, bw = map(int, s.split(","))
                blocked_on.add((min(h * spec.N + w, bh * spec.N + bw) < 64, bh * spec.N + bw))
    if spec.N == 11:       # blockers on squares 63 and 64, the mover in the same word and in the other one
        assert {(True, 63), (True, 64), (False, 64)} <= blocked_on
    print(spec.name, {k: len(v) for k, v in fam.items()})


@pytest.mark.parametrize("spec", [rp.BRANDUBH, rp.OPENTAFL], ids=lambda s: s.name)
def test_special_squares(oracle, spec):
    cases = rp.tafl_special_squares(spec)
    crossing = {"throne-empty": 0, "throne-king": 0}
    for case in cases:
        g = tafl_game(oracle, spec, case)
        assert score(g) is None, case[0]
        canon = g.canonical()
        for m in np.flatnonzero(g.valid()):
            fh, fw, th, tw = spec.unmv(m)
            king = canon[rp.K, fh, fw] == 1
            assert king or not spec.restricted(th, tw), case[0]          # no non-king piece lands on a corner or the throne
            between = fh == th == spec.T and min(fw, tw) < spec.T < max(fw, tw) or fw == tw == spec.T and min(fh, th) < spec.T < max(fh, th)
            for tag in crossing:
                if tag in case[0] and between and not king:
                    crossing[tag] += 1
        if "throne-empty" in case[0] and "far" not in case[0]:
            assert any(spec.T in (spec.unmv(m)[0], spec.unmv(m)[1]) and not spec.throne(*spec.unmv(m)[2:]) for m in np.flatnonzero(g.valid()))
        if case[4]:
            g = play_legal(g, case[4])
            if case[0].startswith("kingwin"):
                assert score(g) == WIN[rp.DEF], case[0]
            else:
                assert score(g) is None and g.canonical()[rp.K, spec.T, spec.T] == 1, case[0]
    assert crossing["throne-empty"] > 0 and crossing["throne-king"] == 0
    if spec is rp.OPENTAFL:      # the reference's own answers for positions of these kinds
        for name in ("NonKingPassesThroughThroneButCannotLand", "KingMayLandOnEmptyThrone", "NonKingCannotLandOnCorner", "KingEscapesToCorner"):
            _reference_case(oracle, name)


def _reference_case(oracle, name):
    case = next(c for c in tc.OPENTAFL_CASES if c[0] == name)
    tc.check_case(oracle.Game.tafl_from_board(oracle.GAME_OPENTAFL, tc.board(case[1]), case[2], turn=case[3]), case)


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_captures_and_kings(oracle, spec):
    fam = rp.by_family(rp.tafl_captures(spec) + rp.tafl_kings(spec))
    want_families = {"capture0", "capture1", "capture2", "capture3", "kingwin"} | ({"kingcap0", "kingcap1"} if spec.strong_king else {"kingcap1"})
    assert want_families <= set(fam)
    for name, cases in fam.items():
        for case in cases:
            g = tafl_game(oracle, spec, case)
            assert score(g) is None, case[0]
            before = pieces(g)
            g = play_legal(g, case[4])
            taken = before - pieces(g)
            if name.startswith("capture"):
                assert taken == int(name[-1]), (case[0], taken)         # (taking a side's last piece ends the game: no score check)
            elif name.startswith("kingcap"):
                assert taken == int(name[-1]) and g.canonical()[rp.K].sum() == 1 - int(name[-1]), (case[0], taken)
                assert score(g) == (WIN[rp.ATK] if name[-1] == "1" else None), case[0]
            else:
                assert name == "kingwin" and score(g) == WIN[rp.DEF], case[0]
    if spec.N == 11:             # victims on squares 63 and 64
        assert any("@5,8" in c[0] for c in fam["capture1"]) and any("@5,9" in c[0] for c in fam["capture1"])
    if spec.special:
        for tag in ("corner", "throne-empty", "throne-king-A"):
            assert any(tag in c[0] for c in fam["capture1"]), tag
        assert any("throne-king-D" in c[0] for c in fam["capture0"])
    if spec is rp.OPENTAFL:
        for name in ("CaptureBetweenTwoEnemies", "CaptureAgainstCorner", "CaptureAgainstEmptyThrone", "ThroneNotHostileToDefenderWithKing",
                     "EdgeIsNotHostile", "CaptureInTwoDirectionsAtOnce", "ThroneHostileToAttackersWhenEmpty", "ThroneHostileToAttackersWithKing",
                     "KingCapturedOnFourSides", "KingNotCapturedOnEdge", "KingCapturedNextToThrone"):
            _reference_case(oracle, name)
    print(spec.name, {k: len(v) for k, v in fam.items()})


def test_encirclement(oracle):
    spec = rp.OPENTAFL
    fam = rp.by_family(rp.tafl_encirclement(spec))
    assert len(fam["encircled"]) >= 8 and len(fam["gap"]) >= 30
    for case in fam["encircled"]:
        assert score(tafl_game(oracle, spec, case)) == WIN[rp.ATK], case[0]
    closing = 0
    for case in fam["gap"]:
        g = tafl_game(oracle, spec, case)
        assert score(g) is None, case[0]
        if case[4]:
            assert score(play_legal(g, case[4])) == WIN[rp.ATK], case[0]      # the spare attacker closes the ring
            closing += 1
    assert closing >= 10 and any("outsider" in c[0] for c in fam["gap"]) and any("rim" in c[0] for c in fam["encircled"])
    _reference_case(oracle, "EncirclementIsAttackerWin")
    _reference_case(oracle, "NotEncircledGameContinues")


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_endings(oracle, spec):
    for case in rp.tafl_boxed(spec):
        g = tafl_game(oracle, spec, case)
        assert not g.valid().any() and score(g) == WIN[1 - case[2]], case[0]
        own = g.canonical()[[rp.A] if case[2] == rp.ATK else [rp.K, rp.D]].sum()
        assert own >= 1, case[0]
    assert {c[2] for c in rp.tafl_boxed(spec)} == {rp.ATK, rp.DEF}
    for case in rp.tafl_forced(spec):
        g = tafl_game(oracle, spec, case)
        assert score(g) is None and g.valid().sum() == 1, case[0]
        assert score(play_legal(g, case[4])) is None
    for case in rp.tafl_last_turn(spec):
        g = tafl_game(oracle, spec, case)
        assert score(g) is None and g.turn() == spec.max_turns - 1, case[0]
        before = pieces(g)
        g = play_legal(g, case[4])
        assert score(g) == (WIN[rp.DEF] if case[0].startswith("lastturn-win") else WIN[2]) and pieces(g) == before, case[0]
    for case in rp.tafl_repetition(spec):
        g = play_legal(tafl_game(oracle, spec, case), case[4])
        if case[0].startswith("repetition-short"):
            assert score(g) is None, case[0]
        else:
            assert score(g) == WIN[g.player()] and g.turn() < spec.max_turns, case[0]
    for case in rp.tafl_illegal(spec):
        g = tafl_game(oracle, spec, case)
        assert score(g) is None and g.valid()[case[4][0]] == 0, case[0]
    if spec is rp.OPENTAFL:
        _reference_case(oracle, "NoLegalMovesLoses")
        _reference_case(oracle, "MaxTurnsIsADraw")
        _reference_case(oracle, "RookMovementSlidesAndIsBlocked")


def dense_follow_up(oracle, spec, case, rng):
    """-> (oracle game at the position, legal follow-up move or None when the game is over or nothing moves)"""
    g = tafl_game(oracle, spec, case)
    legal = np.flatnonzero(g.valid())
    if g.scores() is not None or len(legal) == 0:
        return g, None
    return g, int(rng.choice(legal))


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_dense_family_shares(oracle, spec):
    cases = rp.tafl_dense(spec)
    rng = np.random.default_rng(1)
    terminal = captures = moved = 0
    occupied = set()
    for case in cases:
        occupied.add(round(8 * case[1].sum() / spec.N ** 2))
        g, m = dense_follow_up(oracle, spec, case, rng)
        terminal += g.scores() is not None
        if m is not None:
            before = pieces(g)
            g.play(m)
            moved += 1
            captures += pieces(g) < before
    print(f"{spec.name}: {len(cases)} dense positions, {terminal / len(cases):.1%} terminal before the move, "
          f"{captures / moved:.1%} of {moved} follow-up moves capture")
    assert occupied >= {1, 2, 3, 4, 5, 6}
    assert {c[2] for c in cases} == {0, 1}
    assert captures >= 0.05 * moved and terminal >= 0.01 * len(cases)
