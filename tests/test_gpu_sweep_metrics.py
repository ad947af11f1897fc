"""-m gpu: `MCTSBatch.sweep_metrics()` / `alphazero.policy_divergences()`: a visit sweep scored against its anchor on the device.

Every expectation is the numpy restatement below of the formulas of policy_metrics.py and mcts_analysis.py:1196-1258, computed in
float64 from `checkpoints()` or from the input arrays.  top_k(x) is np.argsort(x, kind="stable")[-k:], the project's definition.

Tolerances: top-k columns, flags, count and valid are exact.  Float columns and means are within 1e-12 absolute: the sums have at
most 2 M terms, each bounded by p |ln 1e-10| ~ 23 p with sum p ~ 1 and each a few ulp off - below 1e-13 at M = 2662; the factor
ten covers the different summation order and the 1-ulp log / sqrt differences between libm and the device."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
POLICY = ("jsd", "tv", "hellinger", "top1", "top3", "top9")
COLUMNS = POLICY + ("reward", "regret", "pressure", "benefit", "entropy", "value_gap", "abs_err", "closer_than_anchor", "closer_than_raw")
EXACT = ("top1", "top3", "top9", "closer_than_anchor", "closer_than_raw")


@pytest.fixture(scope="module")
def az():
    import alphazero
    return alphazero


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def _top_k(x, k):
    return set(np.argsort(x, kind="stable")[-k:].tolist())


def _six(p, q):
    """p, q: float64 [M] -> the six policy figures"""
    m = 0.5 * (p + q)
    mp, mq = p > 0, q > 0
    jsd = 0.5 * np.sum(p[mp] * np.log(p[mp] / m[mp])) + 0.5 * np.sum(q[mq] * np.log(q[mq] / m[mq]))
    tv = 0.5 * np.sum(np.abs(p - q))
    hellinger = np.sqrt(0.5 * np.sum((np.sqrt(p) - np.sqrt(q)) ** 2))
    return (jsd, tv, hellinger) + tuple(len(_top_k(p, k) & _top_k(q, k)) / k for k in (1, 3, 9))


def _kl(p, q):
    m = p > 0
    return np.sum(p[m] * np.log(p[m] / (q[m] + 1e-10)))


def _entropy(p):
    m = p > 0
    return -np.sum(p[m] * np.log(p[m]))


def _expected(snap, ref, anchor, raw, outcomes):
    """snap, ref: checkpoints() of the swept and of the reference batch -> what sweep_metrics must return"""
    n, J, _ = snap["probs"].shape
    out = {k: np.full((n, J), np.nan) for k in COLUMNS}
    out["ceiling"] = np.full(n, np.nan)
    out["valid"] = np.zeros((n, J), bool)
    for i in range(n):
        if not ref["taken"][i, anchor]:
            continue
        p = ref["probs"][i, anchor].astype(np.float64)
        Q = ref["root_q_values"][i, anchor].astype(np.float64)
        v_a = np.float64(ref["root_values"][i, anchor, 0])
        have_raw = raw is not None and bool(ref["taken"][i, raw])
        if have_raw:
            r = ref["probs"][i, raw].astype(np.float64)
            v_r = np.float64(ref["root_values"][i, raw, 0])
            out["ceiling"][i] = _kl(p, r)
        for j in range(J):
            if not snap["taken"][i, j]:
                continue
            out["valid"][i, j] = True
            q = snap["probs"][i, j].astype(np.float64)
            v_j = np.float64(snap["root_values"][i, j, 0])
            for k, x in zip(POLICY, _six(p, q)):
                out[k][i, j] = x
            reward = np.sum(q * Q)
            out["reward"][i, j] = reward
            out["regret"][i, j] = np.sum(p * Q) - reward
            out["entropy"][i, j] = _entropy(q)
            out["value_gap"][i, j] = abs(v_j - v_a)
            if have_raw:
                out["pressure"][i, j] = _kl(q, r)
                out["benefit"][i, j] = reward - np.sum(r * Q)
            if outcomes is not None:
                o = np.float64(outcomes[i])
                out["abs_err"][i, j] = abs(v_j - o)
                out["closer_than_anchor"][i, j] = float(abs(v_j - o) < abs(v_a - o))
                if have_raw:
                    out["closer_than_raw"][i, j] = float(abs(v_j - o) < abs(v_r - o))
    out["mean"], out["count"] = {}, {}
    for k in COLUMNS:
        ok = ~np.isnan(out[k])
        out["count"][k] = ok.sum(axis=0)
        out["mean"][k] = np.array([out[k][ok[:, j], j].sum() / ok[:, j].sum() if ok[:, j].any() else np.nan for j in range(J)])
    return out


def _close(name, got, want, exact):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (name, got.shape, want.shape, got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: NaN where a figure belongs, or the other way round\n{got}\n{want}"
    ok = ~np.isnan(want)
    err = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
    print(f"{name}: max abs error {err:.3e}")
    assert err == 0.0 if exact else err <= TOL, f"{name}: off by {err:.3e}\n{got}\n{want}"


def _check(got, want):
    assert set(got) == set(COLUMNS) | {"ceiling", "valid", "mean", "count"}
    assert got["valid"].dtype == bool and np.array_equal(got["valid"], want["valid"])
    _close("ceiling", got["ceiling"], want["ceiling"], False)
    assert set(got["mean"]) == set(COLUMNS) and set(got["count"]) == set(COLUMNS)
    for k in COLUMNS:
        _close(k, got[k], want[k], k in EXACT)
        _close(f"mean[{k}]", got["mean"][k], want["mean"][k], False)
        assert np.array_equal(got["count"][k], want["count"][k]), (k, got["count"][k], want["count"][k])


# ---- policy_divergences on placed rows ---------------------------------------------------------------------------------------------
def _disjoint(M):
    """two rows of exactly representable probabilities on disjoint supports (M >= 2)"""
    p, q = np.zeros(M, np.float32), np.zeros(M, np.float32)
    if M >= 4:
        p[0], p[2], q[1], q[3] = 0.5, 0.5, 0.25, 0.75
    else:
        p[0], q[1] = 1.0, 1.0
    return p, q


def _placed_rows(M):
    rng = np.random.default_rng(1000 + M)

    def rand():
        x = rng.random(M).astype(np.float32) + np.float32(1e-3)
        return x / x.sum(dtype=np.float32)
    flat = np.full(M, np.float32(1.0) / np.float32(M), np.float32)
    a, b, c = rand(), rand(), rand()
    holes_p, holes_q = b.copy(), c.copy()
    holes_p[::2] = 0.0                          # zeros in p where q > 0
    holes_q[rng.random(M) < 0.5] = 0.0          # and the other way round (possibly every entry at M = 1)
    ties = np.round(rand() * 4).astype(np.float32) / 4      # few distinct values: ties inside a row that is not flat
    rows_p = [a, holes_p, b, flat, flat, ties]
    rows_q = [a, c, holes_q, flat, c, ties[::-1].copy()]
    if M >= 2:
        dp, dq = _disjoint(M)
        rows_p.append(dp)
        rows_q.append(dq)
    return np.stack(rows_p), np.stack(rows_q)


@pytest.mark.parametrize("M", [1, 2, 7, 8, 9, 10, 63, 64, 65, 686, 2662])
def test_policy_divergences_on_placed_rows(az, M):
    p, q = _placed_rows(M)
    got = az.policy_divergences(p, q)
    assert tuple(got) == POLICY
    want = np.array([_six(p[r].astype(np.float64), q[r].astype(np.float64)) for r in range(len(p))])
    for c, k in enumerate(POLICY):
        _close(f"M={M} {k}", got[k], want[:, c], k in EXACT)
    # identical rows: no distance, and top-k agreement min(M, k) / k - the divisor stays k
    assert got["jsd"][0] == 0.0 and got["tv"][0] == 0.0 and got["hellinger"][0] == 0.0
    for k in (1, 3, 9):
        assert got[f"top{k}"][0] == min(M, k) / k and got[f"top{k}"][3] == min(M, k) / k
    if M >= 2:      # disjoint supports
        assert abs(got["jsd"][-1] - np.log(2.0)) <= TOL and got["tv"][-1] == 1.0 and abs(got["hellinger"][-1] - 1.0) <= TOL
        assert got["top1"][-1] == 0.0


@pytest.mark.parametrize("rows", [0, 1, 5])
def test_policy_divergences_row_counts(az, rows):
    p, q = _placed_rows(10)
    got = az.policy_divergences(p[:rows], q[:rows])
    want = np.array([_six(p[r].astype(np.float64), q[r].astype(np.float64)) for r in range(rows)]).reshape(rows, 6)
    for c, k in enumerate(POLICY):
        _close(f"rows={rows} {k}", got[k], want[:, c], k in EXACT)


def test_the_tie_rule_is_the_stable_sort_s(az):
    # all-equal p: top_3 = the three highest indices; q puts its mass on the three lowest / on the three highest
    M = 12
    flat = np.full(M, 1.0 / M, np.float32)
    low, high = np.zeros(M, np.float32), np.zeros(M, np.float32)
    low[:3], high[-3:] = (0.5, 0.25, 0.25), (0.25, 0.25, 0.5)
    got = az.policy_divergences(np.stack([flat, flat]), np.stack([low, high]))
    assert got["top1"].tolist() == [0.0, 1.0] and got["top3"].tolist() == [0.0, 1.0]
    # top_9(flat) = indices 3 .. 11; top_9(low) = 0, 1, 2 and the six highest zeros 6 .. 11; top_9(high) = 9, 10, 11 and 3 .. 8
    assert got["top9"].tolist() == [6 / 9, 1.0]


# ---- Connect4: ties everywhere, M < 9, a tree that never takes the last checkpoint ---------------------------------------------------
_C4_POSITIONS = [(), (3, 3, 2), (1, 6, 3, 6, 4, 2, 2), (3,), (0, 1, 0, 1)]
_C4_OUTCOMES = np.array([1.0, -1.0, 0.0, 0.5, -0.25])


def _c4_at(az, moves):
    gs = az.Connect4GS()
    for mv in moves:
        gs.play_move(mv)
    return gs


@pytest.fixture(scope="module")
def c4_sweep(az):
    mb = az.MCTSBatch(az.Connect4GS, 5, 1.25, max_simulations=16, seeds=range(11, 16))
    mb.reset([_c4_at(az, m) for m in _C4_POSITIONS])
    mb.search_to([12, 12, 3, 12, 12], evaluator="random", checkpoints=(1, 4, 12))
    snap = mb.checkpoints()
    assert snap["taken"].tolist() == [[True] * 3, [True] * 3, [True, False, False], [True] * 3, [True] * 3]
    return mb, snap


def test_connect4_sweep_with_raw_and_outcomes(c4_sweep):
    mb, snap = c4_sweep
    got = mb.sweep_metrics(anchor=-1, raw=0, outcomes=_C4_OUTCOMES)
    _check(got, _expected(snap, snap, 2, 0, _C4_OUTCOMES))
    # tree 2 never took the anchor: its rows are invalid and NaN, and the means leave it out
    assert not got["valid"][2].any() and np.isnan(got["ceiling"][2])
    for k in COLUMNS:
        assert np.isnan(got[k][2]).all() and got["count"][k].tolist() == [4, 4, 4], k
    # the anchor row against itself; 7 moves: top9 of identical policies is 7 / 9
    ok = got["valid"][:, 2]
    assert (got["jsd"][ok, 2] == 0).all() and (got["regret"][ok, 2] == 0).all() and (got["top9"][ok, 2] == 7 / 9).all()
    assert (got["value_gap"][ok, 2] == 0).all() and (got["closer_than_anchor"][ok, 2] == 0).all()


def test_connect4_sweep_without_outcomes(c4_sweep):
    mb, snap = c4_sweep
    got = mb.sweep_metrics(anchor=-1, raw=0, outcomes=None)
    _check(got, _expected(snap, snap, 2, 0, None))
    for k in ("abs_err", "closer_than_anchor", "closer_than_raw"):
        assert np.isnan(got[k]).all() and got["count"][k].tolist() == [0, 0, 0] and np.isnan(got["mean"][k]).all()
    assert not np.isnan(got["pressure"][got["valid"]]).any()


def test_connect4_sweep_without_raw_and_on_an_earlier_anchor(c4_sweep):
    mb, snap = c4_sweep
    got = mb.sweep_metrics(outcomes=_C4_OUTCOMES)                        # raw=None
    _check(got, _expected(snap, snap, 2, None, _C4_OUTCOMES))
    for k in ("pressure", "benefit", "closer_than_raw"):
        assert np.isnan(got[k]).all()
    assert np.isnan(got["ceiling"]).all() and not np.isnan(got["abs_err"][got["valid"]]).any()
    # anchor 0 is taken by every tree: tree 2 is valid at checkpoint 0 alone, and is counted there alone
    got = mb.sweep_metrics(anchor=0, raw=-3, outcomes=_C4_OUTCOMES)
    _check(got, _expected(snap, snap, 0, 0, _C4_OUTCOMES))
    assert got["valid"][2].tolist() == [True, False, False] and got["count"]["tv"].tolist() == [5, 4, 4]


# ---- Brandubh: the strided wide-row path -------------------------------------------------------------------------------------------
def test_brandubh_sweep(az):
    states = [az.BrandubhGS() for _ in range(3)]
    for g, skip in zip(states[1:], (0, 3)):                                # two of them one legal move on
        g.play_move(int(np.flatnonzero(g.valid_moves())[skip]))
    mb = az.MCTSBatch(az.BrandubhGS, 3, 1.25, max_simulations=8, seeds=(5, 6, 7))
    mb.reset(states)
    mb.search_to(8, evaluator="random", checkpoints=(1, 8))
    snap = mb.checkpoints()
    assert snap["taken"].all() and snap["probs"].shape == (3, 2, 686)
    outcomes = np.array([1.0, 0.0, -1.0])
    _check(mb.sweep_metrics(anchor=-1, raw=0, outcomes=outcomes), _expected(snap, snap, 1, 0, outcomes))
    _check(mb.sweep_metrics(anchor=0), _expected(snap, snap, 0, None, None))


# ---- reference= --------------------------------------------------------------------------------------------------------------------
def test_a_noisy_sweep_is_scored_against_a_plain_reference_batch(az):
    states = [_c4_at(az, m) for m in _C4_POSITIONS[:4]]
    plain = az.MCTSBatch(az.Connect4GS, 4, 1.25, max_simulations=32, seeds=range(4))
    noisy = az.MCTSBatch(az.Connect4GS, 4, 1.25, epsilon=0.25, max_simulations=32, seeds=range(4))
    plain.reset(states)
    noisy.reset(states)
    plain.search_to(24, evaluator="random", checkpoints=(1, 6, 24))
    noisy.search_to(24, evaluator="random", root_noise=True, checkpoints=(1, 12))
    ps, ns = plain.checkpoints(), noisy.checkpoints()
    assert not np.array_equal(ps["probs"][:, 2], ns["probs"][:, 1])      # the noise moved the search
    outcomes = np.array([1.0, -1.0, 0.0, 1.0])
    got = noisy.sweep_metrics(anchor=-1, raw=0, reference=plain, outcomes=outcomes)
    assert got["jsd"].shape == (4, 2)
    _check(got, _expected(ns, ps, 2, 0, outcomes))
    assert (got["jsd"][:, 1] > 0).any()
    # a reference of another tree count or game raises by name; both objects still answer
    other_n = az.MCTSBatch(az.Connect4GS, 3, 1.25, max_simulations=8)
    other_n.reset(states[:3])
    other_n.search_to(4, evaluator="random", checkpoints=(1, 4))
    with pytest.raises(RuntimeError, match="the reference batch holds 3 trees, this batch 4"):
        noisy.sweep_metrics(reference=other_n)
    other_game = az.MCTSBatch(az.BrandubhGS, 4, 1.25, max_simulations=4)
    other_game.reset([az.BrandubhGS() for _ in range(4)])
    other_game.search_to(2, evaluator="random", checkpoints=(1,))
    with pytest.raises(RuntimeError, match="the reference batch holds another game"):
        noisy.sweep_metrics(reference=other_game)
    _check(noisy.sweep_metrics(anchor=-1, raw=0, reference=plain, outcomes=outcomes), _expected(ns, ps, 2, 0, outcomes))
    _check(plain.sweep_metrics(raw=0), _expected(ps, ps, 2, 0, None))
    _check(other_n.sweep_metrics(), _expected(other_n.checkpoints(), other_n.checkpoints(), 1, None, None))


def test_the_c_entry_point_refuses_a_mismatched_reference_and_stays_usable(az):
    from alphazero._capi import lib
    a = az.MCTSBatch(az.Connect4GS, 2, 1.25, max_simulations=8)
    b = az.MCTSBatch(az.Connect4GS, 3, 1.25, max_simulations=8)
    fresh = az.MCTSBatch(az.Connect4GS, 2, 1.25, max_simulations=8)
    for mb in (a, b, fresh):
        mb.reset([az.Connect4GS() for _ in range(len(mb))])
    a.search_to(4, evaluator="random", checkpoints=(1, 4))
    b.search_to(4, evaluator="random", checkpoints=(1, 4))
    call = lambda s, ref, anchor, raw: lib.azmi_search_sweep_metrics(s._h, None if ref is None else ref._h, anchor, raw,
                                                                     None, None, None, None, None, None, None)
    invalid, state = -1, -5                                              # AZMI_ERR_INVALID, AZMI_ERR_STATE (include/azmi.h)
    assert call(a, b, 1, -1) == invalid and b"tree count" in lib.azmi_last_error()
    assert call(a, None, 2, -1) == invalid and call(a, None, 1, 2) == invalid and call(a, None, 1, -2) == invalid
    assert call(fresh, None, 0, -1) == state and call(a, fresh, 0, -1) == state
    assert call(a, None, 1, 0) == 0
    snap = a.checkpoints()
    _check(a.sweep_metrics(raw=0), _expected(snap, snap, 1, 0, None))


# ---- bookkeeping -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64])
def test_two_launches_whatever_n_is_the_same_bits_twice_and_the_snapshots_untouched(az, n):
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=16, seeds=range(n))
    mb.reset([_c4_at(az, _C4_POSITIONS[i % len(_C4_POSITIONS)]) for i in range(n)])
    mb.search_to(10, evaluator="random", checkpoints=(1, 5, 10))
    before = mb.checkpoints()
    outcomes = np.linspace(-1.0, 1.0, n)
    l0 = mb.stats()["launches"]
    first = mb.sweep_metrics(anchor=-1, raw=0, outcomes=outcomes)
    assert mb.stats()["launches"] - l0 == 2
    second = mb.sweep_metrics(anchor=-1, raw=0, outcomes=outcomes)
    assert mb.stats()["launches"] - l0 == 4
    for k in COLUMNS:
        assert first[k].tobytes() == second[k].tobytes() and first["mean"][k].tobytes() == second["mean"][k].tobytes(), k
        assert np.array_equal(first["count"][k], second["count"][k])
    assert first["ceiling"].tobytes() == second["ceiling"].tobytes() and np.array_equal(first["valid"], second["valid"])
    after = mb.checkpoints()
    assert set(after) == set(before)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    _check(first, _expected(before, before, 2, 0, outcomes))


# ---- the README snippet ------------------------------------------------------------------------------------------------------------
def test_readme_sweep_metrics_snippet(az):
    lines = open(os.path.join(ROOT, "README.md")).read().splitlines()
    at = next(i for i, ln in enumerate(lines) if "sweep.sweep_metrics(" in ln and ln.startswith("    "))
    lo = hi = at
    while lines[lo - 1].startswith("    "):
        lo -= 1
    while lines[hi + 1].startswith("    "):
        hi += 1
    snippet = "\n".join(ln[4:] for ln in lines[lo: hi + 1])
    assert "search_to(" in snippet and "MCTSBatch(" in snippet
    scope = {"alphazero": az, "np": np}
    exec(snippet, scope)
    scores = scope["scores"]
    assert scope["jsd_by_visits"].shape == (5,) and scores["jsd"].shape == (16, 5) and scores["valid"].all()
    assert scope["jsd_by_visits"][-1] == 0.0 and (scores["count"]["closer_than_raw"] == 16).all()
