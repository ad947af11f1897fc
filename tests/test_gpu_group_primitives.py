"""GPU: the lane-group primitives of the descent on their own (azmi_debug_group_select: one wavefront = eight 8-lane groups per
row): the in-order sum of the visited children's priors as EVERY lane of the group holds it, select_child's winner, and the
group-wide AND / OR of a lane predicate.  Parity games rarely produce the edge inputs (ties across the two quads of a group,
NaN, infinities, signed zeros, denormals), and the way these primitives can go wrong is one group's answer leaking into its
neighbour or one half of a group missing a broadcast: the eight groups of a row always differ from each other.

The reference is Node::best_child / Node::uct (mcts.cc:123-149) restated in numpy float32, operation by operation: seen_policy
starts at 0.0f and takes the visited children's priors in child order, np.sqrt on float32 is correctly rounded like the
library's, the scan replaces the incumbent on a strict `>` only (so a NaN at index 0 stays, a NaN elsewhere never wins).
Equality is bitwise.  k = 0 has no reference (children.at(0) throws; the library's callers raise before they select): the sum
is +0.0 and the winner is the library's 'nobody' value 0xFFFF."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
NOBODY = 0xFFFF
INF, NAN = F(np.inf), F(np.nan)


def ref_group(k, n, q, p, v_parent, n_parent, fpu, cpuct):
    """(seen_policy, winner) of one group, float32 in reference order"""
    with np.errstate(all="ignore"):
        seen = F(0.0)
        for i in range(k):
            if n[i] > 0:
                seen = F(seen + p[i])
        if k == 0:
            return seen, NOBODY
        fpu_value = F(v_parent - F(fpu * np.sqrt(seen)))
        sqrt_n = np.sqrt(F(np.uint32(n_parent)))

        def uct(i):
            return F((fpu_value if n[i] == 0 else q[i]) + F(F(F(cpuct * p[i]) * sqrt_n) / F(np.uint32(n[i] + 1))))
        best, best_u = 0, uct(0)
        for i in range(1, k):
            u = uct(i)
            if u > best_u:
                best, best_u = i, u
        return seen, best


def group(k, n, q, p, v_parent=0.3, n_parent=10, fpu=0.25, cpuct=2.0):
    n = np.asarray(list(n) + [0] * (8 - len(n)), np.uint32)
    q = np.asarray(list(q) + [0] * (8 - len(q)), F)
    p = np.asarray(list(p) + [0] * (8 - len(p)), F)
    return dict(k=k, n=n, q=q, p=p, v_parent=F(v_parent), n_parent=int(n_parent), fpu=F(fpu), cpuct=F(cpuct))


def random_group(rng, k=None):
    """children with quantised q and p (ties are common), some unvisited, now and then a special value"""
    k = int(rng.integers(1, 8)) if k is None else k
    n = rng.integers(0, 4, 8) * rng.integers(0, 2, 8) * rng.integers(1, 50, 8)
    q = (rng.integers(-8, 9, 8) / 8.0).astype(F)
    p = (rng.integers(0, 9, 8) / 16.0).astype(F)
    if rng.random() < 0.5:
        q = rng.uniform(-1, 1, 8).astype(F)
        p = rng.dirichlet(np.ones(8)).astype(F)
    for arr in (q, p):
        if rng.random() < 0.15:
            arr[rng.integers(0, 8)] = rng.choice([NAN, INF, -INF, F(-0.0), F(1e-41)])
    # (lanes past k carry data too: whatever sits there must not reach the result)
    return group(k, n, q, p, v_parent=rng.uniform(-1, 1), n_parent=int(rng.choice([0, 1, 2, 7, 800, int(n.sum()) + 1])),
                 fpu=rng.choice([0.0, 0.25, 1.0]), cpuct=rng.choice([1.25, 2.0, 4.0]))


def hand_rows(rng):
    """the named edge cases, eight different groups per row"""
    u0 = [0] * 7
    tie = lambda a, b: [0.3 if i in (a, b) else 0.1 for i in range(7)]      # unvisited children: equal priors are equal scores
    rows = []
    # k = 0, 1, 4, 7 side by side (twice, in two orders, among different data)
    rows.append([random_group(rng, k) for k in (0, 1, 4, 7, 7, 4, 1, 0)])
    rows.append([random_group(rng, k) for k in (7, 0, 4, 1, 0, 7, 1, 4)])
    # exact ties: inside a quad, across the quads, at the quads' border; visited children with equal q as well
    rows.append([group(7, u0, u0, tie(2, 5), n_parent=9), group(7, u0, u0, tie(1, 6), n_parent=9), group(7, u0, u0, tie(3, 4), n_parent=9),
                 group(7, u0, u0, tie(0, 6), n_parent=16), group(7, u0, u0, tie(5, 6), n_parent=16), group(7, u0, u0, tie(2, 3), n_parent=4),
                 group(7, [3] * 7, [0.5, 0.25, 0.75, 0.5, 0.5, 0.75, 0.25], [0.125] * 7, n_parent=22),
                 group(7, [1] * 7, [0.25] * 7, [0.125] * 7, n_parent=8)])
    # NaN at lane 0 only, at lane 3 only, everywhere (through q, through the parent's value); infinities of both signs
    one = [1] * 7
    qs = [0.1, 0.2, 0.3, 0.4, 0.3, 0.2, 0.1]
    ps = [0.1, 0.2, 0.1, 0.2, 0.1, 0.2, 0.1]
    rows.append([group(7, one, [NAN] + qs[1:], ps), group(7, one, qs[:3] + [NAN] + qs[4:], ps), group(7, one, [NAN] * 7, ps),
                 group(7, u0, qs, ps, v_parent=NAN), group(7, one, qs[:4] + [INF] + qs[5:], ps), group(7, one, [-INF] * 6 + [0.0], ps),
                 group(7, one, [INF, 0.1, 0.2, INF, 0.3, INF, 0.0], ps), group(7, one, [NAN, INF, 0.2, 0.1, 0.3, INF, 0.0], ps)])
    # -0.0 priors, all children unvisited, an infinite prior under n_parent = 0 (inf * 0), a denormal sum, n_parent = 0, 1, 2^24 + 1
    den = [1e-40, 2e-40, 3e-41, 1e-42, 5e-41, 7e-42, 1e-45]
    rows.append([group(7, one, qs, [-0.0] * 7), group(7, u0, u0, ps, n_parent=1), group(7, one, qs, [INF] + ps[1:], n_parent=0),
                 group(7, one, qs, den, fpu=1.0), group(7, [0, 1, 0, 1, 0, 1, 0], qs, ps, n_parent=0),
                 group(7, [0, 2, 0, 0, 5, 0, 0], qs, ps, n_parent=1), group(7, [4, 0, 9, 1, 0, 0, 2], qs, ps, n_parent=(1 << 24) + 1),
                 group(3, u0, u0, [-0.0, 0.0, -0.0], v_parent=-0.0, fpu=0.0)])
    return rows


def build_case():
    rng = np.random.default_rng(20261)
    rows = hand_rows(rng)
    preds = [int(x) for x in rng.integers(0, 1 << 63, len(rows), dtype=np.uint64)]
    # the lane predicate: all ones; one zero at lane j (j = 0 .. 7) of a single group; zeros only in lane 7 of every group (the lane
    # that never holds a child); no bit set; random words
    full = (1 << 64) - 1
    special = [full] + [full ^ (1 << (8 * ((3 * j + 1) % 8) + j)) for j in range(8)] + [full ^ 0x8080808080808080, 0, 1 << 63, 0xFF << 24]
    while len(rows) < 320:
        rows.append([random_group(rng) for _ in range(8)])
        preds.append(special[len(rows) % len(special)] if len(rows) % 2 else int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2)))
    return rows, np.asarray(preds, np.uint64)


@pytest.fixture(scope="module")
def run():
    import __graft_entry__ as g
    g.build()
    from alphazero import _capi
    rows, pred = build_case()
    R = len(rows)
    flat = [gr for row in rows for gr in row]
    k8 = np.asarray([gr["k"] for gr in flat], np.uint32)
    n64 = np.concatenate([gr["n"] for gr in flat]).astype(np.uint32)
    q64 = np.concatenate([gr["q"] for gr in flat]).astype(F)
    p64 = np.concatenate([gr["p"] for gr in flat]).astype(F)
    vp8 = np.asarray([gr["v_parent"] for gr in flat], F)
    np8 = np.asarray([gr["n_parent"] for gr in flat], np.uint32)
    fpu8 = np.asarray([gr["fpu"] for gr in flat], F)
    cp8 = np.asarray([gr["cpuct"] for gr in flat], F)
    s64, b64, a64 = np.full(R * 64, -1.0, F), np.full(R * 64, 12345, np.uint32), np.full(R * 64, 12345, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.check(_capi.lib.azmi_debug_group_select(0, R, ptr(k8), ptr(n64), ptr(q64), ptr(p64), ptr(vp8), ptr(np8), ptr(fpu8), ptr(cp8), ptr(pred),
                                                   ptr(s64), ptr(b64), ptr(a64)))
    ref = [ref_group(gr["k"], gr["n"], gr["q"], gr["p"], gr["v_parent"], gr["n_parent"], gr["fpu"], gr["cpuct"]) for gr in flat]
    return dict(rows=rows, pred=pred, sum=s64.reshape(-1, 8), best=b64.reshape(-1, 8), flags=a64.reshape(-1, 8), ref=ref)


def test_rows_hold_eight_different_groups(run):
    for row in run["rows"]:
        keys = {(gr["k"], gr["n"].tobytes(), gr["q"].tobytes(), gr["p"].tobytes(), gr["v_parent"].tobytes(), gr["n_parent"]) for gr in row}
        assert len(keys) == 8


def test_in_order_sum_reaches_every_lane(run):
    want = np.asarray([s for s, _ in run["ref"]], F)
    got = run["sum"]
    for lane in range(8):      # (lanes 0-3 and 4-7 get the sum by different moves)
        bad = np.flatnonzero(got[:, lane].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"lane {lane}: group {bad[0]} (row {bad[0] // 8}) holds {got[bad[0], lane]!r}, the in-order sum is {want[bad[0]]!r}"


def test_winner_is_the_strict_scan_winner_in_every_lane(run):
    want = np.asarray([b for _, b in run["ref"]], np.uint32)
    got = run["best"]
    for lane in range(8):
        bad = np.flatnonzero(got[:, lane] != want)
        assert bad.size == 0, f"lane {lane}: group {bad[0]} (row {bad[0] // 8}) chose {got[bad[0], lane]}, the scan chooses {want[bad[0]]}"
    # the named ties of the third hand-made row
    assert want[16:22].tolist() == [2, 1, 3, 0, 5, 2]
    # NaN at lane 0 stays, NaN at lane 3 never wins, all NaN is child 0
    assert want[24] == 0 and want[25] != 3 and want[26] == 0 and want[27] == 0


def test_group_and_or_of_a_lane_predicate(run):
    pred = run["pred"]
    bytes_ = (pred[:, None] >> (np.arange(8, dtype=np.uint64) * np.uint64(8))[None, :]) & np.uint64(0xFF)
    want = ((bytes_ == 0xFF).astype(np.uint32) | ((bytes_ != 0).astype(np.uint32) << 1)).reshape(-1)
    got = run["flags"]
    for lane in range(8):
        bad = np.flatnonzero(got[:, lane] != want)
        assert bad.size == 0, f"lane {lane}: group {bad[0]} (row {bad[0] // 8}, predicate {int(pred[bad[0] // 8]):#018x}) says {got[bad[0], lane]}, expected {want[bad[0]]}"
    assert (want == 3).any() and (want == 2).any() and (want == 0).any()
