"""GPU: expand_node (Node::add_children, mcts.cc:93-101) on its own - azmi_debug_group_expand: one wavefront per row, its eight
8-lane groups expand eight Connect4 positions each, one after the other, into their own tree arenas - once with the move word
packed by a loop over the legal moves (k_sim, k_round) and once packed by the group's lanes (the pipeline's tree kernel); the
shuffle behind it is the same code.  The eight groups of a
wavefront hold positions of different k (both parities side by side: the shuffle's steps are shared by the groups of a
wavefront), and the positions cover k = 0 .. 7, full and empty columns at both board edges, the position one move before a
full board, and several RNG states per k.

The reference is a pure-Python restatement of what the oracle plays: the legal moves in ascending order, libstdc++'s
std::shuffle (stl_algo.h:3729-3792, the pair-swap form: one draw below 2 when k is even, then pairs (x / b1, x % b1) from one
draw below swap_range * b1), uniform_int_distribution on a 32-bit generator (Lemire's method with its rejection loop,
uniform_int_dist.h:246-270) and pcg32.  Compared bit for bit in every lane of every group: the lane's child move, c0, k, the
RNG state afterwards, and the whole arena (the child records, the parents' meta words, and every byte expand_node must not
touch).

The rejection branch of Lemire's method is taken with probability 2^-30 or less per draw here, so states that take it are
CONSTRUCTED, not searched for: a 32-bit output u with (u * range) mod 2^32 below the threshold (u = 0, and u = ceil(t 2^32 /
range) for the t that land below it), a pcg32 state with that output (the output permutation inverted), and the generator
stepped backwards to the draw of the expansion that is to be rejected - one state for every pair draw of every k >= 3, i.e.
for each of the ranges 6, 20, 42, 12, 30 (56 needs eight children; range 2 has threshold 0 and never rejects).  The restatement
counts the rejections and the test asserts that each constructed state is rejected where it was meant to be."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MULT, INC = 6364136223846793005, 1442695040888963407
MULT_INV = pow(MULT, -1, 1 << 64)
H, W = 6, 7
REPS, CAP = 8, 80
NODE = np.dtype([("n", "<u4"), ("q", "<f4"), ("pr", "<f4"), ("d", "<f4"), ("v", "<f4"), ("pad", "<u4"), ("meta", "<u8")])


class Pcg32:
    def __init__(self, state):
        self.state = state & M64

    def next(self):
        old = self.state
        self.state = (old * MULT + INC) & M64
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF


def lemire_below(g, rng_range, log):
    product = g.next() * rng_range
    low = product & 0xFFFFFFFF
    if low < rng_range:
        threshold = ((1 << 32) - rng_range) % rng_range
        while low < threshold:
            log.append(rng_range)
            product = g.next() * rng_range
            low = product & 0xFFFFFFFF
    return product >> 32


def std_shuffle(a, g, log):
    k = len(a)
    if k == 0:
        return
    i = 1
    if k % 2 == 0:
        j = lemire_below(g, 2, log)
        a[i], a[j] = a[j], a[i]
        i += 1
    while i != k:
        swap_range = i + 1
        b1 = swap_range + 1
        x = lemire_below(g, swap_range * b1, log)
        p0, p1 = x // b1, x % b1
        a[i], a[p0] = a[p0], a[i]
        i += 1
        a[i], a[p1] = a[p1], a[i]
        i += 1


def state_with_output(u, rot, low27):
    """a pcg32 state whose next() returns u: the xorshift and the rotation inverted"""
    xs = ((u << rot) | (u >> ((32 - rot) & 31))) & 0xFFFFFFFF if rot else u
    y = (rot << 59) | (xs << 27) | (low27 & ((1 << 27) - 1))
    old = y ^ (y >> 18) ^ (y >> 36) ^ (y >> 54)
    assert Pcg32(old).next() == u
    return old


def step_back(state, n):
    for _ in range(n):
        state = ((state - INC) * MULT_INV) & M64
    return state


def rejecting_outputs(rng_range):
    threshold = (1 << 32) % rng_range
    us = [0] if threshold else []
    for t in range(1, rng_range):
        u = -((-t << 32) // rng_range)
        if u < (1 << 32) and (u * rng_range) & 0xFFFFFFFF < threshold:
            us.append(u)
    return us


def position(heights, first_owner=0):
    """bitboards of a board with the given column heights (bit = h * 7 + w, h = 0 the top row), stones alternating"""
    bb = [0, 0]
    owner = first_owner
    for w, c in enumerate(heights):
        for j in range(c):
            bb[owner] |= 1 << ((H - 1 - j) * W + w)
            owner ^= 1
    return bb[0], bb[1]


def build_cases():
    rng = np.random.default_rng(7042)
    shapes = [
        [0] * 7,                                   # empty board, k = 7
        [6, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 6], [6, 0, 0, 0, 0, 0, 6],      # full columns at the edges
        [0, 6, 6, 6, 6, 6, 6], [6, 6, 6, 6, 6, 6, 0], [0, 6, 6, 6, 6, 6, 0],      # only the edge columns open
        [6, 6, 6, 5, 6, 6, 6], [5, 6, 6, 6, 6, 6, 6], [6, 6, 6, 6, 6, 6, 5],      # one move before a full board
        [6] * 7,                                   # full board: k = 0, nothing is appended
        [6, 0, 6, 0, 6, 0, 6], [0, 6, 0, 6, 0, 6, 0], [6, 6, 0, 0, 0, 6, 6], [0, 0, 6, 6, 6, 0, 0],
        [5, 5, 5, 5, 5, 5, 5], [6, 5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5, 6],
    ]
    for k in range(0, 8):                          # random boards of every k
        for _ in range(6):
            full = rng.permutation(7)[:7 - k]
            hs = [6 if w in full else int(rng.integers(0, 6)) for w in range(7)]
            shapes.append(hs)
    cases = []
    for hs in shapes:
        for _ in range(3):                         # several RNG states per position
            cases.append((hs, int(rng.integers(0, 2)), int(rng.integers(0, 1 << 64, dtype=np.uint64))))
    # constructed rejections: for every k >= 3 and each of its pair draws (draw index d among the expansion's next() calls)
    meant = []
    for k in range(3, 8):
        first = 1 if k % 2 else 2
        pre = 0 if k % 2 else 1                    # the draw below 2 of an even k comes first
        for s, i in enumerate(range(first, k, 2)):
            rng_range = (i + 1) * (i + 2)
            for u in rejecting_outputs(rng_range)[:3]:
                old = state_with_output(u, int(rng.integers(0, 32)), int(rng.integers(0, 1 << 27)))
                start = step_back(old, pre + s)
                full = rng.permutation(7)[:7 - k]
                hs = [6 if w in full else int(rng.integers(0, 6)) for w in range(7)]
                meant.append((len(cases), rng_range))
                cases.append((hs, int(rng.integers(0, 2)), start))
    cases.append(([0] * 7, 0, 0))                  # state 0: the first output is 0
    meant.append((len(cases) - 1, 6))
    while len(cases) % (8 * REPS):
        hs = [int(rng.integers(0, 7)) for _ in range(7)]
        cases.append((hs, int(rng.integers(0, 2)), int(rng.integers(0, 1 << 64, dtype=np.uint64))))
    # call r of slot s is cases[order[s * REPS + r]]: a seeded permutation, so the groups of a wavefront differ in k
    order = rng.permutation(len(cases))
    return cases, order, meant


def reference(cases, order):
    """expected words / rng / arena, in the layout of the entry point"""
    calls = len(order)
    slots = calls // REPS
    words = np.zeros((calls, 8, 4), np.uint32)
    rng_out = np.zeros((calls, 8), np.uint64)
    arena = np.frombuffer(bytes([0xAB]) * (slots * 2 * CAP * NODE.itemsize), NODE).copy().reshape(slots, 2, CAP)
    rejected = {}
    for s in range(slots):
        bump = REPS
        for r in range(REPS):
            ci = int(order[s * REPS + r])
            hs, player, state = cases[ci]
            moves = [w for w in range(W) if hs[w] < H]
            g = Pcg32(state)
            log = []
            std_shuffle(moves, g, log)
            rejected[ci] = log
            k = len(moves)
            for lane in range(8):
                words[s * REPS + r, lane] = (moves[lane] if lane < k else 0, bump, k, 1)
                rng_out[s * REPS + r, lane] = g.state
            for j, mv in enumerate(moves):
                rec = arena[s, 0, bump + j]
                rec["n"], rec["q"], rec["pr"], rec["d"], rec["v"] = 0, 0.0, 0.0, 0.0, 0.0
                rec["meta"] = mv << 44
            arena[s, 0, r]["meta"] = bump | (k << 32) | ((r & 7) << 44) | (player << 56)
            bump += k
    return words, rng_out, arena, rejected


@pytest.fixture(scope="module")
def shared():
    """the cases and their reference, computed once for both forms of the packing"""
    cases, order, meant = build_cases()
    return (cases, order, meant) + reference(cases, order)


@pytest.fixture(scope="module", params=[0, 1], ids=["loop_pack", "lane_pack"])
def run(request, shared):
    import __graft_entry__ as g
    g.build()
    from alphazero import _capi
    cases, order, meant, want_words, want_rng, want_arena, rejected = shared
    calls = len(order)
    rows = calls // (8 * REPS)
    bb = [position(cases[int(ci)][0], first_owner=int(ci) & 1) for ci in order]
    bb0 = np.asarray([b[0] for b in bb], np.uint64)
    bb1 = np.asarray([b[1] for b in bb], np.uint64)
    player = np.asarray([cases[int(ci)][1] for ci in order], np.uint32)
    rng_in = np.asarray([cases[int(ci)][2] for ci in order], np.uint64)
    words = np.zeros((calls, 8, 4), np.uint32)
    rng_out = np.zeros((calls, 8), np.uint64)
    arena = np.zeros((calls // REPS, 2, CAP), NODE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.check(_capi.lib.azmi_debug_group_expand(0, request.param, rows, REPS, CAP, ptr(bb0), ptr(bb1), ptr(player), ptr(rng_in), ptr(words), ptr(rng_out), ptr(arena)))
    return dict(cases=cases, order=order, meant=meant, rows=rows, words=words, rng=rng_out, arena=arena,
                want_words=want_words, want_rng=want_rng, want_arena=want_arena, rejected=rejected)


def where(run, call):
    s, r = divmod(int(call), REPS)
    hs, player, state = run["cases"][int(run["order"][call])]
    return f"row {s // 8} group {s % 8} call {r} (heights {hs}, player {player}, rng {state:#018x})"


def test_the_cases_cover_what_they_should(run):
    cases, order, meant, rejected = run["cases"], run["order"], run["meant"], run["rejected"]
    ks = [sum(1 for c in hs if c < H) for hs, _, _ in cases]
    assert set(ks) == set(range(8))
    assert all(sum(1 for k in ks if k == want) >= 9 for want in range(1, 8))      # several RNG states per k
    assert any(hs[0] == 6 and hs[6] < 6 for hs, _, _ in cases) and any(hs[6] == 6 and hs[0] < 6 for hs, _, _ in cases)
    assert any(sum(hs) == 41 for hs, _, _ in cases)
    # every constructed state is rejected at a draw of the range it was made for; all five ranges of k <= 7 occur
    for ci, rng_range in meant:
        assert rng_range in rejected[ci], f"case {ci}: no rejection at range {rng_range}"
    assert {r for _, r in meant} == {6, 12, 20, 30, 42}
    # the groups of a wavefront differ: both parities of k beside each other in most wavefront steps
    mixed = 0
    for row in range(run["rows"]):
        for r in range(REPS):
            par = {ks[int(order[(row * 8 + grp) * REPS + r])] & 1 for grp in range(8)}
            mixed += len(par) == 2
    assert mixed >= run["rows"] * REPS // 2


def test_moves_c0_k_in_every_lane(run):
    got, want = run["words"], run["want_words"]
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{where(run, bad[0][0])} lane {bad[0][1]}: (move, c0, k, ok) = {got[bad[0][0], bad[0][1]].tolist()}, "
                           f"expected {want[bad[0][0], bad[0][1]].tolist()} ({len(bad)} words differ)")


def test_rng_state_afterwards_in_every_lane(run):
    got, want = run["rng"], run["want_rng"]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{where(run, bad[0][0])} lane {bad[0][1]}: rng {int(got[tuple(bad[0])]):#018x}, expected {int(want[tuple(bad[0])]):#018x}"


def test_arena_records_bit_for_bit(run):
    got = run["arena"].view(np.uint8).reshape(-1, 2, CAP, NODE.itemsize)
    want = run["want_arena"].view(np.uint8).reshape(-1, 2, CAP, NODE.itemsize)
    bad = np.argwhere((got != want).any(axis=3))
    assert bad.size == 0, (f"slot {bad[0][0]} tree {bad[0][1]} node {bad[0][2]}: {run['arena'][bad[0][0], bad[0][1], bad[0][2]]}, "
                           f"expected {run['want_arena'][bad[0][0], bad[0][1], bad[0][2]]} ({len(bad)} records differ)")
