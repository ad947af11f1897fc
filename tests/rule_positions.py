"""Placed rule positions for Connect4 and the Tafl family, as data: the places where bit-board rules break and where random
walks from the opening never get.  Plain numpy: no device, no oracle.  Every builder returns a list of cases
    (name, board, player, turn, follow-up moves or None)
board = int8 [2,6,7] (Connect4) or [3,N,N] (king, defenders, attackers).  The part of a name before the first "/" is the
family; a digit at its end is the number of pieces the LAST follow-up move is built to capture (capture1/, kingcap0/, ...).
tests/test_rule_positions.py holds every family to the behaviour it is named for through the oracle;
tests/test_gpu_rule_positions.py runs the same cases through the device rules and the search kernels."""
import itertools

import numpy as np

# ======================================================================================================================
# Connect4: board[p, h, w], h = 0 the top row
# ======================================================================================================================
C4H, C4W = 6, 7


def c4_lines():
    """the 69 four-in-a-row lines as lists of (h, w)"""
    out = []
    for h in range(C4H):
        for w in range(C4W):
            for dh, dw in ((0, 1), (1, 0), (1, 1), (1, -1)):
                cells = [(h + x * dh, w + x * dw) for x in range(4)]
                if all(0 <= a < C4H and 0 <= b < C4W for a, b in cells):
                    out.append(cells)
    assert len(out) == 69
    return out


_C4_LINE_MASKS = [sum(1 << (h * C4W + w) for h, w in line) for line in c4_lines()]


def c4_has_four(plane):
    """naive: any of the 69 lines fully set in a [6,7] plane"""
    bits = sum(1 << i for i in np.flatnonzero(np.asarray(plane).reshape(-1)))
    return any(bits & m == m for m in _C4_LINE_MASKS)


def _c4_board(cells0=(), cells1=()):
    b = np.zeros((2, C4H, C4W), np.int8)
    for h, w in cells0:
        b[0, h, w] = 1
    for h, w in cells1:
        b[1, h, w] = 1
    return b


def c4_lines_alone():
    """every line, for each player, with nothing else on the board"""
    out = []
    for p in (0, 1):
        for i, line in enumerate(c4_lines()):
            b = _c4_board(line, ()) if p == 0 else _c4_board((), line)
            out.append((f"line/alone-p{p}-{i}", b, 1 - p, 7 + p, None))
    return out


def c4_lines_embedded(seed=5):
    """every line, for each player, inside a filled board: gravity respected, stone counts as after alternate moves with the
    line's owner having moved last, the other player without a four"""
    rng = np.random.default_rng(seed)
    out = []
    for p in (0, 1):
        for i, line in enumerate(c4_lines()):
            need = [0] * C4W                              # stones each column needs to carry the line
            for h, w in line:
                need[w] = max(need[w], C4H - h)
            while True:
                heights = [int(rng.integers(n, C4H + 1)) for n in need]
                total = sum(heights)
                if total % 2 != (1 if p == 0 else 0):     # p moved last: n0 == n1 + 1 for p == 0, n0 == n1 for p == 1
                    continue
                n_p = (total + 1) // 2 if p == 0 else total // 2
                cells = [(C4H - 1 - k, w) for w in range(C4W) for k in range(heights[w])]
                rest = [c for c in cells if c not in line]
                if n_p < 4 or n_p - 4 > len(rest):
                    continue
                pick = rng.permutation(len(rest))
                mine = list(line) + [rest[j] for j in pick[: n_p - 4]]
                other = [rest[j] for j in pick[n_p - 4:]]
                b = _c4_board(mine, other) if p == 0 else _c4_board(other, mine)
                if not c4_has_four(b[1 - p]):
                    break
            out.append((f"line/embedded-p{p}-{i}", b, 1 - p, total, None))
    return out


def c4_wraps():
    """near-fours that run over the end of a row into the next one: in the bit order h * 7 + w they are four stones at a line's
    stride.  Every one is a running game."""
    out = []
    for p in (0, 1):
        for stride, name, starts in ((1, "row", (4, 5, 6)), (8, "diag", (4, 5, 6)), (6, "anti", (0, 1, 2))):
            for h in range(C4H):
                for w in starts:
                    idx = [h * C4W + w + stride * x for x in range(4)]
                    if idx[-1] >= C4H * C4W:
                        continue
                    cells = [(i // C4W, i % C4W) for i in idx]
                    b = _c4_board(cells, ()) if p == 0 else _c4_board((), cells)
                    assert not c4_has_four(b[p])
                    out.append((f"wrap/{name}-p{p}-h{h}w{w}", b, 1 - p, 7 + p, None))
    return out


def _c4_full_boards():
    """full boards of 21 + 21 stones without a four: stone (h, w) belongs to (pat[w] + h) % 2, so columns alternate and a row
    is the pattern itself; pat has neither four equal nor four alternating neighbours (the diagonals), and 3 or 4 ones"""
    out = []
    for bits in itertools.product((0, 1), repeat=C4W):
        if sum(bits) not in (3, 4):
            continue
        b = np.zeros((2, C4H, C4W), np.int8)
        for h in range(C4H):
            for w in range(C4W):
                b[(bits[w] + h) % 2, h, w] = 1
        if not c4_has_four(b[0]) and not c4_has_four(b[1]):
            assert b[0].sum() == 21 and b[1].sum() == 21
            out.append(b)
    return out


def c4_full():
    boards = _c4_full_boards()
    assert len(boards) >= 8
    return [(f"full/{i}", b, 0, 42, None) for i, b in enumerate(boards)]


def c4_last_move():
    """41 stones, player 1 to move into the one open cell: "lastdraw/" fills the board without a four, "lastwin/" completes a
    four (two stones of a drawn board swapped so that the counts stay 21 + 20)"""
    out = []
    wins = 0
    for i, full in enumerate(_c4_full_boards()):
        for c in range(C4W):
            if full[1, 0, c] != 1:
                continue
            b = full.copy()
            b[1, 0, c] = 0
            out.append((f"lastdraw/{i}-c{c}", b, 1, 41, [c]))
            if wins >= 24 or (i + c) % 3:
                continue
            for (h0, w0), (h1, w1) in itertools.product(np.argwhere(b[0] == 1), np.argwhere(b[1] == 1)):
                g = b.copy()
                g[0, h0, w0] = 0; g[1, h0, w0] = 1; g[1, h1, w1] = 0; g[0, h1, w1] = 1
                if c4_has_four(g[0]) or c4_has_four(g[1]):
                    continue
                after = g[1].copy(); after[0, c] = 1
                if c4_has_four(after):
                    out.append((f"lastwin/{i}-c{c}", g, 1, 41, [c]))
                    wins += 1
                    break
    assert wins >= 8
    return out


def c4_one_open():
    """exactly one open column with 1..6 free cells; the follow-up drops into it"""
    out = []
    for i, full in enumerate(_c4_full_boards()[:6]):
        for c in range(C4W):
            for k in range(1, C4H + 1):
                if (i + c + k) % 3:
                    continue
                b = full.copy()
                b[:, :k, c] = 0
                out.append((f"oneopen/{i}-c{c}-k{k}", b, (42 - k) % 2, 42 - k, [c]))
    return out


def c4_illegal():
    """a drop into a full column"""
    out = []
    for name, b, player, turn, moves in c4_one_open()[:20]:
        c = moves[0]
        out.append((f"illegal/{name}", b, player, turn, [(c + 1) % C4W]))
    return out


def c4_near_win():
    """nearwin/: three in a row on the bottom row or in a column for the side to move, the follow-up completes the four"""
    out = []
    for p in (0, 1):
        for w in range(5):
            mine, other = [(5, w + x) for x in range(3)], [(4, w + x) for x in range(3)] + [(5, (w + 5) % C4W)] * p
            b = _c4_board(mine, other) if p == 0 else _c4_board(other, mine)
            out.append((f"nearwin/row-p{p}-w{w}", b, p, 6 + p, [w + 3 if w < 4 else w - 1]))
        for c in range(C4W):
            o = (c + 2) % C4W
            mine, other = [(5 - x, c) for x in range(3)], [(5 - x, o) for x in range(3)] + [(5, (c + 4) % C4W)] * p
            b = _c4_board(mine, other) if p == 0 else _c4_board(other, mine)
            out.append((f"nearwin/col-p{p}-c{c}", b, p, 6 + p, [c]))
    return out


def c4_all():
    return c4_lines_alone() + c4_lines_embedded() + c4_wraps() + c4_full() + c4_last_move() + c4_one_open() + c4_near_win()


# ======================================================================================================================
# Tafl family
# ======================================================================================================================
K, D, A = 0, 1, 2          # layers
ATK, DEF = 0, 1            # players


class Spec:
    def __init__(self, name, game_id, n, max_turns, special, strong_king):
        self.name, self.game_id, self.N, self.T, self.max_turns = name, game_id, n, n // 2, max_turns
        self.special = special          # corners and throne are special squares; the king wins on a corner (else: on any edge)
        self.strong_king = strong_king  # the king needs four hostile sides, is safe on an edge; attackers win by encirclement

    def corner(self, h, w):
        return h in (0, self.N - 1) and w in (0, self.N - 1)

    def throne(self, h, w):
        return h == self.T and w == self.T

    def inside(self, h, w):
        return 0 <= h < self.N and 0 <= w < self.N

    def restricted(self, h, w):
        """squares a non-king piece never stands on"""
        return self.special and (self.corner(h, w) or self.throne(h, w))

    def mv(self, fh, fw, th, tw):
        """move index of a slide (fh, fw) -> (th, tw): (fh * N + fw) * 2N + (column move ? N + new_h : new_w)"""
        assert (fh == th) != (fw == tw)
        return (fh * self.N + fw) * 2 * self.N + (tw if fh == th else self.N + th)

    def unmv(self, m):
        """-> (fh, fw, th, tw)"""
        frm, tgt = divmod(int(m), 2 * self.N)
        fh, fw = divmod(frm, self.N)
        return (fh, fw, tgt - self.N, fw) if tgt >= self.N else (fh, fw, fh, tgt)


TAWLBWRDD = Spec("TawlbwrddGS", 1, 11, 400, False, False)
BRANDUBH = Spec("BrandubhGS", 2, 7, 150, True, False)
OPENTAFL = Spec("OpenTaflGS", 3, 11, 400, True, True)
TAFL_SPECS = (TAWLBWRDD, BRANDUBH, OPENTAFL)

DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def _board(spec, pieces):
    b = np.zeros((3, spec.N, spec.N), np.int8)
    for layer, h, w in pieces:
        assert spec.inside(h, w) and b[:, h, w].sum() == 0, (pieces, h, w)
        b[layer, h, w] = 1
    return b


def _park_king(spec, b, lines=()):
    """put the king where it takes no part: an empty interior square that is not the throne, two or more squares from every
    piece, and on none of `lines` = [(h, None) | (None, w)] (the rows / columns under test)"""
    if b[K].any():
        return b
    occ = np.argwhere(b.sum(0) > 0)
    rows = {h for h, w in lines if h is not None}
    cols = {w for h, w in lines if w is not None}
    for h in range(1, spec.N - 1):
        for w in range(1, spec.N - 1):
            if spec.throne(h, w) or h in rows or w in cols:
                continue
            if all(max(abs(h - a), abs(w - c)) >= 2 for a, c in occ):
                b[K, h, w] = 1
                return b
    raise AssertionError("no square to park the king on")


def _owner(layer):
    return ATK if layer == A else DEF


def _rot(spec, case, k):
    """the case turned by k quarter turns (counter-clockwise, as np.rot90): (h, w) -> (N-1-w, h) per turn"""
    name, b, player, turn, moves = case
    n = spec.N

    def sq(h, w):
        for _ in range(k % 4):
            h, w = n - 1 - w, h
        return h, w

    def turn_move(m):
        fh, fw, th, tw = spec.unmv(m)
        return spec.mv(*sq(fh, fw), *sq(th, tw))
    return (f"{name}-r{k}", np.ascontiguousarray(np.rot90(b, k, axes=(1, 2))), player, turn,
            None if moves is None else [turn_move(m) for m in moves])


def _rotations(spec, case):
    return [_rot(spec, case, k) for k in range(4)]


# ---- slides ----------------------------------------------------------------------------------------------------------
def _ray_squares(spec, h, w, dh, dw):
    out = []
    h, w = h + dh, w + dw
    while spec.inside(h, w):
        out.append((h, w))
        h, w = h + dh, w + dw
    return out


def tafl_slides(spec, cap=2500):
    """a lone mover of each kind on every square of the rows and columns 0, T-1, T, T+1, N-1 ("slide0/"); one blocker at
    every distance on each of its four rays ("slide1/"); two blockers, on one ray or on two ("slide2/").  On an 11 x 11 board
    row T is squares 55..65, across the two words of the bit board.  No follow-up: the legal-move mask is what is compared.
    The blocker families are thinned to `cap` cases each; what touches row or column T is always kept."""
    n, t = spec.N, spec.T
    band = {0, t - 1, t, t + 1, n - 1}
    lone, one, two = [], [], []
    idx = 0
    for h in range(n):
        for w in range(n):
            if h not in band and w not in band:
                continue
            for kind in (A, D, K):
                if kind != K and spec.restricted(h, w):
                    continue
                b = _park_king(spec, _board(spec, [(kind, h, w)]), [(h, None), (None, w)])
                lone.append((f"slide0/{'KDA'[kind]}@{h},{w}", b, _owner(kind), 10, None))
            rays = [[s for s in _ray_squares(spec, h, w, dh, dw) if not spec.restricted(*s)] for dh, dw in DIRS]
            singles = [s for ray in rays for s in ray]
            pairs = [(a, c) for ray in rays for a, c in zip(ray, ray[1:])]                     # neighbours on one ray
            pairs += [(ray[0], ray[-1]) for ray in rays if len(ray) > 2]
            pairs += [(a, c) for r0, r1 in ((rays[0], rays[1]), (rays[2], rays[3])) for a in r0 for c in r1]   # either side
            pairs += [(a, c) for a in rays[0][:2] + rays[1][:2] for c in rays[2][:2] + rays[3][:2]]           # row and column
            for blockers, sink in [((s,), one) for s in singles] + [(p, two) for p in pairs]:
                idx += 1
                kind = (A, D, K)[idx % 3]
                if kind != K and spec.restricted(h, w):
                    kind = K
                pieces = [(kind, h, w)] + [((A, D)[(idx + j) % 2], bh, bw) for j, (bh, bw) in enumerate(blockers)]
                b = _park_king(spec, _board(spec, pieces), [(h, None), (None, w)])
                keep = h == t or w == t or any(bh == t or bw == t for bh, bw in blockers)
                sink.append((keep, (f"slide{len(blockers)}/{'KDA'[kind]}@{h},{w}|" + "|".join(f"{a},{c}" for a, c in blockers),
                                    b, _owner(kind), 10, None)))

    def thin(cases):
        kept = [c for keep, c in cases if keep]
        rest = [c for keep, c in cases if not keep]
        room = max(cap - len(kept), 0)
        step = max(1, -(-len(rest) // max(room, 1)))
        return kept[:cap] + (rest[::step] if room else [])
    return lone + thin(one) + thin(two)


def tafl_special_squares(spec):
    """Brandubh / OpenTafl: a non-king piece next to a corner cannot enter it; in line with the empty throne it passes and
    cannot land ("throne-empty"); with the king on the throne the throne blocks ("throne-king"); the king slides onto the
    throne and onto every corner (follow-up moves)."""
    assert spec.special
    n, t = spec.N, spec.T
    out = []
    for kind in (A, D):
        c = "KDA"[kind]
        for h, w in ((0, 1), (1, 0)):
            base = (f"special/corner-{c}@{h},{w}", _park_king(spec, _board(spec, [(kind, h, w)]), [(h, None), (None, w)]), _owner(kind), 10, None)
            out += _rotations(spec, base)
        for d in range(1, t + 1):
            for far in (False, True):                     # a second piece beyond the throne: how far the pass reaches
                pieces = [(kind, t, t - d)] + ([((A, D)[d % 2], t, n - 1)] if far else [])
                tag = f"{c}-d{d}{'-far' if far else ''}"
                b = _park_king(spec, _board(spec, pieces), [(t, None), (None, t)])
                out += _rotations(spec, (f"special/throne-empty-{tag}", b, _owner(kind), 10, None))
                b = _board(spec, pieces + [(K, t, t)])
                out += _rotations(spec, (f"special/throne-king-{tag}", b, _owner(kind), 10, None))
    for d in range(1, t + 1):
        b = _board(spec, [(K, t, t - d), (A, 1, 1)])
        out += _rotations(spec, (f"special/king-to-throne-d{d}", b, DEF, 10, [spec.mv(t, t - d, t, t)]))
    for w in range(1, n - 1):
        for tw in (0, n - 1):
            b = _board(spec, [(K, 0, w), (A, t, t - 1)])
            out += _rotations(spec, (f"kingwin/corner-from-{w}-to-{tw}", b, DEF, 10, [spec.mv(0, w, 0, tw)]))
    return out


# ---- captures --------------------------------------------------------------------------------------------------------
def _arrivals(spec, b, dest, kind, victim_dirs):
    """start squares from which a piece of `kind` slides onto the empty `dest`: from each side that holds no victim, two
    squares out, or one where the board, a piece or a special square leaves no more"""
    out = []
    for dh, dw in DIRS:
        if (dh, dw) in victim_dirs:
            continue
        for dist in (2, 1):
            path = [(dest[0] + dh * x, dest[1] + dw * x) for x in range(1, dist + 1)]
            if not all(spec.inside(*s) and b[:, s[0], s[1]].sum() == 0 for s in path):
                continue
            if any(spec.special and spec.corner(*s) for s in path) or (kind != K and spec.restricted(*path[-1])):
                continue
            out.append(path[-1])
            break
    return out


def _capture_cases(spec, name, pieces, dest, mover_kind, victim_dirs, king_lines=None, turn=10):
    """the position `pieces` + a mover of `mover_kind` arriving on `dest` from every free side"""
    base = _board(spec, pieces)
    out = []
    for sh, sw in _arrivals(spec, base, dest, mover_kind, victim_dirs):
        b = base.copy()
        b[mover_kind, sh, sw] = 1
        if not b[K].any():
            rows_cols = [(dest[0], None), (None, dest[1])] + [(h, None) for _, h, _ in pieces] + [(None, w) for _, _, w in pieces]
            b = _park_king(spec, b, rows_cols if king_lines is None else king_lines)
        out.append((f"{name}-from{sh},{sw}", b, _owner(mover_kind), turn, [spec.mv(sh, sw, dest[0], dest[1])]))
    assert out, name
    return out


def tafl_captures(spec):
    """captureN/: the follow-up move takes N pieces.  Custodial against a piece (also with the victim on squares 63 and 64),
    against a corner, the empty throne, the throne with the king on it (a defender survives, an attacker does not), at the
    board edge (nothing), two and three at once; for every victim direction, the mover arriving from every free side."""
    n, t = spec.N, spec.T
    out = []
    # victims for the plain custodial case: interior squares away from the special squares, + squares 63 and 64
    victims = [(2, 2), (t + 1, 2)] + ([(63 // n, 63 % n), (64 // n, 64 % n)] if n * n > 64 else [])
    for vh, vw in victims:
        for dh, dw in DIRS:
            dest, anchor = (vh - dh, vw - dw), (vh + dh, vw + dw)
            if not (spec.inside(*dest) and spec.inside(*anchor)) or spec.restricted(*dest) or spec.restricted(*anchor):
                continue
            for mover, victim in ((A, D), (D, A)):
                out += _capture_cases(spec, f"capture1/piece-{'KDA'[victim]}@{vh},{vw}-d{dh},{dw}", [(victim, vh, vw), (mover, *anchor)],
                                      dest, mover, [(dh, dw)])
    # the board edge is not hostile
    for (vh, vw), (dh, dw) in (((0, 3), (-1, 0)), ((n - 1, 2), (1, 0)), ((2, 0), (0, -1)), ((3, n - 1), (0, 1))):
        for mover, victim in ((A, D), (D, A)):
            out += _capture_cases(spec, f"capture0/edge-{'KDA'[victim]}@{vh},{vw}", [(victim, vh, vw)], (vh - dh, vw - dw), mover, [(dh, dw)])
    # two and three at once: victims around (2, 3), each backed by a piece of the mover's side
    for count in (2, 3):
        for dirs in itertools.combinations(DIRS, count):
            for mover, victim in ((A, D), (D, A)):
                dest = (3, 3) if n > 7 else (2, 4)
                pieces = []
                for dh, dw in dirs:
                    pieces += [(victim, dest[0] + dh, dest[1] + dw), (mover, dest[0] + 2 * dh, dest[1] + 2 * dw)]
                if any(not spec.inside(h, w) or spec.restricted(h, w) for _, h, w in pieces):
                    continue
                tag = "".join("NSWE"[DIRS.index(d)] for d in dirs)
                out += _capture_cases(spec, f"capture{count}/multi-{'KDA'[victim]}-{tag}", pieces, dest, mover, list(dirs))
    if not spec.special:
        return out
    # against a corner: the victim next to it, the mover on the other side
    for (vh, vw), (dh, dw) in (((0, 1), (0, -1)), ((1, 0), (-1, 0)), ((0, n - 2), (0, 1)), ((1, n - 1), (-1, 0)),
                               ((n - 1, 1), (0, -1)), ((n - 2, 0), (1, 0)), ((n - 1, n - 2), (0, 1)), ((n - 2, n - 1), (1, 0))):
        for mover, victim in ((A, D), (D, A)):
            out += _capture_cases(spec, f"capture1/corner-{'KDA'[victim]}@{vh},{vw}", [(victim, vh, vw)], (vh - dh, vw - dw), mover, [(dh, dw)])
    # against the throne: the victim next to it, the mover opposite
    for dh, dw in DIRS:
        vh, vw = t - dh, t - dw
        dest = (vh - dh, vw - dw)
        lines = [(t, None), (None, t), (vh, None), (None, vw), (dest[0], None), (None, dest[1])]
        for mover, victim in ((A, D), (D, A)):
            out += _capture_cases(spec, f"capture1/throne-empty-{'KDA'[victim]}-d{dh},{dw}", [(victim, vh, vw)], dest, mover, [(dh, dw)],
                                  king_lines=lines)
        out += _capture_cases(spec, f"capture0/throne-king-D-d{dh},{dw}", [(D, vh, vw), (K, t, t)], dest, A, [(dh, dw)])
        out += _capture_cases(spec, f"capture1/throne-king-A-d{dh},{dw}", [(A, vh, vw), (K, t, t)], dest, D, [(dh, dw)])
    return out


def tafl_kings(spec):
    """kingcapN/: the follow-up takes the king (1) or leaves it (0).  Tawlbwrdd and Brandubh: between two attackers.  OpenTafl:
    four attackers, three and the throne; three alone and three on an edge do not.  kingwin/: the king steps onto an edge
    (Tawlbwrdd) or a corner."""
    n, t = spec.N, spec.T
    out = []
    if not spec.strong_king:
        for kh, kw in ((2, 2), (t, t - 2)) + (((63 // n, 63 % n),) if n * n > 64 else ()):
            for dh, dw in DIRS:
                dest, anchor = (kh - dh, kw - dw), (kh + dh, kw + dw)
                if spec.restricted(*dest) or spec.restricted(*anchor):
                    continue
                out += _capture_cases(spec, f"kingcap1/custodial@{kh},{kw}-d{dh},{dw}", [(K, kh, kw), (A, *anchor)], dest, A, [(dh, dw)])
    else:
        for dh, dw in DIRS:                      # the mover closes the side (-dh, -dw) of the king
            for kh, kw in ((3, 3), (63 // n, 63 % n)):
                others = [(kh + a, kw + c) for a, c in DIRS if (a, c) != (-dh, -dw)]
                dest = (kh - dh, kw - dw)
                out += _capture_cases(spec, f"kingcap1/four@{kh},{kw}-d{dh},{dw}", [(K, kh, kw)] + [(A, *s) for s in others], dest, A, [(dh, dw)])
                out += _capture_cases(spec, f"kingcap0/three@{kh},{kw}-d{dh},{dw}", [(K, kh, kw)] + [(A, *s) for s in others[1:]], dest, A, [(dh, dw)])
            # next to the throne: the throne is the fourth side
            for th, tw in DIRS:
                kh, kw = t + th, t + tw
                if (-dh, -dw) == (-th, -tw):
                    continue                     # that side is the throne itself
                others = [(kh + a, kw + c) for a, c in DIRS if (a, c) != (-dh, -dw) and (a, c) != (-th, -tw)]
                dest = (kh - dh, kw - dw)
                out += _capture_cases(spec, f"kingcap1/throne@{kh},{kw}-d{dh},{dw}", [(K, kh, kw)] + [(A, *s) for s in others], dest, A, [(dh, dw)])
        # on an edge with three attackers: safe (a free defender keeps the side mobile)
        base = _board(spec, [(K, 0, 3), (A, 0, 2), (A, 1, 3), (A, 0, 7), (D, t + 1, t + 2)])
        out += _rotations(spec, ("kingcap0/edge", base, ATK, 10, [spec.mv(0, 7, 0, 4)]))
    if spec.special:
        for w in (1, 2, n - 2):
            b = _board(spec, [(K, 0, w), (A, t + 1, t + 1)])
            out += _rotations(spec, (f"kingwin/corner-{w}", b, DEF, 10, [spec.mv(0, w, 0, 0 if w < t else n - 1)]))
    else:
        for w in (1, t, n - 2):
            for d in (1, 3):
                b = _board(spec, [(K, d, w), (A, t + 2, t + 2)])
                out += _rotations(spec, (f"kingwin/edge-{w}-d{d}", b, DEF, 10, [spec.mv(d, w, 0, w)]))
    return out


# ---- endings ---------------------------------------------------------------------------------------------------------
def _ring(lo, hi):
    """the attackers on the outline of the square lo..hi without its corners: the fill is 4-connected, so every one is needed"""
    return sorted({(A, lo, x) for x in range(lo + 1, hi)} | {(A, hi, x) for x in range(lo + 1, hi)}
                  | {(A, x, lo) for x in range(lo + 1, hi)} | {(A, x, hi) for x in range(lo + 1, hi)})


def tafl_encirclement(spec):
    """OpenTafl.  encircled/: a closed attacker ring around every defender and the king; gap/: the same ring with one attacker
    missing, a spare attacker standing in line with the gap (one move from closing it), or with one defender outside."""
    assert spec.strong_king
    n = spec.N
    out = []
    rings = [("box", _ring(3, 7), [(K, 5, 5), (D, 4, 4), (D, 6, 5)], (D, 1, 8)),
             ("wide", _ring(1, 9), [(K, 5, 5), (D, 2, 2), (D, 8, 8), (D, 5, 8), (D, 5, 9 - 1)], None),
             ("small", _ring(4, 6), [(K, 5, 5)], (D, 8, 2)),
             # a ring that stands on the rim: the region (1,1), (1,2) closed by rim squares and two inner ones
             ("rim", [(A, 0, 1), (A, 0, 2), (A, 1, 0), (A, 1, 3), (A, 2, 1), (A, 2, 2)], [(K, 1, 1), (D, 1, 2)], (D, 5, 5 + 2)),
             ("rim-side", [(A, 4, 0), (A, 5, 0), (A, 6, 0), (A, 3, 1), (A, 7, 1), (A, 4, 2), (A, 5, 2), (A, 6, 2)],
              [(K, 5, 1), (D, 4, 1), (D, 6, 1)], (D, 8, 8))]
    for name, ring, inner, outsider in rings:
        inner = list(dict.fromkeys(inner))
        for player in (ATK, DEF):
            out.append((f"encircled/{name}-p{player}", _board(spec, ring + inner), player, 10, None))
        for i, gap in enumerate(ring):
            if name == "wide" and i % 4:
                continue
            _, gh, gw = gap
            pieces = [p for p in ring if p != gap] + inner
            b = _board(spec, pieces)
            spare = None
            for dh, dw in DIRS:                                    # a spare attacker two squares outside the gap, if there is room
                s1, s2 = (gh + dh, gw + dw), (gh + 2 * dh, gw + 2 * dw)
                if all(spec.inside(*s) and not spec.restricted(*s) and b[:, s[0], s[1]].sum() == 0 for s in (s1, s2)):
                    nb = [(s1[0] + a, s1[1] + c) for a, c in DIRS]
                    if any((D, *q) in inner or (K, *q) in inner for q in nb):
                        continue                                  # that side is the inside
                    spare = s2
                    break
            moves = None
            if spare is not None:
                b[A, spare[0], spare[1]] = 1
                moves = [spec.mv(spare[0], spare[1], gh, gw)]
            out.append((f"gap/{name}-{gh},{gw}", b, ATK, 10, moves))
        if outsider is not None:
            out.append((f"gap/{name}-outsider", _board(spec, ring + inner + [outsider]), DEF, 10, None))
    return out


def tafl_boxed(spec):
    """boxed/: the side to move has pieces and none of them can move; the other side wins.  Not encircled: a defender
    stands on the rim, or the king alone is shut in (Tawlbwrdd, Brandubh)."""
    n = spec.N
    out = []
    if spec.special:
        atk = [(A, 0, 1), (D, 0, 2), (D, 1, 1), (K, 3, 4) if n == 7 else (K, 5, 6)]
        dfn = [(D, 0, 1), (D, 1, 0), (K, 1, 1), (A, 0, 2), (A, 1, 2), (A, 2, 1), (A, 2, 0)]
        atk2 = atk + [(A, 1, 0), (D, 2, 0)]
    else:
        atk = [(A, 0, 0), (D, 0, 1), (D, 1, 0), (K, 5, 6)]
        dfn = [(K, 1, 1), (A, 0, 1), (A, 1, 0), (A, 1, 2), (A, 2, 1)]
        atk2 = atk + [(A, 0, n - 1), (D, 0, n - 2), (D, 1, n - 1)]
    # on column 0 away from the corner: one square west of it, in bit order, is the far end of the row above
    col0 = [(A, 3, 0), (D, 2, 0), (D, 4, 0), (D, 3, 1), (K, 3, 4) if n == 7 else (K, 5, 6)]
    for tag, pieces, player in (("atk", atk, ATK), ("atk2", atk2, ATK), ("atk-col0", col0, ATK), ("def", dfn, DEF)):
        out += _rotations(spec, (f"boxed/{tag}", _board(spec, pieces), player, 10, None))
    if not spec.strong_king:                     # the king alone between four attackers in the open (no encirclement rule)
        out.append(("boxed/def-king-alone", _board(spec, [(K, 2, 2), (A, 1, 2), (A, 3, 2), (A, 2, 1), (A, 2, 3)]), DEF, 10, None))
    return out


def tafl_forced(spec):
    """forced/: the side to move has exactly one legal move (the boxed attacker with one square of room)"""
    if spec.special:
        pieces = [(A, 0, 1), (D, 0, 3), (D, 1, 1), (K, 3, 4) if spec.N == 7 else (K, 5, 6)]
        move = spec.mv(0, 1, 0, 2)
    else:
        pieces = [(A, 0, 0), (D, 0, 2), (D, 1, 0), (K, 5, 6)]
        move = spec.mv(0, 0, 0, 1)
    return _rotations(spec, ("forced/atk", _board(spec, pieces), ATK, 10, [move]))


def tafl_last_turn(spec):
    """lastturn/: turn = MAX_TURNS - 1 and a quiet move: the draw.  lastturn-win/: the same turn and the king's winning move"""
    n, t = spec.N, spec.T
    out = []
    b = _board(spec, [(K, t, t), (D, t, t - 1), (A, 1, 2), (A, n - 2, 3)])
    out.append(("lastturn/atk", b, ATK, spec.max_turns - 1, [spec.mv(1, 2, 1, 3)]))
    out.append(("lastturn/def", b, DEF, spec.max_turns - 1, [spec.mv(t, t - 1, t - 1, t - 1)]))
    out.append(("lastturn/def-king", b, DEF, spec.max_turns - 1, [spec.mv(t, t, t + 1, t)]))
    b = _board(spec, [(K, 0, 2) if spec.special else (K, 1, 2), (A, t, t - 1), (A, n - 2, 3)])
    out.append(("lastturn-win/king", b, DEF, spec.max_turns - 1, [spec.mv(0, 2, 0, 0) if spec.special else spec.mv(1, 2, 0, 2)]))
    return out


def tafl_repetition(spec):
    """repetition/: a shuffle played from a placed board until a position stands for the third time; the side to move is
    credited.  From turn 0 the start position counts and stands for the third time after 8 moves; from a later turn it does
    not, and the position behind the first move is the first to come back twice, after 9.  repetition-short/: one move less."""
    n, t = spec.N, spec.T
    b = _board(spec, [(K, t, t), (D, t + 1, t), (A, 1, 2), (A, n - 2, 3)])
    cycle = [spec.mv(1, 2, 1, 3), spec.mv(t + 1, t, t + 1, t + 1), spec.mv(1, 3, 1, 2), spec.mv(t + 1, t + 1, t + 1, t)]
    out = []
    for turn, length in ((0, 8), (10, 9)):
        for cut in (0, 1, 4):
            out.append((f"repetition{'' if cut == 0 else '-short'}/turn{turn}-cut{cut}", b, ATK, turn, (cycle * 3)[: length - cut]))
    return out


def tafl_illegal(spec):
    """illegal/: a follow-up the rules refuse: a slide through a blocker, onto the blocker, of the other side's piece, and, with
    special squares, a non-king piece onto a corner or the throne"""
    n, t = spec.N, spec.T
    out = []
    b = _park_king(spec, _board(spec, [(A, 2, 1), (D, 2, 4), (A, t + 1, 8 % n)]), [(2, None)])
    out.append(("illegal/through", b, ATK, 10, [spec.mv(2, 1, 2, 5)]))
    out.append(("illegal/onto", b, ATK, 10, [spec.mv(2, 1, 2, 4)]))
    out.append(("illegal/not-mine", b, ATK, 10, [spec.mv(2, 4, 2, 3)]))
    out.append(("illegal/empty-square", b, ATK, 10, [spec.mv(1, 1, 1, 2)]))
    b = _park_king(spec, _board(spec, [(D, t, 1), (A, t, n - 2)]), [(t, None), (None, t)])
    out.append(("illegal/across-board", b, DEF, 10, [spec.mv(t, 1, t, n - 1)]))
    if spec.special:
        b = _park_king(spec, _board(spec, [(A, 0, 2), (D, t, 1)]), [(0, None), (t, None), (None, t)])
        out.append(("illegal/corner", b, ATK, 10, [spec.mv(0, 2, 0, 0)]))
        out.append(("illegal/throne", b, DEF, 10, [spec.mv(t, 1, t, t)]))
    return out


def tafl_dense(spec, count=1500, seed=23):
    """dense/: seeded random boards, 1/8 .. 6/8 of the squares occupied, two attackers for every defender, the king on any
    square a king may stand on, either side to move.  The follow-up is chosen by the test from the oracle's legal moves."""
    rng = np.random.default_rng(seed + spec.game_id)
    n = spec.N
    free = [(h, w) for h in range(n) for w in range(n) if not spec.restricted(h, w)]
    out = []
    for i in range(count):
        eighths = 1 + i % 6
        k = max(2, n * n * eighths // 8)
        b = np.zeros((3, n, n), np.int8)
        kh, kw = divmod(int(rng.integers(n * n)), n)
        b[K, kh, kw] = 1
        cells = [free[j] for j in rng.permutation(len(free)) if free[j] != (kh, kw)][: k - 1]
        for h, w in cells:
            b[A if rng.random() < 2 / 3 else D, h, w] = 1
        turn = int(rng.integers(1, spec.max_turns - 1))
        out.append((f"dense/{eighths}-{i}", b, int(rng.integers(2)), turn, None))
    return out


def tafl_placed(spec):
    """every hand-placed family of one game (dense and illegal are separate)"""
    out = tafl_slides(spec) + tafl_captures(spec) + tafl_kings(spec) + tafl_boxed(spec) + tafl_forced(spec)
    out += tafl_last_turn(spec) + tafl_repetition(spec)
    if spec.special:
        out += tafl_special_squares(spec)
    if spec.strong_king:
        out += tafl_encirclement(spec)
    return out


def family(name):
    return name.split("/", 1)[0]


def by_family(cases):
    out = {}
    for c in cases:
        out.setdefault(family(c[0]), []).append(c)
    return out
