"""A plain restatement of the search's root read-outs (mcts.cc:557-674, 717-750; root_value: mcts.h:78-100) and the scripted
sharp evaluators the read-out tests feed the trees with.  numpy scalars only: every value is a float32, every sum runs
sequentially in float32 (dense vectors in ascending move order, child loops in stored order), pow / log are
np.float32(math.pow(float64, float64)) / np.float32(math.log(float64)) - the definition the oracle and the device share."""
import hashlib
import math

import numpy as np

f32 = np.float32

# 0 and 1 are the branches without pow; 2 flattens; 0.5 and 0.2 (self-play's final_temp) sharpen; 0.6137 is a decayed temperature
# (an inexact exponent); 0.05 pushes small entries into the float32 denormal range
TEMPS = (0.0, 1.0, 2.0, 0.5, 0.2, 0.6137, 0.05)


def _pow(x, e):
    return f32(math.pow(float(x), float(e)))


def _log(x):
    return f32(math.log(float(x)))


def _seq_sum(x):
    s = f32(0.0)
    for e in x:
        s = f32(s + f32(e))
    return s


class Root:
    """The numbers the read-outs are functions of: root children (move, n, q, policy, d) in stored order, the root's own
    n, v, d, and cpuct / num_players / num_moves."""

    def __init__(self, move, n, q, policy, d, root_n, root_v, root_d, cpuct, num_players, num_moves):
        self.move = [int(x) for x in move]
        self.n = [int(x) for x in n]
        self.q = [f32(x) for x in q]
        self.policy = [f32(x) for x in policy]
        self.d = [f32(x) for x in d]
        self.root_n, self.root_v, self.root_d = int(root_n), f32(root_v), f32(root_d)
        self.cpuct, self.P, self.M = f32(cpuct), int(num_players), int(num_moves)
        self.k = len(self.move)


def counts(r):                                                    # mcts.cc:557-564
    out = np.zeros(r.M, np.uint32)
    for i in range(r.k):
        out[r.move[i]] = r.n[i]
    return out


def root_q(r):                                                    # mcts.cc:566-573
    out = np.zeros(r.M, np.float32)
    for i in range(r.k):
        out[r.move[i]] = r.q[i]
    return out


def _pow_all(p, e):
    for m in range(len(p)):
        p[m] = _pow(p[m], e)


def _div_all(p, s):
    with np.errstate(all="ignore"):
        for m in range(len(p)):
            p[m] = f32(p[m]) / f32(s)


def probs(r, temp):                                               # mcts.cc:575-618
    temp = f32(temp)
    cnt = counts(r)
    p = np.zeros(r.M, np.float32)
    count_sum = _seq_sum(f32(c) for c in cnt)
    with np.errstate(all="ignore"):
        if count_sum == 0:
            for i in range(r.k):
                p[r.move[i]] = r.policy[i]
            if temp != 0:
                _pow_all(p, f32(1.0) / temp)
            _div_all(p, _seq_sum(p))
            return p
        if temp == 0:
            best, best_count = [0], cnt[0]
            for m in range(1, r.M):
                if cnt[m] > best_count:
                    best_count, best = cnt[m], [m]
                elif cnt[m] == best_count:
                    best.append(m)
            for m in best:
                p[m] = f32(1.0 / len(best))                       # 1.0 / size in double, then to float
            return p
        for m in range(r.M):
            p[m] = f32(cnt[m])
        _div_all(p, _seq_sum(p))
        _pow_all(p, f32(1.0) / temp)
        _div_all(p, _seq_sum(p))
        return p


def probs_pruned(r, temp):                                        # mcts.cc:620-674
    temp = f32(temp)
    if r.root_n <= 1:
        return probs(r, temp)
    with np.errstate(all="ignore"):
        explore_scaling = f32(r.cpuct * np.sqrt(f32(r.root_n)))
        best_sel = f32(-1e30)
        for i in range(r.k):
            if r.n[i] == 0:
                continue
            sel = f32(r.q[i] + f32(f32(explore_scaling * r.policy[i]) / f32(r.n[i] + 1)))
            if sel > best_sel:
                best_sel = sel
        pruned = np.zeros(r.M, np.float32)
        for i in range(r.k):
            if r.n[i] == 0:
                continue
            nf = f32(r.n[i])
            gap = f32(best_sel - r.q[i])
            if gap <= 0:
                desired = nf
            else:
                desired = f32(f32(f32(explore_scaling * r.policy[i]) / gap) - f32(1.0))
            lo = desired if f32(0.0) < desired else f32(0.0)      # std::max(0.0f, desired)
            pruned[r.move[i]] = lo if lo < nf else nf             # std::min(n, .)
        total = _seq_sum(pruned)
        if total == 0:
            return probs(r, temp)
        if temp == 0:
            best_val = pruned[0]
            for m in range(1, r.M):
                best_val = pruned[m] if best_val < pruned[m] else best_val
            count = int(sum(1 for m in range(r.M) if pruned[m] == best_val))
            out = np.zeros(r.M, np.float32)
            for m in range(r.M):
                if pruned[m] == best_val:
                    out[m] = f32(1.0) / f32(count)                # 1.0f / count in float
            return out
        _div_all(pruned, total)
        if temp != 1:
            _pow_all(pruned, f32(1.0) / temp)
            _div_all(pruned, _seq_sum(pruned))
        return pruned


def pick_move(p, u):                                              # mcts.cc:717-735, `u` the uniform it drew
    u = f32(u)
    s = f32(0.0)
    for m in range(len(p)):
        s = f32(s + f32(p[m]))
        if s > u:
            return m
    for m in range(len(p) - 1, -1, -1):
        if p[m] > 0:
            return m
    raise RuntimeError("this shouldn't be possible.")


def root_value(r):                                                # mcts.h:78-100
    q, d, found = f32(0.0), f32(0.0), False
    for i in range(r.k):
        if r.n[i] > 0 and r.q[i] > q:
            q, d, found = r.q[i], r.d[i], True
    if not found and r.root_n > 0:
        q, d = r.root_v, r.root_d
    w = f32(q - f32(d / f32(r.P)))
    lose = f32(1.0 - float(w) - float(d))                         # in double, then to float
    return np.array([w, lose, d], np.float32)


def normalized_root_entropy(r):                                   # mcts.cc:737-750
    k = f32(r.k)
    if k <= 1 or r.root_n <= 1:
        return f32(0.0)
    log_k = _log(k)
    entropy = f32(0.0)
    total_n = f32(r.root_n)
    for i in range(r.k):
        if r.n[i] > 0:
            p = f32(f32(r.n[i]) / total_n)
            entropy = f32(entropy - f32(p * _log(p)))
    return f32(entropy / log_k)


def same_bits(a, b):
    """equality of float32 vectors bit for bit; entries that are NaN on both sides only need to be NaN on both sides"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- scripted sharp evaluators ------------------------------------------------------------------------------------
# What a trained net gives and a uniform evaluator never does: almost all mass on one move, legal moves at exactly 0, mass on
# illegal moves (dropped by set_policy_normalized, mcts.cc:109-121), rows that do not sum to 1, denormal entries; decisive values.
POLICY_PATTERNS = ("one_hot", "peak_and_dust", "half_zero", "mass_on_illegal", "sums_to_3p7", "denormals")
VALUE_PATTERNS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.25, 0.25))


def _stable_hash(canonical):
    return int.from_bytes(hashlib.blake2b(np.ascontiguousarray(canonical, np.float32).tobytes(), digest_size=8).digest(), "little")


def sharp_eval(canonical, valid, policy_pattern=None, value_pattern=None):
    """(value [3], pi [M]) for a leaf with two players: a pure function of the canonical array and the legal-move mask.  A
    stable hash of the canonical bytes picks the patterns (or the caller does).  For a game with relative values the value
    row is read relative to the leaf's player, like any evaluator's."""
    valid = np.asarray(valid).astype(bool)
    M = valid.size
    legal = np.flatnonzero(valid)
    illegal = np.flatnonzero(~valid)
    assert legal.size > 0, "the scripted evaluator is asked about a position without moves"
    h = _stable_hash(canonical)
    pp = POLICY_PATTERNS[h % len(POLICY_PATTERNS)] if policy_pattern is None else policy_pattern
    vp = (h >> 8) % len(VALUE_PATTERNS) if value_pattern is None else value_pattern
    star = int(legal[(h >> 16) % legal.size])
    pi = np.zeros(M, np.float32)
    if pp == "one_hot":
        pi[star] = 1.0
    elif pp == "peak_and_dust":
        pi[legal] = 1e-30
        pi[star] = 0.999
    elif pp == "half_zero":                          # every other legal move (the star's parity) at exactly 0
        j0 = int(np.flatnonzero(legal == star)[0])
        keep = legal[(np.arange(legal.size) - j0) % 2 == 0]
        pi[keep] = f32(1.0) / f32(keep.size)
    elif pp == "mass_on_illegal":                    # without an illegal move the row is the legal tenth alone
        if illegal.size:
            pi[illegal] = f32(0.9) / f32(illegal.size)
        pi[legal] = f32(0.1) / f32(legal.size)
    elif pp == "sums_to_3p7":
        w = (1 + np.arange(legal.size) % 3).astype(np.float64)
        pi[legal] = (3.7 * w / w.sum()).astype(np.float32)
    elif pp == "denormals":
        pi[legal] = (1e-40 * (1 + np.arange(legal.size) % 4)).astype(np.float32)
        pi[star] = 0.5
    else:
        raise ValueError(pp)
    assert float(pi[legal].astype(np.float64).sum()) > 0.0, "an all-zero row over the legal moves gives NaN priors: out of scope"
    return np.array(VALUE_PATTERNS[vp], np.float32), pi


def legal_mask(game, canonical, oracle):
    """the legal-move mask of a position given as its canonical array (an engine's evaluator sees nothing else): Connect4 - the
    columns that are not full; Brandubh - valid_moves() is a function of the board and the player to move, both in the planes"""
    canonical = np.asarray(canonical)
    if game == "connect4":
        return ((canonical[0] + canonical[1]).sum(0) < 6).astype(np.uint8)
    if game == "brandubh":
        player = 0 if canonical[3, 0, 0] == 1 else 1
        return oracle.Game.tafl_from_board(oracle.GAME_BRANDUBH, canonical[:3].astype(np.int8), player, max_turns=150).valid()
    raise ValueError(game)


def sharp_evaluator(game, oracle):
    """evaluator(canonical [n, C, H, W]) -> (v [n, 3], pi [n, M]) for build_batch / update_inferences and the oracle's
    PlayManager.run: sharp_eval of every row, memoised by the canonical bytes"""
    memo = {}

    def evaluator(canon):
        V, PI = [], []
        for c in canon:
            key = c.tobytes()
            if key not in memo:
                memo[key] = sharp_eval(c, legal_mask(game, c, oracle))
            V.append(memo[key][0]); PI.append(memo[key][1])
        return np.stack(V), np.stack(PI)

    return evaluator
