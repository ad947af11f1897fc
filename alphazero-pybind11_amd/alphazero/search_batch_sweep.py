"""MCTSBatch's visit sweep (azmi_search_run_to / _checkpoints / _sweep_metrics, azmi_policy_divergences; the host's
search_batch_sweep.hip): the methods of `_Sweep`, which MCTSBatch (search_batch.py) is built on, and policy_divergences.

A visit sweep (mcts_analysis.py:884-972): search_to(targets, ..., checkpoints=(c0, c1, ...)) searches tree i until
root_n(i) >= targets[i] and records counts / probs / root_values / root_q_values on the device the first time root_n(i)
reaches each checkpoint; checkpoints() returns the snapshots.  See search_to().  sweep_metrics(anchor, raw, reference,
outcomes) scores every snapshot against the anchor one on the device (:1150-1400): divergences, top-k agreement, expected
reward and regret, the signal figures against the one-visit policy, the value gaps, and their per-checkpoint means."""
import numpy as np

from . import _args
from ._capi import lib, check
from .mcts import _ENGINE_STREAM

POLICY_COLUMNS = ("jsd", "tv", "hellinger", "top1", "top3", "top9")
SWEEP_COLUMNS = POLICY_COLUMNS + ("reward", "regret", "pressure", "benefit", "entropy", "value_gap", "abs_err", "closer_than_anchor",
                                  "closer_than_raw")      # the column order of azmi_search_sweep_metrics


def policy_divergences(p, q, device=0):
    """The six policy figures of policy_metrics.py for every row of two [rows, M] policy arrays, on the device
    (azmi_policy_divergences), in float64 from the float32 inputs: jsd, tv, hellinger and top1 / top3 / top9 =
    |top_k(p) & top_k(q)| / k.  top_k(x) is np.argsort(x, kind="stable")[-k:] - among equal values the higher index ranks
    higher; with M < k every index is in both sets and the divisor stays k.  A pair of one-dimensional arrays is one row.
    -> dict of six float64 [rows] arrays.  rows == 0 touches no device."""
    try:
        a = np.asarray(p, dtype=np.float32)
        b = np.asarray(q, dtype=np.float32)
    except (TypeError, ValueError):
        raise RuntimeError("policy_divergences: p and q must be arrays of numbers") from None
    if a.ndim == 1 and b.ndim == 1:
        a, b = a[None, :], b[None, :]
    if a.ndim != 2 or b.ndim != 2:
        raise RuntimeError(f"policy_divergences: p and q must be [rows, M] arrays, got shapes {a.shape} and {b.shape}")
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        raise RuntimeError(f"policy_divergences: p and q must have one shape, got {a.shape} and {b.shape}")
    rows, M = a.shape
    if M < 1 or M > 1 << 20:
        raise RuntimeError(f"policy_divergences: M must be in [1, 2^20], got {M}")
    if rows > 1 << 30:
        raise RuntimeError(f"policy_divergences: at most 2^30 rows, got {rows}")
    device = _args.device_index(device, "policy_divergences")
    out = np.zeros((rows, len(POLICY_COLUMNS)), np.float64)
    check(lib.azmi_policy_divergences(a.ctypes.data if rows else None, b.ctypes.data if rows else None, rows, M,
                                      out.ctypes.data if rows else None, device, None))
    return {k: out[:, c].copy() for c, k in enumerate(POLICY_COLUMNS)}


class _Sweep:
    """search_to, checkpoints and sweep_metrics of MCTSBatch, the one class built on this one: the fields are those of
    MCTSBatch.__init__, and _evaluator / _one_descent_per_step are found on it."""

    def search_to(self, targets, net=None, cache=None, root_noise=False, evaluator=None, checkpoints=None, temp=1.0, pruned=False):
        """Search every tree to its own visit target: tree i descends while root_n(i) < targets[i] (`targets`: an int or n
        integers) - the `while mcts.root_n() < target` loop of mcts_analysis.py:884-972.  A tree at or above its target (a root
        reused by update_roots() already holds visits) and a finished tree take no descent.  net / cache / root_noise /
        evaluator are search()'s.  With leaves_per_step = K every step is K descents of every tree still below its target, so
        a tree may overshoot by fewer than K (mcts_analysis.py:982-1058).
        `checkpoints`: None, or at most 32 strictly ascending positive visit counts.  Snapshot j of tree i is taken once, on the
        device, at the first step boundary at which root_n(i) >= checkpoints[j] - before the first descent for a tree that
        starts there; a checkpoint above the tree's target is never taken.  checkpoints() returns the snapshots; every
        search_to starts a fresh set.  `temp`, `pruned`: the snapshots hold probs(temp), or probs_pruned(temp).
        The call reads root_n once, then enqueues every step without reading anything back; the budget is checked for the
        longest tree's steps x K before anything is enqueued.  A Gumbel batch raises: use search(visits)."""
        self._one_descent_per_step("search_to", "the checkpoint launches are planned from one root_n read and one descent of "
                                   "every tree per step")
        ev = self._evaluator("search_to", evaluator, net, cache)
        if net is not None and (net.desc.num_moves != self._M or (net.desc.in_channels, net.desc.height, net.desc.width) != self._chw):
            raise RuntimeError("search_to: the net's shape does not match the game")
        if self._gumbel:
            raise RuntimeError("search_to on a Gumbel batch: sequential halving plans a fixed budget at its first descent, and a "
                               "root_n target on a reused tree is not one; use search(visits)")
        tg = [int(targets)] * self._n if np.ndim(targets) == 0 else [int(x) for x in targets]
        if len(tg) != self._n:
            raise RuntimeError(f"search_to: one target per tree ({self._n}), got {len(tg)}")
        if any(x < 0 or x > 0xFFFFFFFF for x in tg):
            raise RuntimeError("search_to: targets must be visit counts in [0, 2^32)")
        cp = [] if checkpoints is None else [int(x) for x in checkpoints]
        if len(cp) > 32:
            raise RuntimeError(f"search_to: at most 32 checkpoints, got {len(cp)}")
        if any(x <= 0 or x > 0xFFFFFFFF for x in cp) or any(b <= a for a, b in zip(cp, cp[1:])):
            raise RuntimeError(f"search_to: checkpoints must be positive and strictly ascending, got {cp}")
        if cache is not None:
            cache._ensure_engine_layout()
        tga, cpa = np.ascontiguousarray(tg, dtype=np.uint32), np.ascontiguousarray(cp, dtype=np.uint32)
        check(lib.azmi_search_run_to(self._h, int(ev), None if net is None else net._h, None if cache is None else cache._h,
                                     tga.ctypes.data, cpa.ctypes.data if cp else None, len(cp), float(temp), int(bool(pruned)),
                                     int(bool(root_noise)), _ENGINE_STREAM))
        self._sweep_j = len(cp)

    def checkpoints(self):
        """The snapshots of the last search_to(), one row per tree and checkpoint, as recorded on the device at snapshot time:
        taken bool [n, J], root_n uint32 [n, J], counts uint32 [n, J, M], probs float32 [n, J, M] (probs(temp), or
        probs_pruned(temp) with pruned=True), root_values float32 [n, J, 3], root_q_values float32 [n, J, M].  Rows that were
        not taken are zero.  Synchronises."""
        J = getattr(self, "_sweep_j", None)
        if J is None:
            raise RuntimeError("checkpoints: no search_to call has been made on this batch")
        n, M = self._n, self._M
        mask = np.zeros(n, np.uint32)
        out = dict(root_n=np.zeros((n, J), np.uint32), counts=np.zeros((n, J, M), np.uint32), probs=np.zeros((n, J, M), np.float32),
                   root_values=np.zeros((n, J, 3), np.float32), root_q_values=np.zeros((n, J, M), np.float32))
        check(lib.azmi_search_checkpoints(self._h, mask.ctypes.data, out["root_n"].ctypes.data, out["counts"].ctypes.data,
                                          out["probs"].ctypes.data, out["root_values"].ctypes.data, out["root_q_values"].ctypes.data))
        out["taken"] = ((mask[:, None] >> np.arange(J, dtype=np.uint32)[None, :]) & 1).astype(bool)
        return out

    @staticmethod
    def _sweep_index(what, x, J):
        """-> x as a checkpoint index of a set of J, negative values counting from its end"""
        x = _args.integer(x, f"sweep_metrics: {what} must be a checkpoint index (an integer), got {x!r}")
        if not -J <= x < J:
            raise RuntimeError(f"sweep_metrics: {what} = {x} out of range: the reference set has {J} checkpoints")
        return x % J

    def _sweep_args(self, anchor, raw, reference, outcomes):
        """-> (reference batch, anchor, raw or -1, outcomes float64 [n] or None); every argument error before any device call"""
        J = getattr(self, "_sweep_j", None)
        if J is None:
            raise RuntimeError("sweep_metrics: no search_to call has been made on this batch")
        if getattr(self, "_rows", None) is not None:
            raise RuntimeError("sweep_metrics: a find_leaves step is pending; call process_results first")
        ref = self if reference is None else reference
        if not isinstance(ref, _Sweep):
            raise RuntimeError(f"sweep_metrics: reference must be an MCTSBatch or None, got {type(reference).__name__}")
        if ref is not self:
            if getattr(ref._game, "GAME_ID", None) != getattr(self._game, "GAME_ID", None):
                raise RuntimeError(f"sweep_metrics: the reference batch holds another game ({ref._game.__name__}, "
                                   f"this batch {self._game.__name__})")
            if ref._n != self._n:
                raise RuntimeError(f"sweep_metrics: the reference batch holds {ref._n} trees, this batch {self._n}")
            if ref._device != self._device:
                raise RuntimeError(f"sweep_metrics: the reference batch is on device {ref._device}, this batch on {self._device}")
            if getattr(ref, "_sweep_j", None) is None:
                raise RuntimeError("sweep_metrics: no search_to call has been made on the reference batch")
            if getattr(ref, "_rows", None) is not None:
                raise RuntimeError("sweep_metrics: a find_leaves step is pending on the reference batch; call process_results first")
        Jr = ref._sweep_j
        if Jr == 0:
            raise RuntimeError("sweep_metrics: the reference set has no checkpoints: nothing to anchor on")
        a = self._sweep_index("anchor", anchor, Jr)
        r = -1 if raw is None else self._sweep_index("raw", raw, Jr)
        o = None
        if outcomes is not None:
            try:
                o = np.ascontiguousarray(outcomes, dtype=np.float64)
            except (TypeError, ValueError):
                raise RuntimeError(f"sweep_metrics: outcomes must be {self._n} numbers, got {outcomes!r}") from None
            if o.shape != (self._n,):
                raise RuntimeError(f"sweep_metrics: outcomes: one per tree ({self._n}), got shape {o.shape}")
        return ref, a, r, o

    def sweep_metrics(self, anchor=-1, raw=None, reference=None, outcomes=None):
        """Score every snapshot of the last search_to() against the anchor snapshot of the same tree, on the device
        (azmi_search_sweep_metrics): what mcts_analysis.run_analysis does with its sweep once the search is over
        (mcts_analysis.py:1150-1400), without copying the [n, J, M] snapshots out.  `reference`: the batch whose snapshot set
        supplies the anchor row, the raw row and root_q_values (default: this batch; the reference's `base_ref` tree when the
        swept trees search with root noise) - same game, n and device.  `anchor`, `raw`: checkpoint indices into the
        reference's set, negative ones counting from its end; raw (None: none) is the one-visit checkpoint the "signal"
        figures compare against.  `outcomes`: None or n game outcomes.
        With p the anchor policy, q the policy of row (i, j), r the raw policy, Q the anchor's root_q_values and v =
        root_values[..., 0], all float32 snapshots computed with in float64:
          jsd, tv, hellinger, top1, top3, top9    policy_divergences(p, q)
          reward = sum q Q, regret = reward(anchor row) - reward
          pressure = KL(q || r + 1e-10), benefit = reward - sum r Q, entropy = -sum q ln q         (pressure, benefit: need raw)
          value_gap = |v_j - v_anchor|
          abs_err = |v_j - outcome|, closer_than_anchor, closer_than_raw (1.0 / 0.0)               (need outcomes; the last, raw)
          ceiling[i] = KL(p || r + 1e-10)                                                          (needs raw)
        A row is valid when snapshot j of tree i and the reference's anchor snapshot of tree i were both taken; an invalid row
        is NaN everywhere, and what needs a raw row or outcomes that are not there is NaN.
        -> dict: one float64 [n, J] array per name above, ceiling [n], valid bool [n, J], and mean / count: dicts of [J] arrays,
        per column the mean over the trees that are not NaN there and their number.  Two launches and one synchronisation
        whatever n and J are; the sums run in a fixed order, so two calls give the same bits.  Correlations and calibration
        bins (mcts_analysis.py:1289-1353) are a few numpy lines over the returned arrays."""
        ref, a, r, o = self._sweep_args(anchor, raw, reference, outcomes)
        n, J, C_ = self._n, self._sweep_j, len(SWEEP_COLUMNS)
        rows = np.zeros((n, J, C_), np.float64); ceiling = np.zeros(n, np.float64)
        mean = np.zeros((J, C_), np.float64); count = np.zeros((J, C_), np.uint32); valid = np.zeros((n, J), np.uint8)
        check(lib.azmi_search_sweep_metrics(self._h, None if ref is self else ref._h, a, r, None if o is None else o.ctypes.data,
                                            rows.ctypes.data, ceiling.ctypes.data, mean.ctypes.data, count.ctypes.data,
                                            valid.ctypes.data, _ENGINE_STREAM))
        out = {k: rows[:, :, c].copy() for c, k in enumerate(SWEEP_COLUMNS)}
        out.update(ceiling=ceiling, valid=valid.astype(bool),
                   mean={k: mean[:, c].copy() for c, k in enumerate(SWEEP_COLUMNS)},
                   count={k: count[:, c].astype(np.int64) for c, k in enumerate(SWEEP_COLUMNS)})
        return out
