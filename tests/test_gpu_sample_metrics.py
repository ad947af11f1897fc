"""-m gpu: the per-row policy and value diagnostics on the device - azmi_sample_metrics, azmi_sample_plane_argmax,
azmi_sample_metrics_reduce and the functions of alphazero.samples built on them (sample_metrics, plane_argmax, eval_metrics,
analyze_samples), up to selfplay.analyze_iteration.  The yardstick is a numpy float64 restatement of the column table, written here
from the formulas (network_pareto.py:694-716, game_runner.py:2560-2581), with the tie rule stated there: the lower index wins
(np.argmax, the first three of a stable argsort of -x).

The generated rows are tie-free in their three largest targets and three largest probabilities wherever those are positive; the
edge rows the cases must hold (all-zero targets, one-hot targets, zeroed entries, p = 0) tie at zero by construction, and the
stated rule decides them - the restatement applies it, so every index is compared exactly there too."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLT_MIN = float(np.finfo(np.float32).tiny)
SUMS = ("pi_loss", "v_loss", "target_entropy", "entropy", "kl")
EXACT = ("top1", "net_top1", "net_at_mcts", "top1_gap", "top1_agree", "top3_overlap", "v_pred", "v_actual")
COLUMNS = SUMS[:1] + SUMS[1:2] + SUMS[2:] + EXACT


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


def _block():
    """kPlanBlock, from the kernel header"""
    header = open(os.path.join(ROOT, "alphazero-pybind11_amd", "csrc", "samples_kernels.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+kPlanBlock\s*=\s*(\d+)\s*;", header).group(1))


BLOCK = _block()


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _top3(x):
    """the first three of a stable argsort of -x, per row (NaN-free rows)"""
    return np.argsort(-x, axis=1, kind="stable")[:, :3]


def _restate(t, p, tv, pv, cv=1.0):
    """the column table in numpy float64 -> {column: [n]}, plus "entropy_abs" / "kl_abs" (the sums of |term| the bounds need)"""
    t64, p64, tv64, pv64 = (x.astype(np.float64) for x in (t, p, tv, pv))
    n, M = t.shape
    pos = t64 > 0
    safe_t = np.where(pos, t64, 1.0)
    with np.errstate(all="ignore"):
        pi_terms = np.where(pos, t64 * np.log(np.maximum(p64, FLT_MIN)), 0.0)
        te_terms = np.where(pos, t64 * np.log(safe_t), 0.0)
        en_terms = t64 * np.log(t64 + 1e-9)
        kl_terms = np.where(pos, t64 * np.log(safe_t / (p64 + 1e-10)), 0.0)
        v_terms = np.where(tv64 > 0, tv64 * np.log(np.maximum(pv64, FLT_MIN)), 0.0)
    neg = np.where((t64 < 0).any(axis=1), np.nan, 0.0)
    out = {"pi_loss": -np.sum(pi_terms, axis=1) + neg, "target_entropy": -np.sum(te_terms, axis=1) + neg,
           "entropy": -np.sum(en_terms, axis=1) + neg, "kl": np.sum(kl_terms, axis=1) + neg,
           "v_loss": -cv * np.sum(v_terms, axis=1) + np.where((tv64 < 0).any(axis=1), np.nan, 0.0),
           "entropy_abs": np.sum(np.abs(en_terms), axis=1), "kl_abs": np.sum(np.abs(kl_terms), axis=1)}
    rows = np.arange(n)
    clean_t, clean_p = np.where(np.isnan(t), -np.inf, t), np.where(np.isnan(p), -np.inf, p)      # (indices of NaN rows: unspecified)
    mcts, net = np.argmax(clean_t, axis=1), np.argmax(clean_p, axis=1)
    out["mcts_argmax"], out["net_argmax"] = mcts.astype(np.uint32), net.astype(np.uint32)
    out["top1"], out["net_top1"] = t.max(axis=1).astype(np.float64), p.max(axis=1).astype(np.float64)      # (np.max hands a NaN on)
    out["net_at_mcts"] = p64[rows, mcts]
    out["top1_gap"] = out["top1"] - out["net_at_mcts"]
    out["top1_agree"] = (mcts == net).astype(np.float64)
    tt, tp = _top3(clean_t), _top3(clean_p)
    out["top3_overlap"] = np.array([len(set(tt[i]) & set(tp[i])) for i in range(n)], np.float64)
    out["v_pred"], out["v_actual"] = pv64[:, 0], tv64[:, 0]
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else x.dtype)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- columns ---------------------------------------------------------------------------------------------------------------------
METRIC_M = (1, 2, 3, 4, 7, 8, 9, 63, 64, 65, 1000)
METRIC_V = (1, 3)
METRIC_N = (1, 2, 257)


def _assert_tie_free(x, what):
    """the three largest entries of every row are distinct wherever they are positive (ties at zero: the edge rows, see the docstring)"""
    top = -np.sort(-x, axis=1)[:, :3]
    for k in range(top.shape[1] - 1):
        tied = (top[:, k] == top[:, k + 1]) & (top[:, k] > 0)
        assert not tied.any(), f"{what}: row {int(np.argmax(tied))} ties in its three largest entries"
    if x.shape[1] > 3:      # the third is also clear of the fourth: the SET of three is decided by value
        rest = -np.sort(-x, axis=1)[:, 3]
        tied = (top[:, 2] == rest) & (rest > 0)
        assert not tied.any(), f"{what}: row {int(np.argmax(tied))} ties at the edge of its top three"


def _case(M, V, n):
    """_loss_case of test_gpu_samples.py for the policy rows (zeroed targets, p = 0 under a positive and under a zero target, all-zero
    rows, one-hot rows) and random value rows with a zeroed entry and a p = 0 now and then"""
    rng = np.random.default_rng(100000 * V + 1000 * M + n)
    t = rng.random((n, M)).astype(np.float32)
    t[rng.random((n, M)) < 0.3] = 0.0
    t[:, 0] = np.maximum(t[:, 0], np.float32(0.01))
    t /= t.sum(axis=1, keepdims=True)
    p = rng.random((n, M)).astype(np.float32) + np.float32(1e-6)
    p /= p.sum(axis=1, keepdims=True)
    for r in range(0, n, 16):
        p[r, 0] = 0.0
        if M > 1:
            t[r, 1] = 0.0
            p[r, 1] = 0.0
    for r in range(1, n, 16):
        t[r] = 0.0
        p[r, M - 1] = 0.0
    for r in range(2, n, 16):
        t[r] = 0.0
        t[r, (r * 7) % M] = 1.0
    tv = rng.random((n, V)).astype(np.float32)
    tv[rng.random((n, V)) < 0.3] = 0.0
    tv /= np.maximum(tv.sum(axis=1, keepdims=True), np.float32(1e-3))
    pv = rng.random((n, V)).astype(np.float32) + np.float32(1e-6)
    pv /= pv.sum(axis=1, keepdims=True)
    pv[3::16, V - 1] = 0.0
    _assert_tie_free(t, f"targets M = {M}, n = {n}")
    _assert_tie_free(p, f"probabilities M = {M}, n = {n}")
    return t, p, tv, pv


def _assert_columns(az, got, t, p, tv, pv, cv, label):
    n, M = t.shape
    want = _restate(t, p, tv, pv, cv)
    for name in COLUMNS:
        assert got[name].dtype == np.float64 and got[name].shape == (n,), name
    for name in ("mcts_argmax", "net_argmax"):
        assert got[name].dtype == np.uint32 and np.array_equal(got[name], want[name]), name
    # the two losses are k_sample_loss's, bit for bit
    assert np.array_equal(got["pi_loss"], az.sample_loss(t, p))
    assert np.array_equal(got["v_loss"], az.sample_loss(tv, pv, scale=cv))
    ulp = 2.0 ** -52
    err = np.abs(got["target_entropy"] - want["target_entropy"])
    bound = (M + 2) * ulp * np.abs(want["target_entropy"])      # every term has one sign
    print(f"{label}: target_entropy largest error {float(err.max()):.3e}, bound there {float(bound[np.argmax(err)]):.3e}")
    assert (err <= bound).all()
    for name in ("entropy", "kl"):
        err = np.abs(got[name] - want[name])
        bound = (M + 4) * ulp * want[name + "_abs"]      # one ulp each for the log, the sum / quotient inside it, the product; M for the additions
        k = int(np.argmax(err / np.maximum(bound, 1e-300)))
        print(f"{label}: {name} largest error {float(err.max()):.3e}, the error nearest its bound {float(err[k]):.3e} of {float(bound[k]):.3e}")
        assert (err <= bound).all(), name
    for name in EXACT:
        assert np.array_equal(got[name], want[name]), name
    return want


@pytest.mark.parametrize("n", METRIC_N)
@pytest.mark.parametrize("V", METRIC_V)
@pytest.mark.parametrize("M", METRIC_M)
def test_sample_metrics_columns_are_the_restatement(az, M, V, n):
    t, p, tv, pv = _case(M, V, n)
    cv = 1.5
    got = az.sample_metrics(t, p, tv, pv, cv=cv)
    assert tuple(got) == az.samples.METRIC_COLUMNS + az.samples.INDEX_COLUMNS
    _assert_columns(az, got, t, p, tv, pv, cv, f"M = {M}, V = {V}, n = {n}")
    if n > 1:
        assert got["pi_loss"][1] == 0.0 and got["target_entropy"][1] == 0.0 and got["kl"][1] == 0.0 and got["entropy"][1] == 0.0      # all-zero targets
    if n == 257:
        # a row does not depend on n or on the launch geometry: the same rows alone give the same bits
        for sl in (slice(0, 5), slice(250, 257)):
            alone = az.sample_metrics(t[sl].copy(), p[sl].copy(), tv[sl].copy(), pv[sl].copy(), cv=cv)
            for name in got:
                assert _same_bits(alone[name], got[name][sl]), (name, sl)


@pytest.mark.parametrize("M,V", [(7, 3), (65, 1), (3, 100)])
def test_sample_metrics_on_cuda_tensors_is_the_staged_result(az, M, V):
    """(3, 100): the value row's lane group is wider than the policy row's"""
    import torch
    t, p, tv, pv = _case(M, V, 257)
    dev = torch.device("cuda", 0)
    staged = az.sample_metrics(t, p, tv, pv, cv=2.0)
    _assert_columns(az, staged, t, p, tv, pv, 2.0, f"M = {M}, V = {V}")
    got = az.sample_metrics(*(torch.from_numpy(x).to(dev) for x in (t, p, tv, pv)), cv=2.0)
    for name, x in got.items():
        assert x.is_cuda and x.dtype == (torch.int32 if name.endswith("argmax") else torch.float64)
        host = x.cpu().numpy()
        assert _same_bits(host.view(np.uint32) if name.endswith("argmax") else host, staged[name]), name


# ---- ties ------------------------------------------------------------------------------------------------------------------------
def _tie_rows(M):
    rng = np.random.default_rng(77 + M)
    distinct = lambda: (rng.permutation(M) + 1).astype(np.float32) / np.float32(M * (M + 1) / 2)
    rows = [(np.full(M, 1.0 / M, np.float32), distinct()),                      # a uniform target
            (distinct(), np.full(M, 1.0 / M, np.float32)),                      # equal maxima in p: all of them
            (np.zeros(M, np.float32), np.zeros(M, np.float32))]                 # everything tied at zero
    if M >= 2:
        a, b = sorted(rng.choice(M, 2, replace=False))
        t = np.zeros(M, np.float32)
        t[a] = t[b] = 0.5                                                       # two legal moves, the rest zero
        rows.append((t, distinct()))
        q = distinct() * np.float32(0.25)
        q[a] = q[b] = 0.5                                                       # two equal maxima in p, elsewhere than the lowest index
        rows.append((distinct(), q))
        rows.append((t, q))
        rows.append((t[::-1].copy(), q))
    t, p = (np.stack(x) for x in zip(*rows))
    tv = np.tile(np.array([[0.5, 0.5, 0.0]], np.float32), (len(rows), 1))
    return t, p, tv, tv.copy()


@pytest.mark.parametrize("M", (1, 2, 4, 7))
def test_ties_go_to_the_lower_index(az, M):
    t, p, tv, pv = _tie_rows(M)
    got = az.sample_metrics(t, p, tv, pv)
    # the rule, restated here: np.argmax, and the first three (M < 3: all M) of a stable argsort of -x
    mcts, net = np.argmax(t, axis=1), np.argmax(p, axis=1)
    tt, tp = np.argsort(-t, axis=1, kind="stable")[:, :3], np.argsort(-p, axis=1, kind="stable")[:, :3]
    assert tt.shape[1] == min(3, M)
    overlap = np.array([len(set(a) & set(b)) for a, b in zip(tt, tp)], np.float64)
    print(f"M = {M}: mcts_argmax {got['mcts_argmax'].tolist()} want {mcts.tolist()}, net_argmax {got['net_argmax'].tolist()} want {net.tolist()}, "
          f"top3_overlap {got['top3_overlap'].tolist()} want {overlap.tolist()}")
    assert np.array_equal(got["mcts_argmax"], mcts) and np.array_equal(got["net_argmax"], net)
    assert np.array_equal(got["top3_overlap"], overlap)
    assert np.array_equal(got["top1_agree"], (mcts == net).astype(np.float64))
    assert np.array_equal(got["net_at_mcts"], p[np.arange(len(t)), mcts].astype(np.float64))
    assert got["mcts_argmax"][0] == 0 and got["net_argmax"][1] == 0 and got["top3_overlap"][2] == min(3, M)      # uniform rows: index 0; all tied: {0, 1, 2}
    _assert_columns(az, got, t, p, tv, pv, 1.0, f"ties, M = {M}")


# ---- special values --------------------------------------------------------------------------------------------------------------
def test_a_negative_target_and_a_nan_probability_mark_their_own_row_only(az):
    """ordinary float inputs: a negative target makes the sums of its row NaN, a NaN probability what reads it"""
    import torch
    M, V, n = 7, 3, 40
    t, p, tv, pv = _case(M, V, n)
    base = az.sample_metrics(t, p, tv, pv, cv=1.5)
    t2, p2, tv2, pv2 = (x.copy() for x in (t, p, tv, pv))
    t2[5, 2] = -0.25                                   # a negative policy target
    top9 = int(np.argmax(t[9]))
    assert t[9, top9] > 0
    p2[9, top9] = np.nan                               # a NaN probability under the largest (positive) target
    spare = int(np.argmin(t[12] + (np.arange(M) == np.argmax(t[12]))))
    t2[12, spare] = 0.0
    p2[12, spare] = np.nan                             # a NaN probability under a zero target, away from the target's argmax
    tv2[20, 1] = -0.5                                  # a negative value target
    pv2[25, 2] = np.nan
    tv2[25] = (0.5, 0.25, 0.25)                        # a NaN value probability under a positive target
    expected = {5: {"pi_loss", "target_entropy", "entropy", "kl"}, 9: {"pi_loss", "kl", "net_top1", "net_at_mcts", "top1_gap"},
                12: {"net_top1"}, 20: {"v_loss"}, 25: {"v_loss"}}
    dev = torch.device("cuda", 0)
    for kind in ("numpy", "torch"):
        if kind == "numpy":
            got = az.sample_metrics(t2, p2, tv2, pv2, cv=1.5)
        else:
            got = {k: x.cpu().numpy() for k, x in az.sample_metrics(*(torch.from_numpy(x).to(dev) for x in (t2, p2, tv2, pv2)), cv=1.5).items()}
            got = {k: x.view(np.uint32) if k.endswith("argmax") else x for k, x in got.items()}
        for row in range(n):
            nan_columns = {name for name in COLUMNS if np.isnan(got[name][row])}
            assert nan_columns == expected.get(row, set()), (kind, row, nan_columns)
            if row not in expected:
                for name in got:      # the neighbours keep their bits
                    assert _bits(got[name])[row] == _bits(base[name])[row], (kind, row, name)
        for name in ("mcts_argmax", "net_argmax"):
            assert (got[name] < M).all(), name
    # the reduction names such a row
    cols = torch.from_numpy(np.stack([got[name] for name in az.samples.METRIC_COLUMNS])).to(dev)
    rec = _reduce(az, cols, None, 1)
    assert rec.nonfinite == 4 and rec.first_nonfinite == 5      # rows 5, 9, 20, 25 (row 12's NaN is not in a checked column)


# ---- reduction -------------------------------------------------------------------------------------------------------------------
REDUCE_N = (1, 2, BLOCK, BLOCK + 1, BLOCK * BLOCK + 1)
NCOL = 13


def _reduce(az, cols, bucket, B, stream=None):
    import torch
    rec = az._capi.SampleMetricsRecordC()
    st = torch.cuda.current_stream(cols.device).cuda_stream if stream is None else stream
    rc = az.lib.azmi_sample_metrics_reduce(cols.data_ptr(), cols.shape[1], cols.shape[1], None if bucket is None else bucket.data_ptr(), B,
                                           C.byref(rec), 0, C.c_void_p(st))
    assert rc == 0, az.lib.azmi_samples_last_error().decode()
    return rec


def _record_arrays(rec):
    return np.array(rec.sum, np.float64), np.array(rec.total, np.float64), np.array(rec.count, np.int64)


_REDUCE_CACHE = {}


def _reduce_case(n):
    """the columns (mixed signs) and, per column, math.fsum over all rows - computed once per n"""
    if n not in _REDUCE_CACHE:
        x = np.random.default_rng(4242 + n).standard_normal((NCOL, n))
        _REDUCE_CACHE[n] = x
    return _REDUCE_CACHE[n]


@pytest.mark.parametrize("B", (1, 4, 8))
@pytest.mark.parametrize("n", REDUCE_N)
def test_reduce_is_the_bucketed_tree_sum(az, n, B):
    import torch
    assert NCOL == len(az.samples.Metric) and BLOCK == 1024, "REDUCE_N was chosen for tiles of 1024: BLOCK^2 + 1 needs the third level"
    dev = torch.device("cuda", 0)
    x = _reduce_case(n)
    empty = B - 2 if B > 1 else None                                     # one bucket is left empty
    ids = [b for b in range(B) if b != empty]
    bucket = np.asarray(ids, np.uint8)[np.random.default_rng(n + B).integers(0, len(ids), n)]
    cols, bt = torch.from_numpy(x).to(dev), torch.from_numpy(bucket).to(dev)
    rec = _reduce(az, cols, bt, B)
    sums, total, count = _record_arrays(rec)
    assert rec.nonfinite == 0 and rec.first_nonfinite == 0xFFFFFFFF and rec.invalid == 0
    assert np.array_equal(count[:B], np.bincount(bucket, minlength=B)) and (count[B:] == 0).all() and count.sum() == n      # exact
    if empty is not None:
        assert count[empty] == 0 and (sums[empty] == 0.0).all()
    worst = 0.0
    for b in list(range(B)) + [None]:
        rows = slice(None) if b is None else bucket == b
        got = total if b is None else sums[b]
        for c in range(NCOL):
            col = x[c][rows]
            want, scale = math.fsum(col.tolist()), float(np.abs(col).sum())      # (the scale of the bound needs no exact sum)
            assert abs(got[c] - want) <= n * 2.0 ** -53 * scale, (b, c, got[c], want)
            worst = max(worst, abs(got[c] - want) / scale if scale else 0.0)
    print(f"n = {n}, B = {B}: the largest |sum - fsum| / sum|x| is {worst:.3e}, bound {n * 2.0 ** -53:.3e}")
    # the same bits on a second run and on another stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    for other in (_reduce(az, cols, bt, B), _reduce(az, cols, bt, B, stream=side.cuda_stream)):
        assert bytes(other) == bytes(rec)
    # bucket b's sums are the one-bucket sums of the columns with the other rows zeroed, bit for bit; so is the overall sum
    whole = _reduce(az, cols, None, 1)
    assert _same_bits(_record_arrays(whole)[0][0], total) and _same_bits(_record_arrays(whole)[1], total) and whole.count[0] == n
    for b in ids:
        zeroed = torch.where((bt == b).unsqueeze(0), cols, torch.zeros((), dtype=torch.float64, device=dev)).contiguous()
        alone = _record_arrays(_reduce(az, zeroed, None, 1))[0][0]
        assert _same_bits(alone, sums[b]), b


def test_reduce_names_the_first_non_finite_row_and_counts_invalid_ids(az):
    import torch
    dev = torch.device("cuda", 0)
    n = 3000
    x = np.random.default_rng(5).standard_normal((NCOL, n))
    x[az.samples.Metric.KL, 2999] = np.inf
    x[az.samples.Metric.PI_LOSS, 1500] = np.nan
    x[az.samples.Metric.ENTROPY, 1500] = -np.inf          # one row, two columns: one row counted
    x[az.samples.Metric.TOP1, 7] = np.nan                 # not a checked column
    bucket = (np.arange(n) % 5).astype(np.uint8)          # ids 0..4 with B = 3: 3 and 4 are invalid
    rec = _reduce(az, torch.from_numpy(x).to(dev), torch.from_numpy(bucket).to(dev), 3)
    assert rec.nonfinite == 2 and rec.first_nonfinite == 1500
    assert rec.invalid == int((bucket >= 3).sum()) == 1200
    sums, total, count = _record_arrays(rec)
    assert count.tolist() == [600, 600, 600, 0, 0, 0, 0, 0]
    c = int(az.samples.Metric.V_LOSS)
    assert abs(total[c] - math.fsum(x[c])) <= n * 2.0 ** -53 * math.fsum(np.abs(x[c]))          # the overall sum holds the invalid rows
    assert abs(sums[1][c] - math.fsum(x[c][bucket == 1])) <= n * 2.0 ** -53 * math.fsum(np.abs(x[c][bucket == 1]))


# ---- plane_argmax ------------------------------------------------------------------------------------------------------------
def test_plane_argmax_reads_the_variant_planes(az):
    import torch
    rng = np.random.default_rng(36)
    n = 257
    c = rng.random((n, 36, 13, 13)).astype(np.float32)
    variant = rng.integers(0, 4, n)
    c[:, 32:36] = 0.0
    c[np.arange(n), 32 + variant] = 1.0                   # one-hot planes on the whole board
    c[100, 32:36] = 0.0                                   # all four planes zero: 0
    want = c[:, 32:36, 6, 6].argmax(1)
    assert want[100] == 0 and len(set(want.tolist())) == 4
    got = az.plane_argmax(c, 32, 4, 6, 6)
    assert got.dtype == np.uint8 and got.shape == (n,) and np.array_equal(got, want)
    assert np.array_equal(az.plane_argmax(c, 0, 16, 12, 12), c[:, 0:16, 12, 12].argmax(1))      # random planes, the last cell
    assert np.array_equal(az.plane_argmax(c, 20, 16, 0, 3), c[:, 20:36, 0, 3].argmax(1))        # up to the last plane
    assert (az.plane_argmax(c, 35, 1, 6, 6) == 0).all()                                          # n_planes = 1
    t = az.plane_argmax(torch.from_numpy(c).to(torch.device("cuda", 0)), 32, 4, 6, 6)
    assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), want)
    from alphazero import selfplay
    ids, names = selfplay.variant_buckets(az.StarGambitUnifiedGS, c)
    assert np.array_equal(ids, want) and tuple(names) == ("skirmish", "showdown", "clash", "battle")
    assert selfplay.variant_buckets(az.StarGambitUnifiedBattleGS(), c)[1] == names and selfplay.variant_buckets(az.Connect4GS, c) is None


# ---- end to end on Connect4 --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c4_net(az):
    import torch
    from alphazero import torch_net
    fx = np.load(os.path.join(HERE, "golden", "nn_connect4_6b64c.npz"))
    net = torch_net.LeafNet(torch_net.connect4_spec())
    net.load_state_dict({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")})
    return az.HipLeafNet(net.eval())


def _c4_params(az, games=8):
    params = az.PlayParams()
    params.games_to_play, params.concurrent_games, params.max_batch_size = games, games, games
    params.mcts_visits = [16, 16]; params.model_groups = [0, 0]; params.history_enabled = True
    return params


@pytest.fixture(scope="module")
def c4_samples(az, c4_net):
    """the samples of 32 short games, the net's own answers on them, and the restatement of both - computed once"""
    from alphazero import selfplay
    result, samples = selfplay.self_play(az.Connect4GS, _c4_params(az, 32), c4_net, engines=2)
    assert result.games == 32 and samples[0].shape[0] > 32 * 7
    raw_v, raw_pi = c4_net.process(samples[0])
    host = tuple(x.cpu().numpy() for x in samples)
    return samples, host, raw_v.cpu().numpy(), raw_pi.cpu().numpy()


def _eval_restated(ref, rows, n_all, cv, M, V):
    """the figures of eval_loss from the restated columns of `rows` -> ({key: value}, {key: absolute tolerance}).  A row's column is
    within its bound of the restatement, the float64 tree sum of n_all terms adds at most n_all * 2^-53 of the sum of |term|."""
    k = int(rows.sum())
    ulp, tree = 2.0 ** -52, n_all * 2.0 ** -53
    mean = lambda name: math.fsum(ref[name][rows]) / k
    want = {"pi_loss": mean("pi_loss"), "v_loss": mean("v_loss"), "target_entropy": mean("target_entropy"), "kl_div": mean("kl"),
            "top1_agree": float(ref["top1_agree"][rows].sum()) / k, "top3_agree": float(ref["top3_overlap"][rows].sum()) / (3 * k), "count": k}
    tol = {"pi_loss": ((M + 2) * ulp + tree) * abs(want["pi_loss"]), "v_loss": ((V + 2) * ulp + tree) * abs(want["v_loss"]),
           "target_entropy": ((M + 2) * ulp + tree) * abs(want["target_entropy"]),
           "kl_div": ((M + 4) * ulp + tree) * math.fsum(ref["kl_abs"][rows]) / k, "top1_agree": 0.0, "top3_agree": 0.0, "count": 0}
    want["v_loss_raw"], tol["v_loss_raw"] = want["v_loss"] / cv, tol["v_loss"] / cv + ulp * abs(want["v_loss"] / cv)
    want["total_loss"], tol["total_loss"] = want["v_loss"] + want["pi_loss"], tol["v_loss"] + tol["pi_loss"] + ulp * abs(want["v_loss"] + want["pi_loss"])
    want["kl_gap"] = want["pi_loss"] - want["target_entropy"]
    tol["kl_gap"] = tol["pi_loss"] + tol["target_entropy"] + ulp * abs(want["kl_gap"])
    return want, tol


def _assert_eval(got, want, tol, label):
    assert set(got) == set(want), label
    for key in want:
        print(f"{label}: {key} {got[key]!r} against {want[key]!r}, tolerance {tol[key]:.3e}")
        assert abs(got[key] - want[key]) <= tol[key], (label, key)


@pytest.mark.parametrize("kind", ("torch", "numpy"))
def test_eval_metrics_and_analyze_samples_on_connect4(az, c4_net, c4_samples, kind):
    import torch
    samples_t, samples_h, raw_v, raw_pi = c4_samples
    samples = samples_t if kind == "torch" else samples_h
    c, v, pi = samples_h
    n, M, V, cv = c.shape[0], pi.shape[1], v.shape[1], 1.5
    batch_rows = next(b for b in (61, 59, 53) if n % b)      # smaller than n and not dividing it
    assert batch_rows < n
    ref = _restate(pi, raw_pi, v, raw_v, cv)
    everything = np.ones(n, bool)
    got = az.eval_metrics(samples, c4_net, cv=cv, batch_rows=batch_rows)
    assert tuple(got) == az.samples.EVAL_KEYS
    _assert_eval(got, *_eval_restated(ref, everything, n, cv, M, V), f"{kind}, overall")
    # the two losses are iteration_losses' (the same rows through the same tree)
    v_loss, pi_loss = az.iteration_losses(samples, c4_net, cv=cv, batch_rows=batch_rows)
    print(f"iteration_losses: v {v_loss!r} against {got['v_loss']!r}, pi {pi_loss!r} against {got['pi_loss']!r}, {n} rows")
    assert abs(got["v_loss"] - v_loss) <= n * 2.0 ** -53 * abs(v_loss) and abs(got["pi_loss"] - pi_loss) <= n * 2.0 ** -53 * abs(pi_loss)
    assert az.eval_metrics(samples, c4_net, cv=cv) == got      # one chunk: the same rows, the same bits
    # two arbitrary buckets
    bucket_h = (np.arange(n) % 3 == 0).astype(np.uint8)
    bucket = torch.from_numpy(bucket_h).to(samples_t[0].device) if kind == "torch" else bucket_h
    split = az.eval_metrics(samples, c4_net, cv=cv, batch_rows=batch_rows, buckets=bucket, names=["rest", "third"])
    assert list(split) == ["rest", "third", "overall"] and split["rest"]["count"] + split["third"]["count"] == n
    assert split["overall"] == got
    for b, name in enumerate(("rest", "third")):
        _assert_eval(split[name], *_eval_restated(ref, bucket_h == b, n, cv, M, V), f"{kind}, bucket {name}")
    only = az.eval_metrics(samples, c4_net, cv=cv, buckets=bucket, n_buckets=3)      # an empty bucket is left out
    assert list(only) == ["0", "1", "overall"] and only["1"] == split["third"]
    # analyze_samples: the masked columns of sample_metrics on the net's own answers, bit for bit
    columns = az.sample_metrics(pi, raw_pi, v, raw_v, cv=cv)
    _assert_columns(az, columns, pi, raw_pi, v, raw_v, cv, f"{kind}, connect4")
    to_host = (lambda x: x.cpu().numpy()) if kind == "torch" else (lambda x: x)
    whole = az.analyze_samples(samples, c4_net, cv=cv, batch_rows=batch_rows)
    assert list(whole) == ["overall"] and tuple(whole["overall"]) == az.samples.ANALYSIS_KEYS
    for key, x in whole["overall"].items():
        assert (x.is_cuda if kind == "torch" else isinstance(x, np.ndarray)) and _same_bits(to_host(x), columns[key]), key
    parts = az.analyze_samples(samples, c4_net, cv=cv, batch_rows=batch_rows, buckets=bucket, names=["rest", "third"])
    assert list(parts) == ["rest", "third"]
    for b, name in enumerate(("rest", "third")):
        for key, x in parts[name].items():
            assert _same_bits(to_host(x), columns[key][bucket_h == b]), (name, key)
    from alphazero import selfplay
    again = selfplay.analyze_iteration(az.Connect4GS, samples, c4_net, cv=cv, batch_rows=batch_rows)      # not a unified game: one bucket
    assert list(again) == ["overall"] and all(_same_bits(to_host(again["overall"][k]), columns[k]) for k in columns if k in again["overall"])


def test_eval_metrics_raises_on_a_non_finite_loss_and_on_an_invalid_bucket(az, c4_net, c4_samples):
    samples_t = c4_samples[0]
    c, v, pi = (x.clone() for x in samples_t)
    pi[11, 3] = -0.5
    with pytest.raises(RuntimeError, match=r"eval_metrics: 1 of \d+ samples have a loss, entropy or kl that is not finite, the first at row 11 "):
        az.eval_metrics((c, v, pi), c4_net)
    import torch
    bucket = torch.full((c.shape[0],), 2, dtype=torch.uint8, device=c.device)
    with pytest.raises(RuntimeError, match=r"eval_metrics: \d+ of \d+ bucket ids are >= n_buckets = 2"):
        az.eval_metrics(samples_t, c4_net, buckets=bucket, n_buckets=2)


def test_analyze_iteration_splits_stargambit_samples_by_variant(az):
    """selfplay.analyze_iteration on the samples of four unified StarGambit games (the README's StarGambit snippet): the buckets are
    the variants read from the canonical planes on the host"""
    from alphazero import selfplay, torch_net
    params = az.PlayParams()
    params.games_to_play, params.concurrent_games, params.max_batch_size = 4, 4, 4
    params.mcts_visits = [12, 12]; params.model_groups = [0, 0]; params.history_enabled = True
    sg_net = az.HipLeafNet(torch_net.random_init(torch_net.stargambit_spec()), torch_net.stargambit_spec())
    game = az.StarGambitUnifiedGS(-1, [0.25] * 4)
    result, samples = selfplay.self_play(game, params, sg_net, engines=2)
    c = samples[0].cpu().numpy()
    n = c.shape[0]
    assert n > 0 and c.shape[1:] == (36, 13, 13)
    ids = c[:, 32:36, 6, 6].argmax(1)
    assert (c[:, 32:36, 6, 6].sum(axis=1) == 1.0).all()      # one-hot at the centre cell
    got = selfplay.analyze_iteration(game, samples, sg_net)
    names = ("skirmish", "showdown", "clash", "battle")
    assert list(got) == [names[b] for b in range(4) if (ids == b).any()]
    columns = {k: x.cpu().numpy() for k, x in az.sample_metrics(samples[2], sg_net.process(samples[0])[1], samples[1], sg_net.process(samples[0])[0]).items()}
    for b, name in enumerate(names):
        if name in got:
            assert all(x.shape == (int((ids == b).sum()),) for x in got[name].values()), name
            for key, x in got[name].items():
                assert _same_bits(x.cpu().numpy(), columns[key][ids == b]), (name, key)
    counts = {name: d["count"] for name, d in az.eval_metrics(samples, sg_net, buckets=selfplay.variant_buckets(game, samples[0])[0], names=names).items()}
    assert counts == dict({names[b]: int((ids == b).sum()) for b in range(4) if (ids == b).any()}, overall=n)


# ---- README ----------------------------------------------------------------------------------------------------------------------
def test_readme_metrics_example_runs_as_written(az, c4_net, tmp_path, monkeypatch):
    """the indented lines under the README's diagnostics paragraph, with the `params` and `net` of the README's earlier snippets"""
    readme = open(os.path.join(ROOT, "README.md")).read()
    block = re.search(r"The diagnostics of a net over those samples(?s:.*?)\n\n((?:    \S.*\n)+)", readme).group(1)
    lines = [ln[4:] for ln in block.splitlines()]
    assert len(lines) == 4 and "eval_metrics" in block and "analyze_iteration" in block and "plane_argmax" in block
    monkeypatch.chdir(tmp_path)
    from alphazero import selfplay
    scope = {"alphazero": az, "selfplay": selfplay, "params": _c4_params(az), "net": c4_net}
    exec("\n".join(lines), scope)
    assert scope["metrics"]["count"] == len(scope["samples"][0]) > 0 and 0 <= scope["metrics"]["top1_agree"] <= 1
    assert scope["by_cell"]["overall"] == scope["metrics"]
    assert len(scope["per_sample"]["overall"]["top1_gap"]) == scope["metrics"]["count"]
