"""CPU: the per-row diagnostics of alphazero.samples (sample_metrics, plane_argmax, eval_metrics, analyze_samples) and
selfplay.variant_buckets / analyze_iteration: the entry points are exported with the declared signatures, the C ABI and the Python
functions reject bad arguments by name before any device call, n == 0 returns empty or NaN results without a device, the package
still imports without torch, and the Python column enum is the header's.  The column table is restated here in numpy float64, from
the formulas, for the documentation's sake and to pin the tie rule the GPU file applies (the lower index wins)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-pybind11_amd")

ENTRY_POINTS = {
    "azmi_sample_metrics": "const float* dev_target_pi, const float* dev_p_pi, const float* dev_target_v, const float* dev_p_v, uint32_t n, "
                           "uint32_t M, uint32_t V, double cv, double* dev_cols_out, uint64_t col_stride, uint32_t* dev_mcts_argmax_out, "
                           "uint32_t* dev_net_argmax_out, int device, void* stream",
    "azmi_sample_plane_argmax": "const float* dev_canonical, uint32_t n, uint32_t C, uint32_t H, uint32_t W, uint32_t first_plane, "
                                "uint32_t n_planes, uint32_t row, uint32_t col, uint8_t* dev_out, int device, void* stream",
    "azmi_sample_metrics_reduce": "const double* dev_cols, uint64_t col_stride, uint32_t n, const uint8_t* dev_bucket, uint32_t n_buckets, "
                                  "azmi_sample_metrics_record* host_record_out, int device, void* stream",
}
COLUMNS = ("pi_loss", "v_loss", "target_entropy", "entropy", "kl", "top1", "net_top1", "net_at_mcts", "top1_gap", "top1_agree", "top3_overlap",
           "v_pred", "v_actual")
FLT_MIN = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


class _Lib:
    """stands in for libazmi: any call is a device call the argument checks must come before"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called before the arguments were checked")


class _Tensor:
    """what the checks read of a CUDA tensor, without a device"""
    def __init__(self, shape, device="cuda:0", dtype="torch.float32", contiguous=True, is_cuda=True):
        self.shape, self.device, self.dtype, self.is_cuda, self._contiguous = tuple(shape), device, dtype, is_cuda, contiguous

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        raise AssertionError("data_ptr was read before the arguments were checked")

    def reshape(self, *shape):
        return _Tensor(shape[0] if len(shape) == 1 and isinstance(shape[0], tuple) else shape, self.device, self.dtype, self._contiguous, self.is_cuda)


class _Net:
    def forward(self, *args, **kwargs):
        raise AssertionError("the net ran before the arguments were checked")


# ---- the column table, restated ----------------------------------------------------------------------------------------------
def restate_row(t, p, tv, pv, cv=1.0):
    """one row of the table in float64, element by element: the formulas of network_pareto.py:694-716 and game_runner.py:2560-2581 on
    probabilities, ties to the lower index"""
    t, p, tv, pv = ([float(x) for x in a] for a in (t, p, tv, pv))
    M = len(t)
    ce = lambda ts, ps: -math.fsum(a * math.log(max(b, FLT_MIN)) for a, b in zip(ts, ps) if a > 0)
    order = lambda x: sorted(range(M), key=lambda m: (-x[m], m))[:3]      # a stable argsort of -x
    mcts, net = order(t)[0], order(p)[0]
    return {"pi_loss": ce(t, p), "v_loss": cv * ce(tv, pv), "target_entropy": -math.fsum(a * math.log(a) for a in t if a > 0),
            "entropy": -math.fsum(a * math.log(a + 1e-9) for a in t), "kl": math.fsum(a * math.log(a / (b + 1e-10)) for a, b in zip(t, p) if a > 0),
            "top1": t[mcts], "net_top1": p[net], "net_at_mcts": p[mcts], "top1_gap": t[mcts] - p[mcts], "top1_agree": float(mcts == net),
            "top3_overlap": float(len(set(order(t)) & set(order(p)))), "v_pred": pv[0], "v_actual": tv[0], "mcts_argmax": mcts, "net_argmax": net}


def test_the_restatement_is_the_stated_rule():
    p = [0.1, 0.3, 0.3, 0.3]
    row = restate_row([0.5, 0.5, 0.0, 0.0], p, [1.0, 0.0, 0.0], [0.25, 0.5, 0.25], cv=2.0)
    assert set(row) == set(COLUMNS) | {"mcts_argmax", "net_argmax"}
    assert row["mcts_argmax"] == 0 and row["net_argmax"] == 1 and row["top1_agree"] == 0.0      # the lower of the equal maxima, both times
    assert np.argsort(-np.array(p), kind="stable")[:3].tolist() == [1, 2, 3] and int(np.argmax(p)) == 1
    assert row["top3_overlap"] == 2.0                                                            # {0, 1, 2} (a tied zero: the lower one) & {1, 2, 3}
    assert abs(row["v_loss"] - 2.0 * math.log(4.0)) < 1e-15 and abs(row["target_entropy"] - math.log(2.0)) < 1e-15
    assert abs(row["kl"] - (0.5 * math.log(0.5 / (0.1 + 1e-10)) + 0.5 * math.log(0.5 / (0.3 + 1e-10)))) < 1e-15
    assert row["net_at_mcts"] == 0.1 and row["top1_gap"] == 0.4 and row["v_pred"] == 0.25 and row["v_actual"] == 1.0
    short = restate_row([0.5, 0.5], [0.5, 0.5], [1.0], [1.0])
    assert short["top3_overlap"] == 2.0 and short["mcts_argmax"] == short["net_argmax"] == 0      # M < 3: the sets have M members


# ---- surface -----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_exist_with_the_declared_signatures(az):
    from alphazero import _capi, selfplay
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "azmi.h")).read(), flags=re.S)
    raw = C.CDLL(_capi.LIB_PATH)
    for name, params in ENTRY_POINTS.items():
        assert hasattr(raw, name), f"{name} is not exported by libazmi.so"
        assert name in _capi.SYMBOLS and _capi.SYMBOLS[name][0] is C.c_int and len(_capi.SYMBOLS[name][1]) == params.count(",") + 1
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/azmi.h"
        assert " ".join(m.group(1).split()) == params, f"{name}: the header declares ({' '.join(m.group(1).split())})"
    assert "azmi_sample_metrics_record" in header
    assert C.sizeof(_capi.SampleMetricsRecordC) == 8 * 13 * 8 + 13 * 8 + 8 * 4 + 4 * 4
    for name in ("sample_metrics", "plane_argmax", "eval_metrics", "analyze_samples"):
        assert getattr(az, name) is getattr(az.samples, name)
    assert callable(selfplay.variant_buckets) and callable(selfplay.analyze_iteration)
    import inspect
    assert list(inspect.signature(az.sample_metrics).parameters) == ["pi_target", "pi_p", "v_target", "v_p", "cv", "device", "stream"]
    assert list(inspect.signature(az.plane_argmax).parameters) == ["canonical", "first_plane", "n_planes", "row", "col", "device", "stream"]
    assert list(inspect.signature(az.eval_metrics).parameters) == ["samples", "net", "cv", "batch_rows", "buckets", "n_buckets", "names", "device", "stream"]
    assert list(inspect.signature(az.analyze_samples).parameters) == ["samples", "net", "cv", "batch_rows", "buckets", "names", "device", "stream"]


def test_the_python_columns_are_the_header_enum(az):
    header = open(os.path.join(PKG, "csrc", "sample_metrics_kernels.h")).read()
    body = re.search(r"enum\s+SampleMetric\b[^{]*\{(.*?)\}", header, re.S).group(1)
    device = {re.sub(r"(?<!^)(?=[A-Z])", "_", name).upper(): int(value) for name, value in re.findall(r"\bkSm(\w+)\s*=\s*(\d+)", body)}
    assert len(device) == 13 and device["PI_LOSS"] == 0 and device["NET_AT_MCTS"] == 7 and device["V_ACTUAL"] == 12, device
    assert {m.name: int(m) for m in az.samples.Metric} == device
    assert len(az.samples.Metric.__members__) == len(device), "an alias in Metric"
    assert az.samples.METRIC_COLUMNS == COLUMNS
    assert int(re.search(r"kSampleMetricColumns\s*=\s*(\d+)", header).group(1)) == 13 == az._capi.SAMPLE_METRIC_COLUMNS
    assert int(re.search(r"kMetricMaxBuckets\s*=\s*(\d+)", header).group(1)) == 8 == az._capi.SAMPLE_METRIC_MAX_BUCKETS == az.samples.MAX_BUCKETS
    assert set(az.samples.ANALYSIS_KEYS) < set(COLUMNS) and len(az.samples.ANALYSIS_KEYS) == 10


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_the_c_abi_checks_its_arguments_before_any_device(az):
    lib = az.lib
    err = lambda: lib.azmi_samples_last_error().decode()
    one = (C.c_double * 64)()
    metrics = lambda n=1, M=7, V=3, stride=None, a=one, out=one: lib.azmi_sample_metrics(a, one, one, one, n, M, V, 1.0, out, n if stride is None else stride,
                                                                                        one, one, 0, None)
    assert metrics(M=0) == -1 and "M = 0" in err()
    assert metrics(V=0) == -1 and "V = 0" in err()
    assert metrics(M=(1 << 20) + 1) == -1 and "at most" in err()
    assert metrics(V=(1 << 20) + 1) == -1 and "at most" in err()
    assert metrics(n=(1 << 30) + 1) == -1 and "at most 1073741824 rows" in err()
    assert metrics(n=4, stride=3) == -1 and "col_stride = 3" in err()
    assert metrics(a=None) == -1 and "null argument" in err()
    assert metrics(out=None) == -1 and "null argument" in err()
    assert lib.azmi_sample_metrics(None, None, None, None, 0, 7, 3, 1.0, None, 0, None, None, 0, None) == 0      # n == 0: nothing is touched
    plane = lambda n=1, Cn=36, H=13, W=13, first=32, P=4, row=6, col=6, a=one, out=one: lib.azmi_sample_plane_argmax(a, n, Cn, H, W, first, P, row, col,
                                                                                                                  out, 0, None)
    assert plane(P=0) == -1 and "1 to 16 planes" in err()
    assert plane(P=17, first=0) == -1 and "1 to 16 planes" in err()
    assert plane(first=33) == -1 and "planes 33 .. 33 + 4 of 36" in err()
    assert plane(first=36, P=1) == -1 and "inside the row" in err()
    assert plane(row=13) == -1 and "cell (13, 6) outside the 13 x 13 board" in err()
    assert plane(col=13) == -1 and "outside" in err()
    assert plane(Cn=0) == -1 and "a row of 0 x 13 x 13" in err()
    assert plane(Cn=1 << 16, H=1 << 7, W=1 << 7, first=0) == -1 and "2^30 - 1 float32" in err()
    assert plane(n=(1 << 30) + 1) == -1 and "at most" in err()
    assert plane(a=None) == -1 and "null argument" in err()
    assert plane(n=0, a=None, out=None) == 0
    rec = az._capi.SampleMetricsRecordC()
    reduce_ = lambda n=4, stride=4, B=1, bucket=None, cols=one, r=C.byref(rec): lib.azmi_sample_metrics_reduce(cols, stride, n, bucket, B, r, 0, None)
    assert reduce_(r=None) == -1 and "null argument" in err()
    assert reduce_(B=0, bucket=one) == -1 and "n_buckets = 0: 1 to 8 buckets" in err()
    assert reduce_(B=9, bucket=one) == -1 and "n_buckets = 9" in err()
    assert reduce_(B=2) == -1 and "without a bucket array" in err()
    assert reduce_(stride=3) == -1 and "col_stride = 3" in err()
    assert reduce_(n=(1 << 30) + 1, stride=1 << 31) == -1 and "at most" in err()
    assert reduce_(cols=None) == -1 and "null argument" in err()
    rec.nonfinite = 5
    assert reduce_(n=0, stride=0, cols=None) == 0      # the empty reduction: a zeroed record
    assert rec.nonfinite == 0 and rec.first_nonfinite == 0xFFFFFFFF and rec.invalid == 0 and list(rec.count) == [0] * 8
    assert all(x == 0.0 for row in rec.sum for x in row) and all(x == 0.0 for x in rec.total)


def test_without_a_device_the_entry_points_fail_loudly(az):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    one = (C.c_double * 64)()
    rec = az._capi.SampleMetricsRecordC()
    err = lambda: az.lib.azmi_samples_last_error().decode()
    assert az.lib.azmi_sample_metrics(one, one, one, one, 1, 7, 3, 1.0, one, 1, one, one, 0, None) == -2 and "azmi_sample_metrics: no HIP device" in err()
    assert az.lib.azmi_sample_plane_argmax(one, 1, 36, 13, 13, 32, 4, 6, 6, one, 0, None) == -2 and "azmi_sample_plane_argmax: no HIP device" in err()
    assert az.lib.azmi_sample_metrics_reduce(one, 4, 4, None, 1, C.byref(rec), 0, None) == -2 and "azmi_sample_metrics_reduce: no HIP device" in err()


# ---- the Python functions ----------------------------------------------------------------------------------------------------
def test_sample_metrics_argument_errors_come_before_any_device_call(az, monkeypatch):
    monkeypatch.setattr(az.samples, "lib", _Lib())
    t, v = np.full((4, 7), 1.0 / 7, np.float32), np.full((4, 3), 1.0 / 3, np.float32)
    with pytest.raises(RuntimeError, match=r"sample_metrics: pi_target and pi_p must have one shape, got \(4, 7\) and \(4, 6\)"):
        az.sample_metrics(t, t[:, :6].copy(), v, v)
    with pytest.raises(RuntimeError, match=r"sample_metrics: v_target and v_p must have one shape, got \(4, 3\) and \(3, 3\)"):
        az.sample_metrics(t, t, v, v[:3])
    with pytest.raises(RuntimeError, match=r"one row per sample, got 4 and 3 rows"):
        az.sample_metrics(t, t, v[:3], v[:3])
    with pytest.raises(RuntimeError, match=r"\[n, M\] arrays, v_target and v_p \[n, V\] arrays, got shapes \(4, 7\), \(4, 7\), \(3,\), \(4, 3\)"):
        az.sample_metrics(t, t, v[0], v)
    with pytest.raises(RuntimeError, match=r"M and V must be in \[1, 2\^20\], got M = 0 and V = 3"):
        az.sample_metrics(np.zeros((4, 0), np.float32), np.zeros((4, 0), np.float32), v, v)
    wide = np.broadcast_to(np.float32(0), (4, (1 << 20) + 1))
    with pytest.raises(RuntimeError, match=r"M and V must be in \[1, 2\^20\], got M = 7 and V = 1048577"):
        az.sample_metrics(t, t, wide, wide)
    tall = np.broadcast_to(np.float32(0), ((1 << 30) + 1, 1))
    with pytest.raises(RuntimeError, match=r"sample_metrics: at most 2\^30 rows, got 1073741825"):
        az.sample_metrics(tall, tall, tall, tall)
    with pytest.raises(RuntimeError, match="pi_p must be contiguous float32, got contiguous float64"):
        az.sample_metrics(t, t.astype(np.float64), v, v)
    with pytest.raises(RuntimeError, match="v_target must be contiguous float32, got non-contiguous float32"):
        az.sample_metrics(t, t, np.zeros((4, 6), np.float32)[:, ::2], v)
    with pytest.raises(RuntimeError, match="v_p must be a numpy array or a CUDA tensor, got list"):
        az.sample_metrics(t, t, v, v.tolist())
    for bad in ("one", None, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="sample_metrics: cv must be"):
            az.sample_metrics(t, t, v, v, cv=bad)
    for bad in (-1, 0.0, "0", True, None):
        with pytest.raises(RuntimeError, match="device must be a device index"):
            az.sample_metrics(t, t, v, v, device=bad)
    with pytest.raises(RuntimeError, match="numpy arrays and tensors are mixed: pi_target is a ndarray, pi_p is a ndarray, v_target is a ndarray, v_p is a _Tensor"):
        az.sample_metrics(t, t, v, _Tensor((4, 3)))
    with pytest.raises(RuntimeError, match="v_p must be a CUDA tensor .* it is on cpu"):
        az.sample_metrics(_Tensor((4, 7)), _Tensor((4, 7)), _Tensor((4, 3)), _Tensor((4, 3), device="cpu", is_cuda=False))
    with pytest.raises(RuntimeError, match="the arrays are on different devices: pi_target on cuda:0, pi_p on cuda:1"):
        az.sample_metrics(_Tensor((4, 7)), _Tensor((4, 7), device="cuda:1"), _Tensor((4, 3)), _Tensor((4, 3)))
    with pytest.raises(RuntimeError, match="pi_target must be contiguous float32, got contiguous float16"):
        az.sample_metrics(_Tensor((4, 7), dtype="torch.float16"), _Tensor((4, 7)), _Tensor((4, 3)), _Tensor((4, 3)))


def test_plane_argmax_argument_errors_come_before_any_device_call(az, monkeypatch):
    from alphazero import selfplay
    monkeypatch.setattr(az.samples, "lib", _Lib())
    c = np.zeros((5, 36, 13, 13), np.float32)
    with pytest.raises(RuntimeError, match=r"plane_argmax: canonical must be an \[n, C, H, W\] array, got shape \(36, 13, 13\)"):
        az.plane_argmax(c[0], 32, 4, 6, 6)
    with pytest.raises(RuntimeError, match=r"the planes 33 .. 36 are outside the 36 planes of canonical"):
        az.plane_argmax(c, 33, 4, 6, 6)
    with pytest.raises(RuntimeError, match=r"the planes 36 .. 36 are outside the 36 planes"):
        az.plane_argmax(c, 36, 1, 6, 6)
    for bad in (0, 17):
        with pytest.raises(RuntimeError, match=r"n_planes must be in \[1, 16\], got %d" % bad):
            az.plane_argmax(c, 0, bad, 6, 6)
    with pytest.raises(RuntimeError, match=r"the cell \(13, 6\) is outside the 13 x 13 board"):
        az.plane_argmax(c, 32, 4, 13, 6)
    with pytest.raises(RuntimeError, match=r"the cell \(6, 13\) is outside"):
        az.plane_argmax(c, 32, 4, 6, 13)
    for name, args in (("first_plane", (-1, 4, 6, 6)), ("n_planes", (32, 4.0, 6, 6)), ("row", (32, 4, None, 6)), ("col", (32, 4, 6, True))):
        with pytest.raises(RuntimeError, match=f"plane_argmax: {name} must be an integer >= 0"):
            az.plane_argmax(c, *args)
    with pytest.raises(RuntimeError, match="canonical must be contiguous float32, got contiguous float64"):
        az.plane_argmax(c.astype(np.float64), 32, 4, 6, 6)
    with pytest.raises(RuntimeError, match="canonical must be contiguous float32, got non-contiguous float32"):
        az.plane_argmax(np.zeros((5, 36, 13, 26), np.float32)[..., ::2], 32, 4, 6, 6)
    with pytest.raises(RuntimeError, match="canonical must be a numpy array or a CUDA tensor, got list"):
        az.plane_argmax([[[[0.0]]]], 0, 1, 0, 0)
    with pytest.raises(RuntimeError, match="canonical must be a CUDA tensor"):
        az.plane_argmax(_Tensor((5, 36, 13, 13), device="cpu", is_cuda=False), 32, 4, 6, 6)
    with pytest.raises(RuntimeError, match="device must be a device index"):
        az.plane_argmax(c, 32, 4, 6, 6, device=-1)
    # a Connect4 canonical has no plane 32: the unified encoding's reader says so by name
    with pytest.raises(RuntimeError, match=r"the planes 32 .. 35 are outside the 4 planes"):
        selfplay.variant_buckets(az.StarGambitUnifiedGS, np.zeros((5, 4, 6, 7), np.float32))
    assert selfplay.variant_buckets(az.Connect4GS, c) is None and selfplay.variant_buckets(az.TawlbwrddGS, c) is None


def test_eval_metrics_and_analyze_samples_argument_errors_come_before_any_device_call(az, monkeypatch):
    from alphazero import selfplay
    monkeypatch.setattr(az.samples, "lib", _Lib())
    c, v, pi = np.zeros((5, 4, 6, 7), np.float32), np.zeros((5, 3), np.float32), np.zeros((5, 7), np.float32)
    net = _Net()
    ids = np.zeros(5, np.uint8)
    for fn in (lambda s, **kw: az.eval_metrics(s, net, **kw), lambda s, **kw: az.analyze_samples(s, net, **kw),
               lambda s, **kw: selfplay.analyze_iteration(az.Connect4GS, s, net, **kw)):
        with pytest.raises(RuntimeError, match="the shapes of canonical .* do not agree"):
            fn((c, v[:4], pi))
        with pytest.raises(RuntimeError, match="samples must be the .canonical, v, pi. triple"):
            fn((c, v))
        with pytest.raises(RuntimeError, match="pi must be contiguous float32, got contiguous float64"):
            fn((c, v, pi.astype(np.float64)))
        for bad in (0, -3, 1.5, None, True):
            with pytest.raises(RuntimeError, match="batch_rows must be an integer >= 1"):
                fn((c, v, pi), batch_rows=bad)
        with pytest.raises(RuntimeError, match="the arrays are on different devices: canonical on cuda:0, v on cuda:1, pi on cuda:0"):
            fn((_Tensor((5, 4, 6, 7)), _Tensor((5, 3), device="cuda:1"), _Tensor((5, 7))))
        with pytest.raises(RuntimeError, match="numpy arrays and tensors are mixed"):
            fn((c, v, _Tensor((5, 7))))
        for bad in ("one", None, float("nan")):
            with pytest.raises(RuntimeError, match="cv must be"):
                fn((c, v, pi), cv=bad)
        with pytest.raises(RuntimeError, match="device must be a device index"):
            fn((c, v, pi), device=-1)
    for fn in (az.eval_metrics, az.analyze_samples):
        what = fn.__name__
        with pytest.raises(RuntimeError, match=f"{what}: net must be a HipLeafNet, got NoneType"):
            fn((c, v, pi), None)
        with pytest.raises(RuntimeError, match=rf"{what}: buckets must hold one id per sample \(5\), got shape \(4,\)"):
            fn((c, v, pi), net, buckets=ids[:4], names=["a"])
        with pytest.raises(RuntimeError, match=rf"{what}: buckets must hold one id per sample \(5\), got shape \(5, 1\)"):
            fn((c, v, pi), net, buckets=ids.reshape(5, 1), names=["a"])
        with pytest.raises(RuntimeError, match=f"{what}: buckets must be contiguous uint8, got contiguous int64"):
            fn((c, v, pi), net, buckets=ids.astype(np.int64), names=["a"])
        with pytest.raises(RuntimeError, match=f"{what}: buckets must be contiguous uint8, got non-contiguous uint8"):
            fn((c, v, pi), net, buckets=np.zeros(10, np.uint8)[::2], names=["a"])
        with pytest.raises(RuntimeError, match=f"{what}: numpy arrays and tensors are mixed: .*buckets is a _Tensor"):
            fn((c, v, pi), net, buckets=_Tensor((5,), dtype="torch.uint8"), names=["a"])
        with pytest.raises(RuntimeError, match=f"{what}: names must be distinct strings"):
            fn((c, v, pi), net, buckets=ids, names=["a", "a"])
        with pytest.raises(RuntimeError, match=f"{what}: names must be distinct strings"):
            fn((c, v, pi), net, buckets=ids, names=["a", 1])
        with pytest.raises(RuntimeError, match=f"{what}: .*go with buckets, which is None"):
            fn((c, v, pi), net, names=["a"])
    for bad in (0, 9, -1, 2.0, True, "2"):
        with pytest.raises(RuntimeError, match=r"eval_metrics: n_buckets must be an integer in \[1, 8\]"):
            az.eval_metrics((c, v, pi), net, buckets=ids, n_buckets=bad)
    with pytest.raises(RuntimeError, match="eval_metrics: 9 names for 8 buckets|n_buckets must be an integer"):
        az.eval_metrics((c, v, pi), net, buckets=ids, names=[str(k) for k in range(9)])
    with pytest.raises(RuntimeError, match="eval_metrics: 2 names for 3 buckets"):
        az.eval_metrics((c, v, pi), net, buckets=ids, n_buckets=3, names=["a", "b"])
    with pytest.raises(RuntimeError, match="eval_metrics: with buckets, give n_buckets or names"):
        az.eval_metrics((c, v, pi), net, buckets=ids)
    with pytest.raises(RuntimeError, match='names must be distinct strings other than "overall"'):
        az.eval_metrics((c, v, pi), net, buckets=ids, names=["a", "overall"])
    with pytest.raises(RuntimeError, match="eval_metrics: n_buckets and names go with buckets"):
        az.eval_metrics((c, v, pi), net, n_buckets=2)


def test_no_samples_give_empty_or_nan_results_without_a_device(az, monkeypatch):
    from alphazero import selfplay
    monkeypatch.setattr(az.samples, "lib", _Lib())
    empty, ev = np.zeros((0, 7), np.float32), np.zeros((0, 3), np.float32)
    got = az.sample_metrics(empty, empty, ev, ev)
    assert tuple(got) == COLUMNS + ("mcts_argmax", "net_argmax")
    assert all(got[k].dtype == np.float64 and got[k].shape == (0,) for k in COLUMNS)
    assert got["mcts_argmax"].dtype == got["net_argmax"].dtype == np.uint32 and got["net_argmax"].shape == (0,)
    ids = az.plane_argmax(np.zeros((0, 36, 13, 13), np.float32), 32, 4, 6, 6)
    assert ids.dtype == np.uint8 and ids.shape == (0,)
    none = (np.zeros((0, 4, 6, 7), np.float32), ev, empty)
    figures = az.eval_metrics(none, _Net(), cv=1.5)
    assert tuple(figures) == az.samples.EVAL_KEYS and figures["count"] == 0
    assert all(math.isnan(figures[k]) for k in az.samples.EVAL_KEYS if k != "count")
    split = az.eval_metrics(none, _Net(), buckets=np.zeros(0, np.uint8), n_buckets=4)
    assert list(split) == ["overall"] and split["overall"]["count"] == 0 and math.isnan(split["overall"]["kl_gap"])
    for whole in (az.analyze_samples(none, _Net()), selfplay.analyze_iteration(az.Connect4GS, none, _Net()),
                  selfplay.analyze_iteration(az.StarGambitUnifiedGS, (np.zeros((0, 36, 13, 13), np.float32), ev, empty), _Net())):
        assert list(whole) == ["overall"] and tuple(whole["overall"]) == az.samples.ANALYSIS_KEYS
        assert all(x.dtype == np.float64 and x.shape == (0,) for x in whole["overall"].values())
    assert az.analyze_samples(none, _Net(), buckets=np.zeros(0, np.uint8), names=["a", "b"]) == {}


def test_the_package_and_the_module_import_without_torch(az):
    code = ("import sys; sys.path.insert(0, %r); import alphazero; from alphazero import samples, selfplay; import numpy as np; "
            "e, v = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32); alphazero.sample_metrics(e, e, v, v); "
            "alphazero.plane_argmax(np.zeros((0, 4, 6, 7), np.float32), 0, 2, 0, 0); "
            "alphazero.eval_metrics((np.zeros((0, 4, 6, 7), np.float32), v, e), object.__new__(type('N', (), {'forward': None}))); "
            "print('torch' in sys.modules)" % PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "False", "the samples module pulled in torch"
