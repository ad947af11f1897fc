"""CPU: scoring a visit sweep on the device: azmi_search_sweep_metrics / azmi_policy_divergences are exported with the declared
signatures, and every argument error of MCTSBatch.sweep_metrics() / alphazero.policy_divergences() is raised in Python, by name,
before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p

ENTRY_POINTS = {
    "azmi_search_sweep_metrics": ([VP, VP, C.c_uint32, C.c_int32, VP, VP, VP, VP, VP, VP, VP],
                                  "azmi_search* s, azmi_search* ref, uint32_t anchor, int32_t raw, const double* outcomes, "
                                  "double* out_rows, double* out_tree, double* out_mean, uint32_t* out_count, uint8_t* valid, "
                                  "void* stream"),
    "azmi_policy_divergences": ([VP, VP, C.c_uint32, C.c_uint32, VP, C.c_int, VP],
                                "const float* p, const float* q, uint32_t rows, uint32_t M, double* out, int device, void* stream"),
}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from alphazero import _capi
    return _capi


def test_the_two_symbols_exist_with_the_declared_signatures(capi):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "azmi.h")).read(), flags=re.S)
    raw = C.CDLL(capi.LIB_PATH)
    for name, (argtypes, params) in ENTRY_POINTS.items():
        assert hasattr(raw, name), f"{name} is not exported by libazmi.so"
        assert name in capi.SYMBOLS, f"{name} is missing from _capi.SYMBOLS"
        res, args = capi.SYMBOLS[name]
        assert res is C.c_int and list(args) == argtypes, f"{name}: _capi declares {args}"
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/azmi.h"
        assert " ".join(m.group(1).split()) == params, f"{name}: the header declares ({' '.join(m.group(1).split())})"


def test_the_names_are_exported_and_the_columns_are_the_issue_s(capi):
    import alphazero as az
    assert az.policy_divergences is az.search_batch_sweep.policy_divergences
    assert az.POLICY_COLUMNS == ("jsd", "tv", "hellinger", "top1", "top3", "top9")
    assert az.SWEEP_COLUMNS == az.POLICY_COLUMNS + ("reward", "regret", "pressure", "benefit", "entropy", "value_gap", "abs_err",
                                                    "closer_than_anchor", "closer_than_raw")


class _Lib:
    """stands in for libazmi: any call is a device call the argument checks must come before"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called before the arguments were checked")


def _batch(az, n=3, game=None, device=0, sweep_j=3):
    mb = object.__new__(az.MCTSBatch)                          # no device: the checks below need none
    mb._h, mb._n, mb._M, mb._P, mb._chw, mb._gumbel = None, n, 7, 2, (4, 6, 7), False
    mb._game, mb._device, mb._rows = game or az.Connect4GS, device, None
    if sweep_j is not None:
        mb._sweep_j = sweep_j
    return mb


def test_sweep_metrics_argument_errors_come_before_any_device_call(capi, monkeypatch):
    import alphazero as az
    monkeypatch.setattr(az.search_batch_sweep, "lib", _Lib())
    mb = _batch(az)
    # the state of this batch
    with pytest.raises(RuntimeError, match="sweep_metrics: no search_to call has been made on this batch"):
        _batch(az, sweep_j=None).sweep_metrics()
    pending = _batch(az)
    pending._rows = 2
    with pytest.raises(RuntimeError, match="sweep_metrics: a find_leaves step is pending"):
        pending.sweep_metrics()
    with pytest.raises(RuntimeError, match="no checkpoints: nothing to anchor on"):
        _batch(az, sweep_j=0).sweep_metrics()
    # anchor
    for bad in (3, -4, 100):
        with pytest.raises(RuntimeError, match=r"anchor = %d out of range: the reference set has 3 checkpoints" % bad):
            mb.sweep_metrics(anchor=bad)
    for bad in (1.0, "last", None, True):
        with pytest.raises(RuntimeError, match="anchor must be a checkpoint index"):
            mb.sweep_metrics(anchor=bad)
    # raw
    for bad in (3, -4):
        with pytest.raises(RuntimeError, match=r"raw = %d out of range" % bad):
            mb.sweep_metrics(raw=bad)
    for bad in (0.0, "first", False):
        with pytest.raises(RuntimeError, match="raw must be a checkpoint index"):
            mb.sweep_metrics(raw=bad)
    # outcomes
    with pytest.raises(RuntimeError, match=r"outcomes: one per tree \(3\), got shape \(2,\)"):
        mb.sweep_metrics(outcomes=[1.0, -1.0])
    with pytest.raises(RuntimeError, match=r"outcomes: one per tree \(3\), got shape \(3, 1\)"):
        mb.sweep_metrics(outcomes=np.zeros((3, 1)))
    with pytest.raises(RuntimeError, match=r"outcomes: one per tree \(3\), got shape \(1,\)"):
        mb.sweep_metrics(outcomes=1.0)                          # (a number is an array of one)
    with pytest.raises(RuntimeError, match="outcomes must be 3 numbers"):
        mb.sweep_metrics(outcomes=["win", "loss", "draw"])
    # reference
    with pytest.raises(RuntimeError, match="reference must be an MCTSBatch or None, got list"):
        mb.sweep_metrics(reference=[mb])
    with pytest.raises(RuntimeError, match="the reference batch holds 4 trees, this batch 3"):
        mb.sweep_metrics(reference=_batch(az, n=4))
    with pytest.raises(RuntimeError, match="the reference batch holds another game"):
        mb.sweep_metrics(reference=_batch(az, game=az.BrandubhGS))
    with pytest.raises(RuntimeError, match="the reference batch is on device 1, this batch on 0"):
        mb.sweep_metrics(reference=_batch(az, device=1))
    with pytest.raises(RuntimeError, match="no search_to call has been made on the reference batch"):
        mb.sweep_metrics(reference=_batch(az, sweep_j=None))
    ref_pending = _batch(az)
    ref_pending._rows = 0
    with pytest.raises(RuntimeError, match="a find_leaves step is pending on the reference batch"):
        mb.sweep_metrics(reference=ref_pending)
    # the indices count in the REFERENCE's set
    with pytest.raises(RuntimeError, match=r"anchor = 2 out of range: the reference set has 2 checkpoints"):
        mb.sweep_metrics(anchor=2, reference=_batch(az, sweep_j=2))
    # correct arguments pass the checks: the stand-in is reached
    for kw in (dict(), dict(anchor=-3, raw=2), dict(anchor=np.int64(1), raw=-1, outcomes=np.array([1, 0, -1])),
               dict(reference=_batch(az, sweep_j=5), anchor=4, raw=0)):
        with pytest.raises(AssertionError, match="azmi_search_sweep_metrics was called"):
            mb.sweep_metrics(**kw)


def test_negative_indices_count_from_the_end_of_the_reference_set(capi):
    import alphazero as az
    mb, ref = _batch(az, sweep_j=3), _batch(az, sweep_j=5)
    assert mb._sweep_args(-1, None, None, None)[1:3] == (2, -1)
    assert mb._sweep_args(-3, -1, None, None)[1:3] == (0, 2)
    got = mb._sweep_args(-1, -5, ref, [0, 1, 2])
    assert got[0] is ref and got[1:3] == (4, 0) and got[3].dtype == np.float64 and got[3].tolist() == [0.0, 1.0, 2.0]


def test_policy_divergences_argument_errors_come_before_any_device_call(capi, monkeypatch):
    import alphazero as az
    monkeypatch.setattr(az.search_batch_sweep, "lib", _Lib())
    p = np.full((4, 7), 1.0 / 7, np.float32)
    with pytest.raises(RuntimeError, match=r"one shape, got \(4, 7\) and \(4, 6\)"):
        az.policy_divergences(p, p[:, :6])
    with pytest.raises(RuntimeError, match=r"one shape, got \(4, 7\) and \(3, 7\)"):
        az.policy_divergences(p, p[:3])
    with pytest.raises(RuntimeError, match=r"\[rows, M\] arrays, got shapes \(2, 2, 7\) and \(2, 2, 7\)"):
        az.policy_divergences(np.zeros((2, 2, 7)), np.zeros((2, 2, 7)))
    with pytest.raises(RuntimeError, match=r"\[rows, M\] arrays, got shapes \(4, 7\) and \(7,\)"):
        az.policy_divergences(p, p[0])
    with pytest.raises(RuntimeError, match=r"\[rows, M\] arrays, got shapes \(\) and \(\)"):
        az.policy_divergences(0.5, 0.5)
    with pytest.raises(RuntimeError, match=r"M must be in \[1, 2\^20\], got 0"):
        az.policy_divergences(np.zeros((3, 0)), np.zeros((3, 0)))
    with pytest.raises(RuntimeError, match="must be arrays of numbers"):
        az.policy_divergences([["a", "b"]], [["c", "d"]])
    for bad in (-1, 0.0, "0", True, None):
        with pytest.raises(RuntimeError, match="device must be a device index"):
            az.policy_divergences(p, p, device=bad)
    # correct arguments pass the checks: the stand-in is reached (one-dimensional arrays are one row)
    for a in (p, p[0], np.zeros((0, 7), np.float32)):
        with pytest.raises(AssertionError, match="azmi_policy_divergences was called"):
            az.policy_divergences(a, a)
