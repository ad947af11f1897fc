"""CPU: the history window and the reservoir of alphazero.samples (reservoir_keys, select_top, window_batches, SampleWindow,
selfplay.training_batches): the entry points exist with the declared signatures, every refusal is a RuntimeError raised by name
before the library is touched, empty calls need no device, and the reference permutation of tests/sample_window_ref.py is a
bijection."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_window_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {
    "azmi_samples_reservoir_keys": "const int32_t* dev_iters, const uint64_t* dev_row_ids, uint32_t n, double iteration, double decay, "
                                   "uint64_t seed, double* dev_keys_out, uint64_t* dev_bits_out, int device, void* stream",
    "azmi_samples_select_top": "const double* dev_keys, uint32_t n, uint32_t k, int64_t* dev_index_out, azmi_select_record* host_record_out, "
                               "int device, void* stream",
    "azmi_samples_window_gather": "const void* const* dev_segments, const uint64_t* segment_rows, uint32_t n_segments, uint32_t row_bytes, "
                                  "const int64_t* dev_index, uint64_t seed, uint64_t pass_index, uint64_t first, uint32_t rows, void* dev_out, "
                                  "int device, void* stream",
}


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


def _segment(n, row=(1, 2, 3), V=3, M=7):
    return (np.zeros((n,) + row, np.float32), np.zeros((n, V), np.float32), np.zeros((n, M), np.float32))


def test_the_entry_points_exist_with_the_declared_signatures(az):
    from alphazero import _capi, selfplay
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "azmi.h")).read(), flags=re.S)
    raw = C.CDLL(_capi.LIB_PATH)
    for name, params in ENTRY_POINTS.items():
        assert hasattr(raw, name), f"{name} is not exported by libazmi.so"
        assert name in _capi.SYMBOLS and _capi.SYMBOLS[name][0] is C.c_int
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/azmi.h"
        assert " ".join(m.group(1).split()) == params, f"{name}: the header declares ({' '.join(m.group(1).split())})"
        assert len(_capi.SYMBOLS[name][1]) == params.count(",") + 1
    assert C.sizeof(_capi.SelectRecordC) == 24 and _capi.WINDOW_MAX_SEGMENTS == 64
    assert re.search(r"#define\s+AZMI_WINDOW_MAX_SEGMENTS\s+64\b", header)
    for name in ("reservoir_keys", "select_top", "window_batches", "SampleWindow"):
        assert getattr(az, name) is getattr(az.samples, name)
    assert callable(selfplay.training_batches)
    assert az.lib.azmi_abi_version() == 1      # the entry points are additive


def test_the_c_abi_checks_its_arguments_before_any_device(az):
    lib = az.lib
    err = lambda: lib.azmi_samples_last_error().decode()
    one = (C.c_double * 8)()
    rec = az._capi.SelectRecordC()
    assert lib.azmi_samples_reservoir_keys(None, None, 0, 3.0, 0.5, 1, None, None, 0, None) == 0
    for decay in (0.0, -0.5, 1.5, float("nan")):
        assert lib.azmi_samples_reservoir_keys(one, None, 4, 3.0, decay, 1, one, None, 0, None) == -1 and "decay must be in (0, 1]" in err()
    for it in (float("inf"), float("nan")):
        assert lib.azmi_samples_reservoir_keys(one, None, 4, it, 0.5, 1, one, None, 0, None) == -1 and "iteration must be finite" in err()
    assert lib.azmi_samples_reservoir_keys(None, None, 4, 3.0, 0.5, 1, one, None, 0, None) == -1 and "null argument" in err()
    assert lib.azmi_samples_reservoir_keys(one, None, (1 << 30) + 1, 3.0, 0.5, 1, one, None, 0, None) == -1 and "at most" in err()
    assert lib.azmi_samples_select_top(None, 5, 0, None, C.byref(rec), 0, None) == 0      # k == 0: nothing is touched
    assert (rec.selected, rec.nan_rows, rec.first_bad_row) == (0, 0, 0xFFFFFFFF)
    assert lib.azmi_samples_select_top(one, 5, 6, one, C.byref(rec), 0, None) == -1 and "k = 6 of n = 5 keys" in err()
    assert lib.azmi_samples_select_top(one, 5, 2, one, None, 0, None) == -1 and "null argument" in err()
    assert lib.azmi_samples_select_top(None, 5, 2, one, C.byref(rec), 0, None) == -1 and "null argument" in err()
    ptrs = (C.c_void_p * 65)(*[C.addressof(one)] * 65)
    rows = (C.c_uint64 * 65)(*[2] * 65)
    gather = lambda ns, rb, first, n, out=one: lib.azmi_samples_window_gather(ptrs, rows, ns, rb, None, 1, 0, first, n, out, 0, None)
    assert gather(65, 8, 0, 1) == -1 and "65 segments: 1 to 64 per call" in err()
    assert gather(0, 8, 0, 0) == -1 and "0 segments" in err()
    assert gather(3, 6, 0, 1) == -1 and "a row of 6 bytes" in err()
    assert gather(3, 8, 5, 2) == -1 and "of a window of 6 rows" in err()
    assert gather(3, 8, 7, 0) == -1 and "of a window of 6 rows" in err()
    assert gather(3, 8, 6, 0) == 0 and gather(3, 8, 2, 0, None) == 0      # no rows: nothing is touched
    assert gather(3, 8, 0, 2, None) == -1 and "dev_out" in err()
    ptrs[1] = None
    assert gather(3, 8, 0, 2) == -1 and "segment 1: null argument" in err()
    rows[1] = 0
    assert gather(3, 8, 4, 0) == 0      # (an empty segment needs no array)


def test_reservoir_keys_and_select_top_refusals_come_before_the_library(az, monkeypatch):
    monkeypatch.setattr(az.samples, "lib", _Lib())
    iters = np.zeros(5, np.int32)
    for bad in (0, 0.0, -0.1, 1.0000001, 2, float("nan"), float("inf"), "0.5", None, True):
        with pytest.raises(RuntimeError, match=r"reservoir_keys: decay must be a number in \(0, 1\]"):
            az.reservoir_keys(iters, 3, bad, 1)
    for bad in (float("nan"), float("inf"), -1, "3", None):
        with pytest.raises(RuntimeError, match="reservoir_keys: iteration must be a finite number >= 0"):
            az.reservoir_keys(iters, bad, 0.5, 1)
    for bad in (-1, 1 << 64, 1.0, None):
        with pytest.raises(RuntimeError, match=r"reservoir_keys: seed must be an integer in \[0, 2\^64\)"):
            az.reservoir_keys(iters, 3, 0.5, bad)
    with pytest.raises(RuntimeError, match="iters must be contiguous int32, got contiguous int64"):
        az.reservoir_keys(iters.astype(np.int64), 3, 0.5, 1)
    with pytest.raises(RuntimeError, match="iters must be contiguous int32, got non-contiguous int32"):
        az.reservoir_keys(np.zeros(10, np.int32)[::2], 3, 0.5, 1)
    with pytest.raises(RuntimeError, match=r"iters must be one-dimensional, got shape \(5, 1\)"):
        az.reservoir_keys(iters.reshape(5, 1), 3, 0.5, 1)
    with pytest.raises(RuntimeError, match=r"row_ids must hold one id per row \(5\), got shape \(4,\)"):
        az.reservoir_keys(iters, 3, 0.5, 1, row_ids=np.zeros(4, np.uint64))
    with pytest.raises(RuntimeError, match="row_ids must be contiguous uint64 or int64, got contiguous int32"):
        az.reservoir_keys(iters, 3, 0.5, 1, row_ids=iters)
    keys = np.zeros(6)
    for bad in (-1, 7, 1.0, "2", None, True):
        with pytest.raises(RuntimeError, match=r"select_top: k must be an integer in \[0, n = 6\]"):
            az.select_top(keys, bad)
    with pytest.raises(RuntimeError, match="keys must be contiguous float64, got contiguous float32"):
        az.select_top(keys.astype(np.float32), 2)
    with pytest.raises(RuntimeError, match="keys must be contiguous float64, got non-contiguous float64"):
        az.select_top(np.zeros(12)[::2], 2)
    with pytest.raises(RuntimeError, match=r"keys must be one-dimensional, got shape \(2, 3\)"):
        az.select_top(keys.reshape(2, 3), 2)
    with pytest.raises(RuntimeError, match="keys must be a numpy array or a CUDA tensor, got list"):
        az.select_top([1.0, 2.0], 1)
    # empty calls need no device
    assert az.reservoir_keys(np.zeros(0, np.int32), 3, 0.5, 1).shape == (0,)
    index, record = az.select_top(keys, 0)
    assert index.shape == (0,) and index.dtype == np.int64 and record["selected"] == 0


def test_window_batches_refusals_come_before_the_library(az, monkeypatch):
    monkeypatch.setattr(az.samples, "lib", _Lib())
    seg = _segment(4)
    with pytest.raises(RuntimeError, match="window_batches: at most 64 segments, got 65"):
        az.window_batches([seg] * 65, 8, 1)
    for bad in (0, -3, 1.0, "8", None, True):
        with pytest.raises(RuntimeError, match=r"window_batches: batch_rows must be an integer in \[1, 2\^30\]"):
            az.window_batches([seg], bad, 1)
    c, v, pi = seg
    with pytest.raises(RuntimeError, match=r"segments\[1\]: canonical, v and pi must hold one row per sample, got 4, 3 and 4 rows"):
        az.window_batches([seg, (c, v[:3], pi)], 8, 1)
    with pytest.raises(RuntimeError, match=r"segments\[0\]: canonical, v and pi must hold one row per sample, got 4, 4 and 5 rows"):
        az.window_batches([(c, v, np.zeros((5, 7), np.float32))], 8, 1)
    with pytest.raises(RuntimeError, match=r"segments\[0\].pi must be contiguous float32, got contiguous float64"):
        az.window_batches([(c, v, pi.astype(np.float64))], 8, 1)
    with pytest.raises(RuntimeError, match=r"segments\[1\].canonical must be contiguous float32, got non-contiguous float32"):
        az.window_batches([seg, (np.zeros((4, 1, 2, 6), np.float32)[..., ::2], v, pi)], 8, 1)
    with pytest.raises(RuntimeError, match=r"segments\[1\]: rows of shapes \(1, 2, 3\), \(3,\), \(6,\) in a window of \(1, 2, 3\), \(3,\), \(7,\)"):
        az.window_batches([seg, _segment(2, M=6)], 8, 1)
    with pytest.raises(RuntimeError, match=r"segments\[0\] must be the \(canonical, v, pi\) triple"):
        az.window_batches([(c, v)], 8, 1)
    with pytest.raises(RuntimeError, match=r"canonical \[n, C, H, W\], v \[n, V\] and pi \[n, M\] are wanted"):
        az.window_batches([(c.reshape(4, 6), v, pi)], 8, 1)
    with pytest.raises(RuntimeError, match=r"window_batches: seed must be an integer in \[0, 2\^64\)"):
        az.window_batches([seg], 8, -1)
    with pytest.raises(RuntimeError, match="pass_index must be an integer"):
        az.window_batches([seg], 8, 1, pass_index=-1)
    with pytest.raises(RuntimeError, match=r"first must be a row of the window, an integer in \[0, 4\], got 5"):
        az.window_batches([seg], 8, 1, first=5)
    with pytest.raises(RuntimeError, match="batches must be None or an integer >= 0"):
        az.window_batches([seg], 8, 1, batches=-1)
    # nothing to yield: no device
    assert list(az.window_batches([], 8, 1)) == [] and list(az.window_batches([seg], 8, 1, first=4)) == []
    assert list(az.window_batches([seg], 8, 1, batches=0)) == [] and list(az.window_batches([_segment(0)], 8, 1)) == []


def test_sample_window_refusals_come_before_the_library(az, monkeypatch):
    from alphazero import selfplay
    monkeypatch.setattr(az.samples, "lib", _Lib())
    for bad in (0, -1, 1.0, None, True):
        with pytest.raises(RuntimeError, match="SampleWindow: hist_size must be an integer >= 1"):
            az.SampleWindow(bad, 100, 0.9, 1)
    for bad in (0.0, 1.5, -1, float("nan"), None):
        with pytest.raises(RuntimeError, match=r"SampleWindow: decay must be a number in \(0, 1\]"):
            az.SampleWindow(2, 100, bad, 1)
    with pytest.raises(RuntimeError, match="SampleWindow: reservoir_rows must be an integer"):
        az.SampleWindow(2, -1, 0.9, 1)
    with pytest.raises(RuntimeError, match="SampleWindow: update_interval must be an integer >= 1"):
        az.SampleWindow(2, 100, 0.9, 1, update_interval=0)
    with pytest.raises(RuntimeError, match=r"SampleWindow: seed must be an integer in \[0, 2\^64\)"):
        az.SampleWindow(2, 100, 0.9, -1)
    w = az.SampleWindow(2, 100, 0.9, 1)
    c, v, pi = _segment(4)
    with pytest.raises(RuntimeError, match="SampleWindow.append: the shapes of canonical"):
        w.append(0, (c, v[:3], pi))
    with pytest.raises(RuntimeError, match="pi must be contiguous float32, got contiguous float64"):
        w.append(0, (c, v, pi.astype(np.float64)))
    with pytest.raises(RuntimeError, match="SampleWindow.append: iteration must be an integer"):
        w.append(-1, (c, v, pi))
    for bad in (0, -2, 1.5, None):
        with pytest.raises(RuntimeError, match=r"SampleWindow.batches: batch_rows must be an integer in \[1, 2\^30\]"):
            w.batches(bad)
    with pytest.raises(RuntimeError, match="SampleWindow.batches: sample_rate must be a finite number >= 0"):
        w.batches(8, sample_rate=float("nan"))
    with pytest.raises(RuntimeError, match="training_batches: window must be a SampleWindow, got list"):
        selfplay.training_batches([], 8)
    with pytest.raises(RuntimeError, match=r"SampleWindow.batches: batch_rows must be an integer in \[1, 2\^30\]"):
        selfplay.training_batches(w, 0)
    # an empty window yields nothing and reports zeros, without a device
    assert list(w.batches(8)) == [] and w.update_reservoir(0) == 0
    assert w.stats() == {"window_rows": 0, "reservoir_rows": 0, "staged_rows": 0, "window_iterations": [], "evicted_iterations": 0, "host_syncs": 0}


@pytest.mark.parametrize("total", [1, 2, 3, 255, 256, 257, 70001])
def test_the_reference_permutation_is_a_bijection(total):
    perms = [ref.permutation(total, seed, p) for seed, p in ((0, 0), (20261021, 0), (20261021, 1), ((1 << 64) - 1, 7))]
    for perm in perms:
        assert perm.shape == (total,) and np.array_equal(np.sort(perm), np.arange(total))
    if total >= 255:      # two passes, and two seeds, are different orders
        assert not np.array_equal(perms[1], perms[2]) and not np.array_equal(perms[0], perms[1])
        assert not np.array_equal(perms[1], np.arange(total))


def test_the_reference_mixer_is_the_package_mixer(az):
    from alphazero import _rng
    xs = [0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1, 20261021]
    assert [int(x) for x in ref.mix64(np.array(xs, np.uint64))] == [_rng.mix64(x) for x in xs]
    m = ref.uniform_bits(7, np.arange(1000))
    assert (m & np.uint64(1)).all() and int(m.max()) < 1 << 53
    keys = ref.reservoir_keys(np.zeros(1000, np.int32), 5, 0.5, 7)
    assert np.isfinite(keys).all() and (keys < 0).all()
    assert np.array_equal(ref.reservoir_keys(np.array([0], np.int32), 5000, 0.5, 7), [-np.inf])      # the weight underflows
    assert np.array_equal(ref.select_top(np.array([1.0, 3.0, 3.0, -np.inf, 3.0, 0.0, -0.0]), 3), [1, 2, 4])
    assert np.array_equal(ref.select_top(np.array([-0.0, 0.0, -1.0]), 1), [0])
