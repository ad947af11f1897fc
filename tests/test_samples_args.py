"""CPU: alphazero.samples (sample_loss, resample_plan, resample_rows, resample_by_surprise, iteration_losses) and
selfplay.process_samples: the entry points are exported with the declared signatures, every argument error is a RuntimeError
raised by name before any device call, n == 0 returns empty results without a device, and the package still imports without
torch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-pybind11_amd")
VP = C.c_void_p

ENTRY_POINTS = {
    "azmi_sample_loss": "const float* dev_target, const float* dev_p, uint32_t n, uint32_t M, double scale, double* dev_loss_out, "
                        "int device, void* stream",
    "azmi_resample_plan": "const double* dev_loss, uint32_t n, uint64_t seed, uint32_t* dev_copies, uint64_t* dev_offsets, "
                          "azmi_resample_record* host_record_out, int device, void* stream",
    "azmi_resample_gather": "const uint32_t* dev_copies, const uint64_t* dev_offsets, uint32_t n, uint32_t n_arrays, "
                            "const void* const* dev_in, void* const* dev_out, const uint32_t* row_bytes, int device, void* stream",
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


def test_the_entry_points_exist_with_the_declared_signatures(az):
    from alphazero import _capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "azmi.h")).read(), flags=re.S)
    raw = C.CDLL(_capi.LIB_PATH)
    for name, params in ENTRY_POINTS.items():
        assert hasattr(raw, name), f"{name} is not exported by libazmi.so"
        assert name in _capi.SYMBOLS and _capi.SYMBOLS[name][0] is C.c_int
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/azmi.h"
        assert " ".join(m.group(1).split()) == params, f"{name}: the header declares ({' '.join(m.group(1).split())})"
    assert hasattr(raw, "azmi_samples_last_error") and "azmi_samples_last_error" in _capi.SYMBOLS
    assert C.sizeof(_capi.ResampleRecordC) == 24
    for name in ("sample_loss", "resample_plan", "resample_rows", "resample_by_surprise", "iteration_losses"):
        assert getattr(az, name) is getattr(az.samples, name)
    from alphazero import selfplay
    assert callable(selfplay.process_samples)


def test_the_c_abi_checks_its_arguments_before_any_device(az):
    lib = az.lib
    err = lambda: lib.azmi_samples_last_error().decode()
    rec = az._capi.ResampleRecordC()
    one = (C.c_float * 8)()
    assert lib.azmi_sample_loss(one, one, 1, 0, 1.0, one, 0, None) == -1 and "M = 0" in err()
    assert lib.azmi_sample_loss(one, one, 1, (1 << 20) + 1, 1.0, one, 0, None) == -1 and "at most" in err()
    assert lib.azmi_sample_loss(one, one, (1 << 30) + 1, 7, 1.0, one, 0, None) == -1 and "at most 1073741824 rows" in err()
    assert lib.azmi_sample_loss(None, one, 1, 7, 1.0, one, 0, None) == -1 and "null argument" in err()
    assert lib.azmi_sample_loss(None, None, 0, 7, 1.0, None, 0, None) == 0      # n == 0: nothing is touched
    assert lib.azmi_resample_plan(None, 0, 5, None, None, C.byref(rec), 0, None) == 0
    assert (rec.total_loss, rec.rows_out, rec.nonfinite, rec.first_nonfinite) == (0.0, 0, 0, 0xFFFFFFFF)      # the empty plan
    assert lib.azmi_resample_plan(None, 0, 5, None, None, None, 0, None) == -1 and "null argument" in err()
    assert lib.azmi_resample_plan(one, (1 << 30) + 1, 5, one, one, C.byref(rec), 0, None) == -1 and "at most" in err()
    assert lib.azmi_resample_plan(one, 4, 5, one, None, C.byref(rec), 0, None) == -1 and "both, or neither" in err()
    ptrs = (VP * 9)(*[C.addressof(one)] * 9)
    sizes = (C.c_uint32 * 9)(*[12] * 9)
    assert lib.azmi_resample_gather(None, None, 0, 0, None, None, None, 0, None) == 0
    assert lib.azmi_resample_gather(one, one, 0, 3, ptrs, ptrs, sizes, 0, None) == 0
    assert lib.azmi_resample_gather(one, one, 4, 9, ptrs, ptrs, sizes, 0, None) == -1 and "at most 8 per call" in err()
    sizes[1] = 10
    assert lib.azmi_resample_gather(one, one, 4, 3, ptrs, ptrs, sizes, 0, None) == -1 and "array 1: a row of 10 bytes" in err()
    sizes[1] = 12
    assert lib.azmi_resample_gather(None, one, 4, 3, ptrs, ptrs, sizes, 0, None) == -1 and "null argument" in err()


def test_without_a_device_the_entry_points_fail_loudly(az):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    one = (C.c_float * 8)()
    rec = az._capi.ResampleRecordC()
    assert az.lib.azmi_sample_loss(one, one, 1, 7, 1.0, one, 0, None) == -2
    assert "azmi_sample_loss: no HIP device" in az.lib.azmi_samples_last_error().decode()
    assert az.lib.azmi_resample_plan(one, 1, 5, one, one, C.byref(rec), 0, None) == -2
    assert "azmi_resample_plan: no HIP device" in az.lib.azmi_samples_last_error().decode()


def test_sample_loss_argument_errors_come_before_any_device_call(az, monkeypatch):
    monkeypatch.setattr(az.samples, "lib", _Lib())
    t = np.full((4, 7), 1.0 / 7, np.float32)
    with pytest.raises(RuntimeError, match=r"sample_loss: target and p must have one shape, got \(4, 7\) and \(4, 6\)"):
        az.sample_loss(t, t[:, :6].copy())
    with pytest.raises(RuntimeError, match=r"one shape, got \(4, 7\) and \(3, 7\)"):
        az.sample_loss(t, t[:3])
    with pytest.raises(RuntimeError, match=r"\[n, M\] arrays, got shapes \(4, 7\) and \(7,\)"):
        az.sample_loss(t, t[0])
    with pytest.raises(RuntimeError, match=r"M must be in \[1, 2\^20\], got 0"):
        az.sample_loss(np.zeros((3, 0), np.float32), np.zeros((3, 0), np.float32))
    wide = np.broadcast_to(np.float32(0), (1, (1 << 20) + 1))
    with pytest.raises(RuntimeError, match=r"M must be in \[1, 2\^20\], got 1048577"):
        az.sample_loss(wide, wide)
    tall = np.broadcast_to(np.float32(0), ((1 << 30) + 1, 1))
    with pytest.raises(RuntimeError, match=r"sample_loss: at most 2\^30 rows, got 1073741825"):
        az.sample_loss(tall, tall)
    with pytest.raises(RuntimeError, match="target must be contiguous float32, got contiguous float64"):
        az.sample_loss(t.astype(np.float64), t)
    with pytest.raises(RuntimeError, match="p must be contiguous float32, got non-contiguous float32"):
        az.sample_loss(t, np.zeros((4, 14), np.float32)[:, ::2])
    with pytest.raises(RuntimeError, match="target must be a numpy array or a CUDA tensor, got list"):
        az.sample_loss(t.tolist(), t)
    neg = t.copy()
    neg[2, 3] = -0.25
    with pytest.raises(RuntimeError, match=r"sample_loss: a negative target: target\[2, 3\] = "):
        az.sample_loss(neg, t)
    for bad in ("one", None, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="scale must be"):
            az.sample_loss(t, t, scale=bad)
    for bad in (-1, 0.0, "0", True, None):
        with pytest.raises(RuntimeError, match="device must be a device index"):
            az.sample_loss(t, t, device=bad)
    # tensors: one kind, CUDA, one device
    with pytest.raises(RuntimeError, match="numpy arrays and tensors are mixed"):
        az.sample_loss(t, _Tensor((4, 7)))
    with pytest.raises(RuntimeError, match="p must be a CUDA tensor .* it is on cpu"):
        az.sample_loss(_Tensor((4, 7)), _Tensor((4, 7), device="cpu", is_cuda=False))
    with pytest.raises(RuntimeError, match="the arrays are on different devices: target on cuda:0, p on cuda:1"):
        az.sample_loss(_Tensor((4, 7)), _Tensor((4, 7), device="cuda:1"))
    with pytest.raises(RuntimeError, match="p must be contiguous float32, got contiguous float16"):
        az.sample_loss(_Tensor((4, 7)), _Tensor((4, 7), dtype="torch.float16"))
    with pytest.raises(RuntimeError, match="target must be contiguous float32, got non-contiguous float32"):
        az.sample_loss(_Tensor((4, 7), contiguous=False), _Tensor((4, 7)))
    with pytest.raises(RuntimeError, match=r"one shape, got \(4, 7\) and \(5, 7\)"):
        az.sample_loss(_Tensor((4, 7)), _Tensor((5, 7)))
    import torch
    with pytest.raises(RuntimeError, match="target must be a CUDA tensor"):
        az.sample_loss(torch.zeros(4, 7), torch.zeros(4, 7))


def test_resample_plan_and_rows_argument_errors_come_before_any_device_call(az, monkeypatch):
    monkeypatch.setattr(az.samples, "lib", _Lib())
    loss = np.ones(6)
    for bad in (-1, 1 << 64, 1.0, "7", None, True):
        with pytest.raises(RuntimeError, match=r"resample_plan: seed must be an integer in \[0, 2\^64\)"):
            az.resample_plan(loss, bad)
    with pytest.raises(RuntimeError, match=r"loss must be one-dimensional, got shape \(2, 3\)"):
        az.resample_plan(loss.reshape(2, 3), 1)
    with pytest.raises(RuntimeError, match="loss must be contiguous float64, got contiguous float32"):
        az.resample_plan(loss.astype(np.float32), 1)
    with pytest.raises(RuntimeError, match="loss must be contiguous float64, got non-contiguous float64"):
        az.resample_plan(np.ones(12)[::2], 1)
    with pytest.raises(RuntimeError, match=r"resample_plan: at most 2\^30 rows, got 1073741825"):
        az.resample_plan(np.broadcast_to(np.float64(0), ((1 << 30) + 1,)), 1)
    with pytest.raises(RuntimeError, match="loss must be a numpy array or a CUDA tensor, got list"):
        az.resample_plan([1.0, 2.0], 1)
    copies, offsets = np.ones(6, np.uint32), np.arange(6, dtype=np.uint64)
    x = np.zeros((6, 3), np.float32)
    with pytest.raises(RuntimeError, match=r"copies and offsets must be one-dimensional and of one length, got shapes \(6,\) and \(5,\)"):
        az.resample_rows(copies, offsets[:5], x)
    with pytest.raises(RuntimeError, match="copies must be contiguous uint32 or int32, got contiguous int64"):
        az.resample_rows(copies.astype(np.int64), offsets, x)
    with pytest.raises(RuntimeError, match="offsets must be contiguous uint64 or int64, got contiguous uint32"):
        az.resample_rows(copies, offsets.astype(np.uint32), x)
    with pytest.raises(RuntimeError, match=r"arrays\[1\] must hold one row per sample \(6\), got shape \(5, 3\)"):
        az.resample_rows(copies, offsets, x, x[:5])
    with pytest.raises(RuntimeError, match=r"arrays\[0\] must be contiguous float32, got contiguous float64"):
        az.resample_rows(copies, offsets, x.astype(np.float64))
    with pytest.raises(RuntimeError, match=r"arrays\[0\]: a row of 0 elements"):
        az.resample_rows(copies, offsets, np.zeros((6, 0), np.float32))
    with pytest.raises(RuntimeError, match="rows_out must be a row count"):
        az.resample_rows(copies, offsets, x, rows_out=-1)
    with pytest.raises(RuntimeError, match=r"the arrays are on different devices: .*arrays\[0\] on cuda:1"):
        az.resample_rows(_Tensor((6,), dtype="torch.int32"), _Tensor((6,), dtype="torch.int64"), _Tensor((6, 3), device="cuda:1"))


class _Net:
    def forward(self, *args, **kwargs):
        raise AssertionError("the net ran before the arguments were checked")


def test_resample_by_surprise_argument_errors_come_before_any_device_call(az, monkeypatch):
    from alphazero import selfplay
    monkeypatch.setattr(az.samples, "lib", _Lib())
    c, v, pi = np.zeros((5, 4, 6, 7), np.float32), np.zeros((5, 3), np.float32), np.zeros((5, 7), np.float32)
    net = _Net()
    for fn in (lambda s, **kw: az.resample_by_surprise(s, net, 1, **kw), lambda s, **kw: az.iteration_losses(s, net, **kw),
               lambda s, **kw: selfplay.process_samples(_OneSymmetry, s, net, 1, **kw),
               lambda s, **kw: selfplay.process_samples(az.Connect4GS, s, net, 1, **kw)):      # (before symmetries_batch's own checks)
        with pytest.raises(RuntimeError, match="the shapes of canonical .* do not agree"):
            fn((c, v[:4], pi))
        with pytest.raises(RuntimeError, match="the shapes of canonical .* do not agree"):
            fn((c, v, pi.reshape(5, 7, 1)))
        with pytest.raises(RuntimeError, match="samples must be the .canonical, v, pi. triple"):
            fn((c, v))
        with pytest.raises(RuntimeError, match="pi must be contiguous float32, got contiguous float64"):
            fn((c, v, pi.astype(np.float64)))
        with pytest.raises(RuntimeError, match="canonical must be contiguous float32, got non-contiguous float32"):
            fn((np.zeros((5, 4, 6, 14), np.float32)[..., ::2], v, pi))
        for bad in (0, -3, 1.5, None, True):
            with pytest.raises(RuntimeError, match="batch_rows must be an integer >= 1"):
                fn((c, v, pi), batch_rows=bad)
        with pytest.raises(RuntimeError, match="the arrays are on different devices: canonical on cuda:0, v on cuda:1, pi on cuda:0"):
            fn((_Tensor((5, 4, 6, 7)), _Tensor((5, 3), device="cuda:1"), _Tensor((5, 7))))
        with pytest.raises(RuntimeError, match="numpy arrays and tensors are mixed"):
            fn((c, v, _Tensor((5, 7))))
    for bad in (-1, 1 << 64, 0.5):
        with pytest.raises(RuntimeError, match=r"resample_by_surprise: seed must be an integer in \[0, 2\^64\)"):
            az.resample_by_surprise((c, v, pi), net, bad)
    with pytest.raises(RuntimeError, match=r"process_samples: seed must be an integer in \[0, 2\^64\)"):
        selfplay.process_samples(az.Connect4GS, (c, v, pi), net, -1)
    with pytest.raises(RuntimeError, match="net must be a HipLeafNet, got NoneType"):
        az.resample_by_surprise((c, v, pi), None, 1)
    with pytest.raises(RuntimeError, match="cv must be a number"):
        az.iteration_losses((c, v, pi), net, cv="one")


class _OneSymmetry:
    """a game without symmetries: process_samples goes straight to resample_by_surprise"""
    @staticmethod
    def NUM_SYMMETRIES():
        return 1


def test_no_samples_give_empty_results_without_a_device(az, monkeypatch):
    from alphazero import selfplay
    monkeypatch.setattr(az.samples, "lib", _Lib())
    empty = np.zeros((0, 7), np.float32)
    loss = az.sample_loss(empty, empty)
    assert loss.dtype == np.float64 and loss.shape == (0,)
    copies, offsets, rows_out, total = az.resample_plan(np.zeros(0), 9)
    assert copies.dtype == np.uint32 and offsets.dtype == np.uint64 and copies.shape == offsets.shape == (0,) and rows_out == 0 and total == 0.0
    got = az.resample_rows(copies, offsets, np.zeros((0, 4, 6, 7), np.float32), np.zeros((0, 3), np.float32))
    assert [g.shape for g in got] == [(0, 4, 6, 7), (0, 3)] and all(g.dtype == np.float32 for g in got)
    none = (np.zeros((0, 4, 6, 7), np.float32), np.zeros((0, 3), np.float32), empty)
    for (c, v, pi), loss in (az.resample_by_surprise(none, _Net(), 3), selfplay.process_samples(az.Connect4GS, none, _Net(), 3)):
        assert c.shape == (0, 4, 6, 7) and v.shape == (0, 3) and pi.shape == (0, 7) and loss.shape == (0,) and loss.dtype == np.float64
    assert az.iteration_losses(none, _Net()) == (0.0, 0.0)


def test_the_package_and_the_module_import_without_torch(az):
    code = ("import sys; sys.path.insert(0, %r); import alphazero; from alphazero import samples, selfplay; import numpy as np; "
            "alphazero.resample_plan(np.zeros(0), 1); alphazero.sample_loss(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)); "
            "print('torch' in sys.modules)" % PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "False", "the samples module pulled in torch"
