"""The argument checks the package's entry points share.  Each takes the value and the finished error text (device_index and
seed64, whose texts differ in the caller's name alone, take that name), raises RuntimeError(text) and returns the value as a plain
int or float, so a caller's errors keep their own words and their own order."""
import numpy as np


def integer(x, text, lo=None, hi=None):
    """x: an int or a numpy integer, never a bool, with lo <= x <= hi (None: no bound on that side) -> int(x)"""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise RuntimeError(text)
    v = int(x)
    if (lo is not None and v < lo) or (hi is not None and v > hi):
        raise RuntimeError(text)
    return v


def device_index(x, what):
    return integer(x, f"{what}: device must be a device index, got {x!r}", 0)


def seed64(x, what):
    return integer(x, f"{what}: seed must be an integer in [0, 2^64), got {x!r}", 0, (1 << 64) - 1)


def unit_fraction(x, text):
    """x: an int, float or numpy real, never a bool, with 0 < x <= 1 (a NaN fails both) -> float(x)"""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not (0 < x <= 1):
        raise RuntimeError(text)
    return float(x)


def number(x, text, positive=False):
    """x: a finite int, float or numpy real, never a bool, x >= 0 (positive: x > 0) -> float(x)"""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x) or x < 0 or (positive and not x > 0):
        raise RuntimeError(text)
    return float(x)


def is_tensor(x):
    """a torch tensor (the check imports nothing: the numpy-only callers never load torch)"""
    return hasattr(x, "is_cuda") and hasattr(x, "data_ptr")


def is_device_tensor(x):
    """a torch tensor in device memory (a CPU tensor is a host array like any other)"""
    return is_tensor(x) and bool(x.is_cuda)


def device_tensor(x, what, name, dtypes, shape, device):
    """x: a contiguous CUDA tensor on device index `device` whose dtype is one of `dtypes` (names as str(dtype) prints them, e.g.
    "torch.float32") and whose shape is `shape` (None: any length on that axis) -> x.  Every failure is RuntimeError
    "<what>: <name> ..."; nothing touches the device.  Dtype, shape and contiguity are judged first, then where the tensor lives."""
    if not is_tensor(x):
        raise RuntimeError(f"{what}: {name} must be a CUDA tensor like the keys (host and device arguments do not mix), got {type(x).__name__}")
    if str(x.dtype) not in dtypes:
        raise RuntimeError(f"{what}: {name} must be {' or '.join(d.split('.')[-1] for d in dtypes)}, got {str(x.dtype).split('.')[-1]}")
    got = tuple(x.shape)
    if len(got) != len(shape) or any(s is not None and s != g for s, g in zip(shape, got)):
        want = "[" + ", ".join("n" if s is None else str(s) for s in shape) + "]"
        raise RuntimeError(f"{what}: {name} must have shape {want}, got {list(got)}")
    if not x.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be contiguous")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: {name} must be a CUDA tensor like the keys (host and device arguments do not mix), got a {x.device} tensor")
    if x.device.index != device:
        raise RuntimeError(f"{what}: {name} is on {x.device}, the cache on cuda:{device}")
    return x
