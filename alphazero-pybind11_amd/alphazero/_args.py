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
