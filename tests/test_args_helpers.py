"""CPU: alphazero/_args.py, the argument checks the entry points share, at the smallest inputs at which each can go wrong.  The
module is loaded from its file: no library, no device."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = "what: x must be what the caller says, got it"
NOT_INTEGERS = (True, False, 1.0, "1", None, np.float64(1.0), np.bool_(True), [1])


@pytest.fixture(scope="module")
def args():
    spec = importlib.util.spec_from_file_location("_args_alone", os.path.join(ROOT, "alphazero-pybind11_amd", "alphazero", "_args.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _raises(f, *a, text=TEXT, **kw):
    with pytest.raises(RuntimeError) as e:
        f(*a, **kw)
    assert str(e.value) == text, "the text raised is not the text passed in"


def test_integer_accepts_the_bounds_and_numpy_scalars(args):
    lo, hi = 1, 64
    for x in (lo, hi, np.int32(lo), np.uint8(hi), np.int64(7)):
        got = args.integer(x, TEXT, lo, hi)
        assert type(got) is int and got == int(x)
    for x in (0, 2 ** 64 - 1, np.uint64(2 ** 64 - 1), -5, 2 ** 70):
        if x in (0, 2 ** 64 - 1):
            assert args.integer(x, TEXT, 0, 2 ** 64 - 1) == int(x)
        assert args.integer(x, TEXT) == int(x)                      # no bound on either side
    assert args.integer(0, TEXT, lo=0) == 0 and args.integer(2 ** 64, TEXT, lo=0) == 2 ** 64
    assert args.integer(-3, TEXT, hi=-3) == -3


def test_integer_rejects_bools_other_types_and_the_neighbours_of_the_bounds(args):
    lo, hi = 1, 64
    for x in NOT_INTEGERS:
        _raises(args.integer, x, TEXT, lo, hi)
        _raises(args.integer, x, TEXT)
    for x in (lo - 1, hi + 1, np.int64(lo - 1), np.int64(hi + 1), -1):
        _raises(args.integer, x, TEXT, lo, hi)
    _raises(args.integer, -1, TEXT, lo=0)
    _raises(args.integer, -2, TEXT, hi=-3)
    _raises(args.integer, 2 ** 64, TEXT, 0, 2 ** 64 - 1)
    _raises(args.integer, np.int8(-1), TEXT, 0, 2 ** 64 - 1)        # a signed numpy scalar against a bound past its range


def test_device_index(args):
    for x in (0, 1, 7, np.int32(3), 2 ** 64 - 1):
        got = args.device_index(x, "f")
        assert type(got) is int and got == int(x)
    for x in NOT_INTEGERS + (-1, np.int64(-1)):
        _raises(args.device_index, x, "f", text=f"f: device must be a device index, got {x!r}")
    _raises(args.device_index, -1, "another_f", text="another_f: device must be a device index, got -1")


def test_seed64(args):
    for x in (0, 1, 2 ** 64 - 1, np.uint64(2 ** 64 - 1), np.int64(5)):
        got = args.seed64(x, "f")
        assert type(got) is int and got == int(x)
    for x in NOT_INTEGERS + (-1, 2 ** 64, np.int64(-1)):
        _raises(args.seed64, x, "f", text=f"f: seed must be an integer in [0, 2^64), got {x!r}")


def test_number_accepts_finite_reals(args):
    for x in (0, 0.0, 1, 2 ** 64 - 1, 0.25, np.float32(0.25), np.float64(1e300), np.int64(3), np.uint8(0)):
        got = args.number(x, TEXT)
        assert type(got) is float and got == float(x)
    for x in (1, 1e-300, np.float32(0.25), np.int64(2 ** 62)):
        assert args.number(x, TEXT, positive=True) == float(x)


def test_number_rejects_bools_other_types_and_what_is_not_finite_or_negative(args):
    for positive in (False, True):
        for x in (True, False, "1", None, 1j, [1.0], np.bool_(True), float("nan"), float("inf"), -float("inf"), np.float32("nan"),
                  np.float64("inf"), -0.1, -1, np.int64(-1), np.float32(-0.1)):
            _raises(args.number, x, TEXT, positive=positive)
    for x in (0, 0.0, -0.0, np.float32(0), np.int64(0)):
        assert args.number(x, TEXT) == 0.0
        _raises(args.number, x, TEXT, positive=True)
