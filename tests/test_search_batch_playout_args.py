"""CPU: the PLAYOUT evaluator of the batched search: azmi_search_run_eval / play_eval / set_rollout_seeds are exported with the
declared signatures, MCTSBatch.rollout_seed is a pure function of (rollout seed, j), and the evaluator argument errors of
search() / play() are raised in Python, before any device call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p

# name -> (argument types of include/azmi.h in ctypes terms, the C parameter list the header must declare)
ENTRY_POINTS = {
    "azmi_search_run_eval": ([VP, C.c_int, VP, VP, C.c_uint32, C.c_int, VP],
                             "azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, uint32_t visits, int root_noise_enabled, "
                             "void* stream"),
    "azmi_search_play_eval": ([VP, C.c_int, VP, VP, C.c_uint32, C.c_float, C.c_uint32, C.c_int, VP],
                              "azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, uint32_t visits, float temp, "
                              "uint32_t max_moves, int root_noise, void* stream"),
    "azmi_search_set_rollout_seeds": ([VP, VP], "azmi_search* s, const uint64_t* seeds"),
}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from alphazero import _capi
    return _capi


def test_the_three_symbols_exist_with_the_declared_signatures(capi):
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
    assert capi.lib.azmi_abi_version() == 1


def _mix64(x):
    """splitmix64's finaliser of x + the golden-ratio increment, restated from its published definition"""
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def test_rollout_seed_is_a_pure_function(capi):
    import alphazero as az
    f = az.MCTSBatch.rollout_seed
    m = (1 << 64) - 1
    for rs in (0, 1, 12345, m, 0xDEADBEEFCAFEF00D):
        vals = [f(rs, j) for j in range(1000)]
        assert all(isinstance(v, int) and 0 <= v <= m for v in vals)
        assert len(set(vals)) == 1000, "the seeds of the first 1000 rollouts of a tree are not distinct"
        assert vals == [f(rs, j) for j in range(1000)]
        assert vals == [_mix64((rs + 0x9E3779B97F4A7C15 * (j + 1)) & m) for j in range(1000)]
    assert max(f(rs, 0) for rs in range(64)) > 1 << 63, "64-bit values"
    assert f(m + 1 + 5, 3) == f(5, 3)                          # the seed is taken mod 2^64, like MCTSBatch's seeds
    with pytest.raises(RuntimeError, match="counts from 0"):
        f(1, -1)


class _Lib:
    """stands in for libazmi: any call is a device call the argument checks must come before"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called before the evaluator arguments were checked")


def test_evaluator_argument_errors_come_before_any_device_call(capi, monkeypatch):
    import alphazero as az
    mb = object.__new__(az.MCTSBatch)                          # no device: the checks below need none
    mb._h = None
    monkeypatch.setattr(az.search_batch, "lib", _Lib())
    net, cache = object(), object()
    for call in (mb.search, mb.play):
        with pytest.raises(RuntimeError, match="takes no cache"):
            call(8, cache=cache, evaluator="playout")
        with pytest.raises(RuntimeError, match="'playout' takes no net"):
            call(8, net=net, evaluator="playout")
        with pytest.raises(RuntimeError, match="'random' takes no net"):
            call(8, net=net, evaluator=az.EvalType.RANDOM)
        with pytest.raises(RuntimeError, match="'net' needs a net"):
            call(8, evaluator="net")
        with pytest.raises(RuntimeError, match="evaluator must be"):
            call(8, evaluator="rollout")
        with pytest.raises(RuntimeError, match="evaluator must be"):
            call(8, evaluator=2)
    ev = az.MCTSBatch._evaluator
    assert ev("search", None, None, None) == az.EvalType.RANDOM and ev("search", None, net, cache) == az.EvalType.NN
    assert ev("search", "playout", None, None) == ev("play", az.EvalType.PLAYOUT, None, None) == az.EvalType.PLAYOUT
    assert ev("search", "random", None, cache) == az.EvalType.RANDOM      # (a cache without a net is ignored, as before)
