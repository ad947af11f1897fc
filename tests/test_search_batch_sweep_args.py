"""CPU: search to per-tree visit targets: azmi_search_run_to / azmi_search_checkpoints are exported with the declared signatures,
and every argument error of MCTSBatch.search_to() / checkpoints() is raised in Python, before any device call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p

# name -> (argument types of include/azmi.h in ctypes terms, the C parameter list the header must declare)
ENTRY_POINTS = {
    "azmi_search_run_to": ([VP, C.c_int, VP, VP, VP, VP, C.c_uint32, C.c_float, C.c_int, C.c_int, VP],
                           "azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, const uint32_t* targets, "
                           "const uint32_t* checkpoints, uint32_t n_checkpoints, float temp, int pruned, int root_noise_enabled, "
                           "void* stream"),
    "azmi_search_checkpoints": ([VP, VP, VP, VP, VP, VP, VP],
                                "azmi_search* s, uint32_t* taken_mask, uint32_t* root_n, uint32_t* counts, float* probs, "
                                "float* root_values, float* root_q"),
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
    assert capi.lib.azmi_abi_version() == 1


class _Lib:
    """stands in for libazmi: any call is a device call the argument checks must come before"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called before the arguments were checked")


def _batch(az, n=3, gumbel=False):
    mb = object.__new__(az.MCTSBatch)                          # no device: the checks below need none
    mb._h, mb._n, mb._M, mb._P, mb._chw, mb._gumbel = None, n, 7, 2, (4, 6, 7), gumbel
    return mb


def test_argument_errors_come_before_any_device_call(capi, monkeypatch):
    import alphazero as az
    monkeypatch.setattr(az.search_batch_sweep, "lib", _Lib())
    mb = _batch(az)
    with pytest.raises(RuntimeError, match=r"one target per tree \(3\)"):
        mb.search_to([5, 5])
    with pytest.raises(RuntimeError, match=r"one target per tree \(3\)"):
        mb.search_to([5, 5, 5, 5])
    with pytest.raises(RuntimeError, match="targets must be"):
        mb.search_to([5, -1, 5])
    with pytest.raises(RuntimeError, match="targets must be"):
        mb.search_to(-3)
    with pytest.raises(RuntimeError, match="at most 32 checkpoints"):
        mb.search_to(100, checkpoints=range(1, 34))
    with pytest.raises(RuntimeError, match="strictly ascending"):
        mb.search_to(10, checkpoints=(1, 4, 4))
    with pytest.raises(RuntimeError, match="strictly ascending"):
        mb.search_to(10, checkpoints=(4, 1))
    with pytest.raises(RuntimeError, match="positive"):
        mb.search_to(10, checkpoints=(0, 4))
    with pytest.raises(RuntimeError, match="checkpoints: no search_to call"):
        mb.checkpoints()
    # the evaluator errors are search()'s
    with pytest.raises(RuntimeError, match="takes no cache"):
        mb.search_to(8, cache=object(), evaluator="playout")
    with pytest.raises(RuntimeError, match="'net' needs a net"):
        mb.search_to(8, evaluator="net")
    with pytest.raises(RuntimeError, match="'random' takes no net"):
        mb.search_to(8, net=object(), evaluator="random")
    # 32 ascending checkpoints and n targets pass the checks: the stand-in is reached
    with pytest.raises(AssertionError, match="azmi_search_run_to was called"):
        mb.search_to([0, 5, 2 ** 32 - 1], checkpoints=range(1, 33))


def test_a_gumbel_batch_is_refused_with_the_reason(capi, monkeypatch):
    import alphazero as az
    monkeypatch.setattr(az.search_batch_sweep, "lib", _Lib())
    with pytest.raises(RuntimeError, match="Gumbel.*sequential halving plans a fixed budget"):
        _batch(az, gumbel=True).search_to(10)
