"""CPU: the batched search's move entry points (azmi_search_pick_moves / update_roots / root_prior / play / game_state) are
exported with the declared signatures, the ABI version is unchanged, and without a device every one of them fails with the
project's no-device error instead of crashing."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p

# name -> (argument types of include/azmi.h in ctypes terms, the C parameter list the header must declare)
ENTRY_POINTS = {
    "azmi_search_pick_moves": ([VP, C.c_float, VP, VP], "azmi_search* s, float temp, int32_t* host_moves, void* stream"),
    "azmi_search_update_roots": ([VP, VP, VP], "azmi_search* s, const int32_t* host_moves, void* stream"),
    "azmi_search_root_prior": ([VP, C.c_int, C.c_int, VP], "azmi_search* s, int apply_temp, int add_noise, void* stream"),
    "azmi_search_play": ([VP, VP, VP, C.c_uint32, C.c_float, C.c_uint32, C.c_int, VP],
                         "azmi_search* s, azmi_net* net, azmi_cache* cache, uint32_t visits, float temp, uint32_t max_moves, "
                         "int root_noise, void* stream"),
    "azmi_search_game_state": ([VP, VP, VP, VP, VP],
                               "azmi_search* s, int32_t* status, uint32_t* log_len, int32_t* log, float* final_scores"),
}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from alphazero import _capi
    return _capi


def _null_call(lib, name):
    args = {"azmi_search_pick_moves": (None, 1.0, None, None), "azmi_search_update_roots": (None, None, None),
            "azmi_search_root_prior": (None, 1, 1, None), "azmi_search_play": (None, None, None, 8, 1.0, 2, 0, None),
            "azmi_search_game_state": (None, None, None, None, None)}[name]
    return getattr(lib, name)(*args)


def test_the_five_symbols_exist_with_the_declared_signatures(capi):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "azmi.h")).read(), flags=re.S)
    raw = C.CDLL(capi.LIB_PATH)
    for name, (argtypes, params) in ENTRY_POINTS.items():
        assert hasattr(raw, name), f"{name} is not exported by libazmi.so"
        assert name in capi.SYMBOLS, f"{name} is missing from _capi.SYMBOLS"
        res, args = capi.SYMBOLS[name]
        assert res is C.c_int and list(args) == argtypes, f"{name}: _capi declares {args}"
        fn = getattr(capi.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/azmi.h"
        assert " ".join(m.group(1).split()) == params, f"{name}: the header declares ({' '.join(m.group(1).split())})"


def test_abi_version_is_unchanged(capi):
    assert capi.lib.azmi_abi_version() == 1
    assert re.search(r"#define\s+AZMI_ABI_VERSION\s+1\b", open(os.path.join(ROOT, "include", "azmi.h")).read())


def test_mctsbatch_has_the_move_methods(capi):
    import alphazero as az
    for name in ("pick_moves", "update_roots", "add_root_noise", "apply_root_policy_temp", "play", "finished", "move_logs",
                 "final_scores", "states"):
        assert callable(getattr(az.MCTSBatch, name, None)), name
    assert "No move is played" not in az.MCTSBatch.__doc__


def test_without_a_device_the_calls_fail_with_the_no_device_error(capi):
    """No device: no batch can exist, and the entry points say so for the handle a failed create leaves (NULL).  With a device
    the same NULL handle is an invalid argument.  Either way an error code and a message, never a crash."""
    import alphazero as az
    lib = capi.lib
    if lib.azmi_device_count() > 0:
        for name in ENTRY_POINTS:
            assert _null_call(lib, name) == -1, name          # AZMI_ERR_INVALID
            assert b"null argument" in lib.azmi_last_error()
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        az.MCTSBatch(az.Connect4GS, 4, 1.25, max_simulations=64)
    for name in ENTRY_POINTS:
        assert _null_call(lib, name) == -2, name              # AZMI_ERR_NO_DEVICE
        assert b"no HIP device" in lib.azmi_last_error(), name
        with pytest.raises(RuntimeError, match="no HIP device"):
            capi.check(_null_call(lib, name))
