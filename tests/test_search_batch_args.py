"""CPU: the argument checks of the batched search (azmi_search_*, alphazero.MCTSBatch) that are made on the host before any
device is touched, and the ABI's additive shape."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


def _cfg(az, **kw):
    from alphazero import _capi
    base = dict(cpuct=2.0, num_players=2, num_moves=7, epsilon=0.0, root_policy_temp=1.0, fpu_reduction=0.0, relative_values=0,
                root_fpu_zero=0, shaped_dirichlet=0, gumbel_enabled=0, gumbel_m=16, gumbel_c_visit=50.0, gumbel_c_scale=1.0,
                gumbel_full=0, max_simulations=100)
    base.update(kw)
    return _capi.MctsConfigC(*[base[k] for k in ("cpuct", "num_players", "num_moves", "epsilon", "root_policy_temp", "fpu_reduction",
                                                 "relative_values", "root_fpu_zero", "shaped_dirichlet", "gumbel_enabled", "gumbel_m",
                                                 "gumbel_c_visit", "gumbel_c_scale", "gumbel_full", "max_simulations")])


def _create(az, game, cfg, n):
    from alphazero import _capi
    h = C.c_void_p()
    rc = _capi.lib.azmi_search_create(game, None if cfg is None else C.byref(cfg), n, 0, C.byref(h))
    msg = _capi.lib.azmi_last_error().decode()
    if rc == 0:
        _capi.lib.azmi_search_destroy(h)
    return rc, msg


def test_create_rejects_bad_arguments_before_touching_a_device(az):
    rc, msg = _create(az, 0, None, 4)
    assert rc == -1 and "null" in msg
    rc, msg = _create(az, 0, _cfg(az), 0)
    assert rc == -1 and "n_trees" in msg
    rc, msg = _create(az, 0, _cfg(az, max_simulations=0), 4)
    assert rc == -1 and "max_simulations is required" in msg
    rc, msg = _create(az, 99, _cfg(az), 4)
    assert rc == -1 and "unknown game" in msg
    rc, msg = _create(az, 0, _cfg(az, num_moves=8), 4)
    assert rc == -1 and "do not match the game" in msg
    rc, msg = _create(az, 1, _cfg(az, num_moves=az.TawlbwrddGS.NUM_MOVES(), max_simulations=8001), 4)
    assert rc == -1 and "8000" in msg
    rc, msg = _create(az, 0, _cfg(az, relative_values=1), 4)
    assert rc == -1 and "relative_values" in msg


def test_null_handles_are_errors_not_crashes(az):
    from alphazero import _capi
    lib = _capi.lib
    n = C.c_uint32()
    assert lib.azmi_search_reset(None, None, 0, None, None, None) == -1
    assert lib.azmi_search_find_leaves(None, None, None, None, C.byref(n)) == -1
    assert lib.azmi_search_process_results(None, None, None, 0, None) == -1
    assert lib.azmi_search_run(None, None, None, 10, 0, None) == -1
    assert lib.azmi_search_query(None, 0, 0.0, 0, None, None) == -1
    assert lib.azmi_search_sync(None) == -1
    assert lib.azmi_search_stats(None, None) == -1
    lib.azmi_search_destroy(None)
    assert lib.azmi_abi_version() == 1          # the batched search is additive


def test_python_class_reports_the_library_message(az):
    with pytest.raises(RuntimeError, match="max_simulations is required"):
        az.MCTSBatch(az.Connect4GS, 4, 2.0, max_simulations=0)
    with pytest.raises(RuntimeError, match="n_trees"):
        az.MCTSBatch(az.Connect4GS, 0, 2.0, max_simulations=10)
    with pytest.raises(TypeError):
        az.MCTSBatch(az.Connect4GS, 4, 2.0)      # max_simulations is a required keyword
