"""CPU: the argument checks of `MCTSBatch.expand_frontier` and `alphazero.build_opening_tree` that are made on the host before any
device is touched, the temperature schedule, the seed rule, and the two C entry points without a handle."""
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


def _batch(az, n=4):
    """An MCTSBatch without a device: only the fields the host-side checks read."""
    mb = object.__new__(az.MCTSBatch)
    mb._h, mb._n, mb._P, mb._M, mb._chw, mb._k, mb._dl, mb._rows, mb._gumbel = None, n, 2, 7, (4, 6, 7), 1, 1, None, False
    return mb


@pytest.mark.parametrize("reach,temp,min_reach,cap,match", [
    ([1.0] * 3, 1.0, 0.01, None, r"reach: one per tree \(4\)"),
    ([[1.0] * 4], 1.0, 0.01, None, r"reach: one per tree \(4\)"),
    ("abcd", 1.0, 0.01, None, r"reach must be 4 numbers"),
    ([1.0, -0.5, 1.0, 1.0], 1.0, 0.01, None, r"reach must be finite and not negative"),
    ([1.0, float("nan"), 1.0, 1.0], 1.0, 0.01, None, r"reach must be finite and not negative"),
    ([1.0, float("inf"), 1.0, 1.0], 1.0, 0.01, None, r"reach must be finite and not negative"),
    ([1.0] * 4, [1.0] * 5, 0.01, None, r"temp: a number or one per tree \(4\)"),
    ([1.0] * 4, "hot", 0.01, None, r"temp must be a number or 4 numbers"),
    ([1.0] * 4, -1.0, 0.01, None, r"temp must be finite and not negative"),
    ([1.0] * 4, [1.0, 1.0, float("nan"), 1.0], 0.01, None, r"temp must be finite and not negative"),
    ([1.0] * 4, 1.0, 0.0, None, r"min_reach must be a positive finite number"),
    ([1.0] * 4, 1.0, -0.01, None, r"min_reach must be a positive finite number"),
    ([1.0] * 4, 1.0, float("nan"), None, r"min_reach must be a positive finite number"),
    ([1.0] * 4, 1.0, float("inf"), None, r"min_reach must be a positive finite number"),
    ([1.0] * 4, 1.0, "0.01", None, r"min_reach must be a positive finite number"),
    ([1.0] * 4, 1.0, True, None, r"min_reach must be a positive finite number"),
    ([1.0] * 4, 1.0, 0.01, 0, r"max_children must be an integer in \[1, 2\^32\)"),
    ([1.0] * 4, 1.0, 0.01, -3, r"max_children must be an integer in \[1, 2\^32\)"),
    ([1.0] * 4, 1.0, 0.01, 2 ** 32, r"max_children must be an integer in \[1, 2\^32\)"),
    ([1.0] * 4, 1.0, 0.01, 2.5, r"max_children must be an integer in \[1, 2\^32\)"),
    ([1.0] * 4, 1.0, 0.01, True, r"max_children must be an integer in \[1, 2\^32\)"),
])
def test_expand_frontier_argument_errors_are_raised_by_name(az, reach, temp, min_reach, cap, match):
    with pytest.raises(RuntimeError, match="expand_frontier: " + match):
        _batch(az).expand_frontier(reach, temp, min_reach, cap)


def test_expand_frontier_accepted_arguments(az):
    """a scalar temp is one value per tree, max_children defaults to n * M, numpy scalars pass"""
    mb = _batch(az)
    r, t, mr, cap = mb._frontier_args([1.0, 0.0, 0.5, 1e-3], 0.37, np.float32(0.25), None)
    assert r.dtype == np.float64 and t.dtype == np.float64 and t.tolist() == [0.37] * 4 and mr == 0.25 and cap == 4 * 7
    r, t, mr, cap = mb._frontier_args(np.ones(4, np.float32), [0, 1, 0.37, 2.5], 1, np.int64(5))
    assert t.tolist() == [0.0, 1.0, 0.37, 2.5] and mr == 1.0 and cap == 5 and isinstance(cap, int)


def _tree(az, **kw):
    args = dict(game=az.Connect4GS, start_state=az.Connect4GS(), sims=8)
    args.update(kw)
    return az.build_opening_tree(args.pop("game"), args.pop("start_state"), args.pop("sims"), **args)


@pytest.mark.parametrize("kw,match", [
    (dict(game=7), r"game must be a game class or a state of one"),
    (dict(game=object), r"game must be a game class or a state of one"),
    (dict(start_state=None), r"start_state must be a state of the tree's game"),
    (dict(sims=0), r"sims must be an integer >= 1"),
    (dict(sims=2.0), r"sims must be an integer >= 1"),
    (dict(sims=True), r"sims must be an integer >= 1"),
    (dict(batch=0), r"batch must be an integer >= 1"),
    (dict(batch="8"), r"batch must be an integer >= 1"),
    (dict(max_depth=-1), r"max_depth must be an integer >= 0"),
    (dict(seed=1.5), r"seed must be an integer"),
    (dict(min_reach=0.0), r"min_reach must be a finite positive number"),
    (dict(min_reach=float("nan")), r"min_reach must be a finite positive number"),
    (dict(start_temp=-1.0), r"start_temp must be a finite non-negative number"),
    (dict(final_temp=float("inf")), r"final_temp must be a finite non-negative number"),
    (dict(half_life="ten"), r"half_life must be a finite non-negative number"),
    (dict(max_simulations=100), r"max_simulations is set by the builder"),
    (dict(seeds=[1, 2]), r"seeds is set by the builder"),
    (dict(evaluator="net"), r"evaluator 'net' needs a net"),
    (dict(evaluator="mcts"), r"evaluator must be None, 'net', 'random', 'playout' or an EvalType"),
    (dict(evaluator="playout", cache=object()), r"evaluator 'playout' takes no cache"),
    (dict(evaluator="random", net=object()), r"evaluator 'random' takes no net"),
])
def test_build_opening_tree_argument_errors_are_raised_by_name(az, kw, match):
    with pytest.raises(RuntimeError, match="build_opening_tree: " + match):
        _tree(az, **kw)


def test_start_state_of_another_game_is_refused(az):
    with pytest.raises(RuntimeError, match="start_state must be a state of the tree's game"):
        az.build_opening_tree(az.Connect4GS, az.BrandubhGS(), 8)
    with pytest.raises(RuntimeError, match="start_state must be a state of the tree's game"):
        az.build_opening_tree(az.BrandubhGS(), az.Connect4GS(), 8)      # a state stands for its class


def test_temperature_schedule_is_the_reference_expression(az):
    """opening_analysis.py:167-172: final + (start - final) * exp(-(0.693 / max(1, half_life)) * depth), ln 2 written as 0.693"""
    from alphazero.opening_tree import temperature_at_depth
    for start, final, hl in ((1.0, 0.2, 10), (1.5, 0.0, 3), (0.5, 0.5, 7), (1.0, 0.2, 0), (1.0, 0.2, 0.25)):
        for d in (0, 1, 2, 9, 10, 37, 1000):
            want = final + (start - final) * math.exp(-(0.693 / max(1, hl)) * d)
            assert temperature_at_depth(d, start, final, hl) == want
    assert temperature_at_depth(0) == 1.0 and temperature_at_depth(10 ** 6) == 0.2
    assert abs(temperature_at_depth(10) - 0.6) < 1e-3, "half way after one half life (0.693 for ln 2)"
    assert temperature_at_depth(3, half_life=0) == temperature_at_depth(3, half_life=1)


def test_node_seed_is_mix64_of_seed_plus_index(az):
    from alphazero.opening_tree import node_seed
    mask = 0xFFFFFFFFFFFFFFFF
    for seed, b in ((0, 0), (0, 1), (7, 12), (mask, 1), (mask - 2, 5), (-1, 3)):
        assert node_seed(seed, b) == az.MCTSBatch._mix64((seed + b) & mask)
    assert node_seed(mask, 1) == node_seed(0, 0), "the sum wraps at 64 bits"
    assert node_seed(0, 0) == 0xE220A8397B1DCDAF, "mix64(0): splitmix64's first output"
    assert len({node_seed(3, b) for b in range(1000)}) == 1000
    assert az.build_opening_tree is not None and az.OpeningTree is not None and az.temperature_at_depth is not None


def test_library_entry_points_without_a_handle(az):
    """A NULL handle is what a caller holds whose create failed: without a device the two calls repeat the no-device error, as
    the move entry points do (include/azmi.h); both are part of the ABI _capi declares."""
    import ctypes as C
    from alphazero import _capi
    lib = _capi.lib
    vp = C.c_void_p
    assert _capi.SYMBOLS["azmi_search_expand"] == (C.c_int, [vp, vp, vp, C.c_double, C.c_uint32, vp])
    assert _capi.SYMBOLS["azmi_search_frontier"] == (C.c_int, [vp] * 16)
    no_device = lib.azmi_device_count() <= 0
    reach = np.ones(1); temp = np.ones(1)
    rc = lib.azmi_search_expand(None, reach.ctypes.data, temp.ctypes.data, 0.01, 7, None)
    assert rc == (-2 if no_device else -1), lib.azmi_last_error().decode()
    assert ("no HIP device" if no_device else "null") in lib.azmi_last_error().decode()
    rc = lib.azmi_search_frontier(None, *([None] * 15))
    assert rc == (-2 if no_device else -1), lib.azmi_last_error().decode()
    assert ("no HIP device" if no_device else "null") in lib.azmi_last_error().decode()
    assert lib.azmi_abi_version() == 1          # the entry points are additive
