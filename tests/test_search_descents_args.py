"""CPU: the argument checks of `alphazero.MCTSBatch(..., descents_per_step=L)` / azmi_search_set_descents_per_step that are made
on the host before any device is touched."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


@pytest.mark.parametrize("v", [0, 257, True, 2.5, -1, "8", None])
def test_descents_per_step_out_of_range_or_not_an_integer_is_refused(az, v):
    with pytest.raises(RuntimeError, match=r"descents_per_step must be an integer in \[1, 256\]"):
        az.MCTSBatch(az.Connect4GS, 4, 1.25, max_simulations=10, descents_per_step=v)


def test_descents_with_several_leaves_per_step_is_refused_by_name(az):
    with pytest.raises(RuntimeError, match=r"descents_per_step = 2 with leaves_per_step = 2"):
        az.MCTSBatch(az.Connect4GS, 4, 1.25, max_simulations=10, descents_per_step=2, leaves_per_step=2)


def test_accepted_values_reach_the_library(az):
    """1, 256 and a numpy integer pass the host checks: what fails next is the library's own first check (its message about
    the missing max_simulations, which it makes before it looks for a device)."""
    for v in (1, 256, np.int64(8)):
        with pytest.raises(RuntimeError, match="max_simulations is required"):
            az.MCTSBatch(az.Connect4GS, 4, 1.25, max_simulations=0, descents_per_step=v)


def test_library_entry_points_check_their_arguments(az):
    from alphazero import _capi
    lib = _capi.lib
    assert lib.azmi_search_set_descents_per_step(None, 8) == -1
    assert "null" in lib.azmi_last_error().decode()
    assert lib.azmi_search_host_reads(None, None) == -1
    assert lib.azmi_abi_version() == 1          # the entry points are additive


def _batch(az, L):
    """An MCTSBatch without a device: only the fields the host-side checks of the refused calls read."""
    mb = object.__new__(az.MCTSBatch)
    mb._h, mb._n, mb._P, mb._M, mb._chw, mb._k, mb._dl, mb._rows, mb._gumbel = None, 4, 2, 7, (4, 6, 7), 1, L, None, False
    return mb


def test_step_api_and_search_to_are_refused_by_name_before_any_device_call(az):
    mb = _batch(az, 8)
    assert mb.descents_per_step == 8
    with pytest.raises(RuntimeError, match=r"search_to with descents_per_step = 8"):
        mb.search_to(12)
    with pytest.raises(RuntimeError, match=r"find_leaves with descents_per_step = 8"):
        mb.find_leaves()
    with pytest.raises(RuntimeError, match=r"process_results with descents_per_step = 8"):
        mb.process_results(np.zeros((0, 3), np.float32), np.zeros((0, 7), np.float32))
