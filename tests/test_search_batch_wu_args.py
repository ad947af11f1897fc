"""CPU: the argument checks of `alphazero.MCTSBatch(..., leaves_per_step=K)` / azmi_search_set_leaves_per_step that are made on
the host before any device is touched."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


@pytest.mark.parametrize("k", [0, 65, -1, 2.0, 8.5, "8", None, True])
def test_leaves_per_step_out_of_range_or_not_an_integer_is_refused(az, k):
    with pytest.raises(RuntimeError, match=r"leaves_per_step must be an integer in \[1, 64\]"):
        az.MCTSBatch(az.Connect4GS, 4, 2.0, max_simulations=100, leaves_per_step=k)


def test_gumbel_with_several_leaves_per_step_is_refused_by_name(az):
    with pytest.raises(RuntimeError, match=r"leaves_per_step = 8 with gumbel_enabled.*plain PUCT"):
        az.MCTSBatch(az.Connect4GS, 4, 2.0, gumbel_enabled=True, max_simulations=100, leaves_per_step=8)


def test_accepted_values_reach_the_library(az):
    """1, 64 and a numpy integer pass the host checks: what fails next is the library's own first check (here: its message
    about the missing max_simulations, which it makes before it looks for a device)."""
    for k in (1, 64, np.int64(8)):
        with pytest.raises(RuntimeError, match="max_simulations is required"):
            az.MCTSBatch(az.Connect4GS, 4, 2.0, max_simulations=0, leaves_per_step=k)


def test_library_entry_point_checks_its_arguments(az):
    from alphazero import _capi
    lib = _capi.lib
    assert lib.azmi_search_set_leaves_per_step(None, 8) == -1
    assert "null" in lib.azmi_last_error().decode()
    assert lib.azmi_abi_version() == 1          # the entry point is additive


def _pending(az, rows, k):
    """An MCTSBatch as find_leaves() leaves it, without a device: only the fields the host-side shape check reads."""
    mb = object.__new__(az.MCTSBatch)
    mb._h, mb._n, mb._P, mb._M, mb._k, mb._rows = None, 4, 2, 7, k, rows
    return mb


def test_process_results_names_the_row_count_of_the_step(az):
    mb = _pending(az, 19, 8)                    # 4 trees x 8 descents gave 19 rows
    assert mb.leaves_per_step == 8
    with pytest.raises(RuntimeError, match=r"the step has 19 rows: v must be \[19, 3\] and pi \[19, 7\], got \(4, 3\) and \(4, 7\)"):
        mb.process_results(np.zeros((4, 3), np.float32), np.zeros((4, 7), np.float32))
    with pytest.raises(RuntimeError, match=r"the step has 19 rows"):
        mb.process_results(np.zeros((19, 3), np.float32), np.zeros((32, 7), np.float32))
    with pytest.raises(RuntimeError, match=r"the step has 0 rows: v must be \[0, 3\]"):
        _pending(az, 0, 8).process_results(np.zeros((1, 3), np.float32), np.zeros((1, 7), np.float32))
    with pytest.raises(RuntimeError, match="no leaf batch is pending"):
        _pending(az, None, 8).process_results(np.zeros((0, 3), np.float32), np.zeros((0, 7), np.float32))
