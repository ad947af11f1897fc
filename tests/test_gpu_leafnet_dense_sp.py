"""The dense spatial-head tile on the device (csrc/leafnet_dense_sp.h: DenseNet trunk, spatial policy head with global actions,
7x7 / 11x11 / 13x13, bf16 matrix cores): against the reference NNArch's own outputs (tests/golden/nn_sg_dense_4x16_k3.npz) and
the fp64 forward of tests/leafnet_ref.py, with the fp32 tier beside it on the same nets.

The bounds are the project's own: leafnet_ref.TOL (1e-3) for a bf16 tile, TOL_F32 (1e-5) for the fp32 tier.

Measured on an MI355X, max |error| of the bf16 tile: fixture dv 7.0e-6 dpi 2.1e-6; output layers x4 against fp64
dv 2.9e-5, dpi spatial 2.7e-6, global 5.6e-4; the case table (output layers x8) dv <= 1.3e-4, dpi <= 4.7e-4; all-zero / all-one /
one-cell boards dv 4.1e-5 dpi 4.3e-4.
"""
import numpy as np
import pytest
import torch

import leafnet_dense_ref as dr
import leafnet_dense_sp_ref as sr
import leafnet_ref as lr
from test_gpu_search_batch import az  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPATIAL = 1690          # 10 x 13 x 13 spatial logits of the fixture net, 19 global actions behind them


@pytest.fixture(scope="module")
def peaked():
    """(deep copy of the fixture net with its output layers x4, the fixture's inputs, fp64 v, fp64 pi) - shared, not to be changed"""
    net, x, _, _ = dr.fixture("sg_dense")
    pk = sr.peaked(net, 4.0)
    v_ref, pi_ref, _ = lr.reference(pk, x)
    return pk, x, v_ref, pi_ref


@pytest.fixture(scope="module")
def hip(peaked):
    """HipLeafNet of (fixture, "sg_dense_peaked" or case name, precision), built once"""
    import alphazero
    made = {}

    def get(name, precision):
        if (name, precision) not in made:
            net = peaked[0] if name == "sg_dense_peaked" else dr.fixture(name)[0] if name in dr.FIXTURES else sr.make_net(sr.BY_NAME[name])
            made[name, precision] = alphazero.HipLeafNet(net, precision=precision)
        return made[name, precision]
    return get


def _run(h, x):
    v, pi = h.process(x.to(DEV))
    torch.cuda.synchronize()
    return v.cpu(), pi.cpu()


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- 1. the reference's own outputs ----------------------------------------------------------------------------------------------
def test_fixture_against_the_reference_outputs(hip):
    _, x, v_ref, pi_ref = dr.fixture("sg_dense")
    v, pi = _run(hip("sg_dense", "bf16"), x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"sg_dense bf16: |dv| {ev:.3g} |dpi| {epi:.3g}")
    assert v.shape == (8, 3) and pi.shape == (8, 1709)
    assert ev <= lr.TOL and epi <= lr.TOL
    v32, pi32 = _run(hip("sg_dense", "fp32"), x)
    assert _err(v32, v_ref) <= lr.TOL_F32 and _err(pi32, pi_ref) <= lr.TOL_F32


# ---- 2. peaked net: a constant answer must fail -------------------------------------------------------------------------------------
def test_peaked_net_against_fp64_spatial_and_global_halves(hip, peaked):
    net, x, v_ref, pi_ref = peaked
    rows = lr.decided_rows(pi_ref)
    assert float(pi_ref.max() - pi_ref.min()) > 0.3 and float(pi_ref.max(1).values.min()) > 0.3 and bool(rows.all()), "a constant answer must fail"
    assert torch.equal(net.v_fc2.weight, dr.fixture("sg_dense")[0].v_fc2.weight * 4.0), "the shared fixture net is not the scaled one"
    v, pi = _run(hip("sg_dense_peaked", "bf16"), x)
    ev, esp, egl = _err(v, v_ref), _err(pi[:, :SPATIAL], pi_ref[:, :SPATIAL]), _err(pi[:, SPATIAL:], pi_ref[:, SPATIAL:])
    print(f"sg_dense peaked bf16: |dv| {ev:.3g} |dpi spatial| {esp:.3g} |dpi global| {egl:.3g}; max pi {float(pi_ref.max()):.3g}")
    assert ev <= lr.TOL and esp <= lr.TOL and egl <= lr.TOL
    assert torch.equal(pi.argmax(1), pi_ref.argmax(1))


# ---- 3. both ends of every bound -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in sr.ACCEPTED])
def test_case_table_at_both_ends_of_the_bounds(az, name):     # noqa: F811
    case = sr.BY_NAME[name]
    net, x = sr.peaked(sr.make_net(case), 8.0), sr.case_inputs(case, 6, bf16_exact=True)
    v_ref, pi_ref, _ = lr.reference(net, x)
    v, pi = _run(az.HipLeafNet(net, precision="bf16"), x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"{name} bf16: |dv| {ev:.3g} |dpi| {epi:.3g}; max pi per row {[round(float(m), 3) for m in pi_ref.max(1).values]}")
    assert v.shape == v_ref.shape and pi.shape == pi_ref.shape
    assert ev <= lr.TOL and epi <= lr.TOL
    v32, pi32 = _run(az.HipLeafNet(net, precision="fp32"), x)
    assert _err(v32, v_ref) <= lr.TOL_F32 and _err(pi32, pi_ref) <= lr.TOL_F32


# ---- 4. batch sizes, batch invariance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("board", [7, 11, 13])
def test_batch_sizes_and_batch_invariance(hip, peaked, board):
    if board == 13:
        name, (_, x, v_ref, pi_ref) = "sg_dense_peaked", peaked
    else:
        name = f"dsp_b{board}"
        case = sr.BY_NAME[name]
        x = sr.case_inputs(case, 6)
        v_ref, pi_ref, _ = lr.reference(sr.make_net(case), x)
    h = hip(name, "bf16")
    tbw = sr.DSP_TBW[board]
    v_all, pi_all = _run(h, x)
    assert _err(v_all, v_ref) <= lr.TOL and _err(pi_all, pi_ref) <= lr.TOL
    for batch in sorted({1, tbw - 1, tbw, tbw + 1, len(x)} - {0}):
        v, pi = _run(h, x[:batch])
        assert v.shape == (batch, v_ref.shape[1]) and pi.shape == (batch, pi_ref.shape[1])
        assert torch.equal(v, v_all[:batch]) and torch.equal(pi, pi_all[:batch])
    for r in (0, 3, len(x) - 1):     # a row alone has the bits it has inside the batch
        v1, pi1 = _run(h, x[r:r + 1])
        assert torch.equal(v1[0], v_all[r]) and torch.equal(pi1[0], pi_all[r])


# ---- 5. row lists -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_row_lists_touch_only_the_listed_slots(hip, peaked, precision):
    _, x, _, _ = peaked
    h = hip("sg_dense_peaked", precision)
    xs = torch.cat([x, x.flip(0)])[:16].to(DEV).contiguous()
    v_all, pi_all = h.process(xs)
    listed = [11, 2, 7, 15, 0]
    rows = torch.tensor(listed + [3] * 7, dtype=torch.int32, device=DEV)      # 12 entries, the count says 5
    for count in (len(listed), 0):
        v = torch.full((16, 3), -7.0, device=DEV)
        pi = torch.full((16, 1709), -9.0, device=DEV)
        h.forward_rows(xs, v, pi, rows, torch.tensor([count], dtype=torch.int32, device=DEV), max_rows=12)
        torch.cuda.synchronize()
        on = torch.zeros(16, dtype=torch.bool)
        on[listed[:count]] = True
        assert torch.equal(v.cpu()[on], v_all.cpu()[on]) and torch.equal(pi.cpu()[on], pi_all.cpu()[on])
        assert bool((v.cpu()[~on] == -7.0).all()) and bool((pi.cpu()[~on] == -9.0).all())


# ---- 6. extreme logits, degenerate boards ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_extreme_logits_stay_finite_and_keep_the_argmax(az, precision):     # noqa: F811
    net, x, _, _ = dr.fixture("sg_dense")
    big = sr.peaked(net, 400.0)
    v_ref, pi_ref, logits = lr.reference(big, x)
    assert float(logits.abs().max()) > 88.7
    v, pi = _run(az.HipLeafNet(big, precision=precision), x)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(pi).all())
    assert float((v.sum(1) - 1).abs().max()) <= 1e-5 and float((pi.sum(1) - 1).abs().max()) <= 1e-5
    rows = lr.decided_rows(pi_ref)
    assert rows.any() and torch.equal(pi.argmax(1)[rows], pi_ref.argmax(1)[rows])


def test_all_zero_all_one_and_one_cell_boards(hip, peaked):
    net = peaked[0]
    x = torch.zeros((3, 36, 13, 13))
    x[1] = 1.0
    x[2, 5, 12, 12] = 1.0
    v_ref, pi_ref, _ = lr.reference(net, x)
    v, pi = _run(hip("sg_dense_peaked", "bf16"), x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"degenerate boards bf16: |dv| {ev:.3g} |dpi| {epi:.3g}")
    assert ev <= lr.TOL and epi <= lr.TOL


# ---- 7. integration -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_search_with_a_dense_spatial_net_equals_the_step_api(az, hip, precision):     # noqa: F811
    h = hip("sg_dense_peaked", precision)
    n, visits = 4, 8
    rng = np.random.default_rng(11)
    states, gs = [], az.StarGambitUnifiedGS(0)
    for _ in range(n):
        states.append(gs.copy())
        for _ in range(2):                      # the next position is two plies further down a random playout
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            assert gs.scores() is None
    mb = az.MCTSBatch(az.StarGambitUnifiedGS, n, 1.25, max_simulations=visits, seeds=[700 + i for i in range(n)])
    mb.reset(states)
    mb.search(visits, net=h)
    counts, rv = mb.counts(), mb.root_values()
    assert counts.sum() > 0
    mb.reset(states)
    for _ in range(visits):
        canon, idx = mb.find_leaves()
        if canon.shape[0]:
            v, pi = h.process(canon)
        else:
            v, pi = np.zeros((0, 3), np.float32), np.zeros((0, 1709), np.float32)
        mb.process_results(v, pi)
    assert np.array_equal(counts, mb.counts()) and np.array_equal(rv, mb.root_values())
    params = az.PlayParams()
    params.games_to_play = params.concurrent_games = params.max_batch_size = 4
    params.mcts_visits = [8, 8]; params.model_groups = [0, 0]
    # the pipeline asks azmi_net_c4_view_get, which answers 0 for this net whatever the engine's game
    for game in (az.StarGambitUnifiedGS(0), az.Connect4GS()):
        assert not az.pipeline_supported(az.PlayManager(game, params, seed=5), h)
