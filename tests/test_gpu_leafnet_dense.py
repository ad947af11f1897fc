"""DenseNet leaf nets on the device: the fp32 tier (csrc/leafnet_f32.hip, every dense shape, kernel sizes 1 / 3 / 5 / 7) and
the bf16 matrix-core tile of the dense Connect4 family (csrc/leafnet_dense.h), against the reference NNArch's own outputs
(tests/golden/nn_*dense*.npz) and the fp64 forward of tests/leafnet_ref.py.

Measured on an MI355X, max |error| against the reference's fp32 outputs: bf16 tile, default fixture dv 5.6e-6
dpi 3.2e-5, peaked fixture dv 4.7e-5 dpi 3.9e-4; fp32 tier <= 5e-8.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import leafnet_dense_ref as dr
import leafnet_ref as lr
from test_gpu_search_batch import _c4_states, az  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    """HipLeafNet of (fixture or case name, precision), built once"""
    import alphazero
    made = {}

    def get(name, precision):
        if (name, precision) not in made:
            net = dr.fixture(name)[0] if name in dr.FIXTURES else dr.make_net(dr.BY_NAME[name])
            made[name, precision] = alphazero.HipLeafNet(net, precision=precision)
        return made[name, precision]
    return get


def _run(h, x):
    v, pi = h.process(x.to(DEV))
    torch.cuda.synchronize()
    return v.cpu(), pi.cpu()


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- fp32 tier ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dr.FIXTURES))
def test_fp32_tier_reproduces_the_reference_outputs(hip, name):
    _, x, v_ref, pi_ref = dr.fixture(name)
    h = hip(name, "fp32")
    for batch in (1, len(x)):
        v, pi = _run(h, x[:batch])
        ev, epi = _err(v, v_ref[:batch]), _err(pi, pi_ref[:batch])
        print(f"{name} fp32 batch {batch}: |dv| {ev:.3g} |dpi| {epi:.3g}")
        assert ev <= lr.TOL_F32 and epi <= lr.TOL_F32


def test_fp32_tier_regrows_above_its_4096_row_reservation(hip):
    _, x, v_ref, pi_ref = dr.fixture("connect4_dense")
    reps = 4100 // len(x) + 1
    v, pi = _run(hip("connect4_dense", "fp32"), x.repeat(reps, 1, 1, 1)[:4100])
    assert _err(v, v_ref.repeat(reps, 1)[:4100]) <= lr.TOL_F32 and _err(pi, pi_ref.repeat(reps, 1)[:4100]) <= lr.TOL_F32


@pytest.mark.parametrize("name", [c.name for c in dr.ACCEPTED_F32])
def test_fp32_tier_shape_table(hip, name):
    case = dr.BY_NAME[name]
    net, x = dr.make_net(case), dr.case_inputs(case, 5)
    v_ref, pi_ref, _ = lr.reference(net, x)
    v, pi = _run(hip(name, "fp32"), x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"{name} fp32: |dv| {ev:.3g} |dpi| {epi:.3g}")
    assert ev <= lr.TOL_F32 and epi <= lr.TOL_F32


# ---- bf16 tile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["connect4_dense", "connect4_dense_peaked"])
def test_bf16_tile_is_within_the_bf16_bound_of_the_reference_outputs(hip, name):
    """1e-3 is the bound every bf16 tile of the project is held to (tests/leafnet_ref.py TOL)"""
    _, x, v_ref, pi_ref = dr.fixture(name)
    v, pi = _run(hip(name, "bf16"), x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"{name} bf16: |dv| {ev:.3g} |dpi| {epi:.3g}")
    if name.endswith("peaked"):
        assert float(pi_ref.max() - pi_ref.min()) > 0.3, "a constant answer must fail"
    assert ev <= lr.TOL and epi <= lr.TOL
    if name.endswith("peaked"):
        rows = lr.decided_rows(pi_ref)
        assert rows.any() and torch.equal(pi.argmax(1)[rows], pi_ref.argmax(1)[rows])


@pytest.mark.parametrize("name", [c.name for c in dr.ACCEPTED_TILE])
def test_bf16_tile_at_both_ends_of_its_bounds(hip, name):
    case = dr.BY_NAME[name]
    net, x = dr.make_net(case), dr.case_inputs(case, 6)
    v_ref, pi_ref, _ = lr.reference(net, x)
    v, pi = _run(hip(name, "bf16"), x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"{name} bf16: |dv| {ev:.3g} |dpi| {epi:.3g}")
    assert ev <= lr.TOL and epi <= lr.TOL
    v32, pi32 = _run(hip(name, "fp32"), x)
    assert _err(v32, v_ref) <= lr.TOL_F32 and _err(pi32, pi_ref) <= lr.TOL_F32


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_batch_sizes_and_batch_invariance(hip, precision):
    _, x, v_ref, pi_ref = dr.fixture("connect4_dense_peaked")
    h = hip("connect4_dense_peaked", precision)
    tol = lr.TOL if precision == "bf16" else lr.TOL_F32
    v_all, pi_all = _run(h, x)
    for batch in (1, dr.DENSE_TBW - 1, dr.DENSE_TBW, dr.DENSE_TBW + 1, len(x)):
        v, pi = _run(h, x[:batch])
        assert v.shape == (batch, 3) and pi.shape == (batch, 7)
        assert _err(v, v_ref[:batch]) <= tol and _err(pi, pi_ref[:batch]) <= tol
        assert torch.equal(v, v_all[:batch]) and torch.equal(pi, pi_all[:batch])
    for r in (0, 5, len(x) - 1):     # a row alone has the bits it has inside the batch
        v1, pi1 = _run(h, x[r:r + 1])
        assert torch.equal(v1[0], v_all[r]) and torch.equal(pi1[0], pi_all[r])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_row_lists_touch_only_the_listed_slots(hip, precision):
    _, x, _, _ = dr.fixture("connect4_dense_peaked")
    h = hip("connect4_dense_peaked", precision)
    xs = x[:16].to(DEV).contiguous()
    v_all, pi_all = h.process(xs)
    listed = [11, 2, 7, 15, 0]
    rows = torch.tensor(listed + [3] * 7, dtype=torch.int32, device=DEV)      # 12 entries, the count says 5
    for count in (len(listed), 0):
        v = torch.full((16, 3), -7.0, device=DEV)
        pi = torch.full((16, 7), -9.0, device=DEV)
        h.forward_rows(xs, v, pi, rows, torch.tensor([count], dtype=torch.int32, device=DEV), max_rows=12)
        torch.cuda.synchronize()
        on = torch.zeros(16, dtype=torch.bool)
        on[listed[:count]] = True
        assert torch.equal(v.cpu()[on], v_all.cpu()[on]) and torch.equal(pi.cpu()[on], pi_all.cpu()[on])
        assert bool((v.cpu()[~on] == -7.0).all()) and bool((pi.cpu()[~on] == -9.0).all())


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_extreme_logits_stay_finite_and_keep_the_argmax(az, precision):     # noqa: F811
    """output layers scaled as leafnet_ref.extreme_net does, until the reference's logits are past fp32 exp overflow"""
    from alphazero import torch_net
    spec = torch_net.connect4_dense_spec()
    net = torch_net.random_init(spec, seed=2)
    with torch.no_grad():
        net.pi_fc1.weight.mul_(400.0); net.pi_fc1.bias.mul_(400.0)
        net.v_fc2.weight.mul_(400.0); net.v_fc2.bias.mul_(400.0)
    x = (torch.rand((64,) + tuple(spec.in_shape), generator=torch.Generator().manual_seed(2)) < 0.25).float()
    v_ref, pi_ref, logits = lr.reference(net, x)
    assert float(logits.abs().max()) > 88.7
    v, pi = _run(az.HipLeafNet(net, precision=precision), x)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(pi).all())
    assert float((v.sum(1) - 1).abs().max()) <= 1e-5 and float((pi.sum(1) - 1).abs().max()) <= 1e-5
    rows = lr.decided_rows(pi_ref)
    assert rows.any() and torch.equal(pi.argmax(1)[rows], pi_ref.argmax(1)[rows])


# ---- integration ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_search_with_a_dense_net_equals_the_step_api(az, hip, precision):     # noqa: F811
    h = hip("connect4_dense_peaked", precision)
    n, visits = 8, 16
    states = _c4_states(az, n, seed=5)
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=visits, seeds=[700 + i for i in range(n)])
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
            v, pi = np.zeros((0, 3), np.float32), np.zeros((0, 7), np.float32)
        mb.process_results(v, pi)
    assert np.array_equal(counts, mb.counts()) and np.array_equal(rv, mb.root_values())


def test_the_pipeline_refuses_a_dense_net_and_self_play_takes_the_lock_step_rounds(az, hip):     # noqa: F811
    from alphazero import selfplay
    params = az.PlayParams()
    params.games_to_play = params.concurrent_games = params.max_batch_size = 8
    params.mcts_visits = [16, 16]; params.model_groups = [0, 0]; params.history_enabled = True
    for precision in ("bf16", "fp32"):
        h = hip("connect4_dense_peaked", precision)
        pm = az.PlayManager(az.Connect4GS(), params, seed=5)
        assert not az.pipeline_supported(pm, h)
        with pytest.raises(RuntimeError):
            az.run_pipeline(pm, h, 1, 64)
    result, _ = selfplay.self_play(az.Connect4GS, params, hip("connect4_dense_peaked", "bf16"))
    assert result.games == 8 and result.driver_used == "rounds" and result.fallbacks == 0


def test_the_old_entry_refuses_5x5_and_reserved_words_must_be_zero(az):     # noqa: F811
    from alphazero import hip_net
    d2, blob = hip_net.fold(dr.make_net(dr.BY_NAME["f32_dn_5x5_k5"]), "fp32")
    h = C.c_void_p()
    assert hip_net.lib.azmi_net_create(C.byref(d2.base), blob, len(blob), 0, C.byref(h)) == -1 and not h.value      # kernel_size 5
    bad = hip_net.NetDesc2C(d2.base, 1)
    bad.reserved[6] = 5
    assert hip_net.lib.azmi_net_create2(C.byref(bad), blob, len(blob), 0, C.byref(h)) == -1 and not h.value     # AZMI_ERR_INVALID
    assert hip_net.lib.azmi_net_create2(C.byref(d2), blob, len(blob), 0, C.byref(h)) == 0 and h.value
    hip_net.lib.azmi_net_destroy(h)
