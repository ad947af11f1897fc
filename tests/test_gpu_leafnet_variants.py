"""The trunk variants on the device - trunk_norm="layer" (GroupNorm(1, C): per-sample statistics), trunk_act="crelu",
pi_fc_layers > 0 - on the fp32 tier (csrc/leafnet_f32.hip), which takes them all, at the project's 1e-5, and the layer-norm
instance of the dense Connect4 tile (csrc/leafnet_dense.h, k_leafnet_dense<true>) at the project's bf16 figure 1e-3: against the
reference NNArch's own outputs (tests/golden/nn_*layer*.npz) and the fp64 forward of tests/leafnet_variants_ref.py.

Measured on an MI355X (DESIGN.md 4.6b has the table): see the figures each test prints.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import leafnet_ref as lr
import leafnet_variants_ref as vr
from test_gpu_search_batch import _c4_states, az  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    """HipLeafNet of (fixture or case name, precision), built once"""
    import alphazero
    made = {}

    def get(name, precision="fp32"):
        if (name, precision) not in made:
            net = vr.fixture(name)[0] if name in vr.FIXTURES else vr.make_net(vr.BY_NAME[name])
            made[name, precision] = alphazero.HipLeafNet(net, precision=precision)
        return made[name, precision]
    return get


def _run(h, x):
    v, pi = h.process(x.to(DEV))
    torch.cuda.synchronize()
    return v.cpu(), pi.cpu()


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("name", sorted(vr.FIXTURES))
def test_fp32_tier_reproduces_the_reference_outputs(hip, name):
    _, x, v_ref, pi_ref = vr.fixture(name)
    h = hip(name)
    for batch in (1, len(x)):
        v, pi = _run(h, x[:batch])
        ev, epi = _err(v, v_ref[:batch]), _err(pi, pi_ref[:batch])
        print(f"{name} fp32 batch {batch}: |dv| {ev:.3g} |dpi| {epi:.3g}")
        assert ev <= lr.TOL_F32 and epi <= lr.TOL_F32


@pytest.mark.parametrize("name", [c.name for c in vr.SHAPES])
def test_fp32_tier_shape_table(hip, name):
    case = vr.BY_NAME[name]
    net, x = vr.make_net(case), vr.case_inputs(case, 5)
    v_ref, pi_ref = vr.reference(net, x)
    v, pi = _run(hip(name), x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"{name} fp32: |dv| {ev:.3g} |dpi| {epi:.3g}")
    assert v.shape == v_ref.shape and pi.shape == pi_ref.shape
    assert ev <= lr.TOL_F32 and epi <= lr.TOL_F32


def test_dense_tile_layer_instance_is_within_the_bf16_bound_of_the_reference_outputs(hip):
    """1e-3 is the bound every bf16 tile of the project is held to (tests/leafnet_ref.py TOL)"""
    net, x, v_ref, pi_ref = vr.fixture("c4_dense_layer")
    v, pi = _run(hip("c4_dense_layer", "bf16"), x)
    v64, pi64 = vr.reference(net, x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"c4_dense_layer bf16 tile: |dv| {ev:.3g} |dpi| {epi:.3g} (against fp64: {_err(v, v64):.3g} {_err(pi, pi64):.3g})")
    assert float(pi_ref.max() - pi_ref.min()) > 0.05, "a constant answer must fail"
    assert ev <= lr.TOL and epi <= lr.TOL and _err(v, v64) <= lr.TOL and _err(pi, pi64) <= lr.TOL


@pytest.mark.parametrize("name", [c.name for c in vr.TILE_LAYER])
def test_dense_tile_layer_instance_at_both_ends_of_its_bounds(hip, name):
    case = vr.BY_NAME[name]
    net, x = vr.make_net(case), vr.case_inputs(case, 6, bf16_exact=True)
    v_ref, pi_ref = vr.reference(net, x)
    v, pi = _run(hip(name, "bf16"), x)
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"{name} bf16 tile: |dv| {ev:.3g} |dpi| {epi:.3g}")
    assert ev <= lr.TOL and epi <= lr.TOL
    v32, pi32 = _run(hip(name, "fp32"), x)
    assert _err(v32, v_ref) <= lr.TOL_F32 and _err(pi32, pi_ref) <= lr.TOL_F32


@pytest.mark.parametrize("name,precision", [("c4_dense_layer", "fp32"), ("c4_dense_layer", "bf16"), ("c4_res_layer_crelu_fc2", "fp32")])
def test_degenerate_boards_stay_finite_and_within_the_bound(hip, name, precision):
    """an all-zero and an all-one board: the first norm of a dense trunk (over the planes) has zero variance, inv = 1 / sqrt(eps);
    one set cell: a variance of the order of 1 / (C * H * W)"""
    net, x, _, _ = vr.fixture(name)
    boards = torch.zeros((3,) + tuple(x.shape[1:]))
    boards[1] = 1.0
    boards[2, 1, 3, 4] = 1.0
    v_ref, pi_ref = vr.reference(net, boards)
    v, pi = _run(hip(name, precision), boards)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(pi).all())
    ev, epi = _err(v, v_ref), _err(pi, pi_ref)
    print(f"{name} {precision} degenerate boards: |dv| {ev:.3g} |dpi| {epi:.3g}")
    tol = lr.TOL if precision == "bf16" else lr.TOL_F32
    assert ev <= tol and epi <= tol


@pytest.mark.parametrize("name,precision", [("c4_dense_layer_crelu", "fp32"), ("brandubh_res_layer", "fp32"), ("c4_dense_layer", "bf16")])
def test_a_row_has_the_same_bits_alone_and_anywhere_in_a_batch(hip, name, precision):
    """per-sample statistics: batch statistics, or a reduction that strays into a neighbour's lanes, would change a row with its company"""
    _, x, _, _ = vr.fixture(name)
    h = hip(name, precision)
    v_all, pi_all = _run(h, x)
    for r in (0, 3, 37, 63):
        v1, pi1 = _run(h, x[r:r + 1])
        assert torch.equal(v1[0], v_all[r]) and torch.equal(pi1[0], pi_all[r])
    perm = torch.roll(torch.arange(64), 19)
    v_p, pi_p = _run(h, x[perm])
    assert torch.equal(v_p, v_all[perm]) and torch.equal(pi_p, pi_all[perm])
    other = x.clone()
    other[1::2] = 1.0 - other[1::2]                        # every other row changes: the rows between keep their bits
    v_s, pi_s = _run(h, other)
    assert torch.equal(v_s[0::2], v_all[0::2]) and torch.equal(pi_s[0::2], pi_all[0::2])
    assert not torch.equal(pi_s[1::2], pi_all[1::2])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_row_lists_touch_only_the_listed_slots(hip, precision):
    _, x, _, _ = vr.fixture("c4_dense_layer")
    h = hip("c4_dense_layer", precision)
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


def test_refusals_raise_by_name(az):     # noqa: F811
    from alphazero import hip_net, torch_net
    for spec_fn, kw in (("connect4_spec", dict(trunk_norm="layer")), ("connect4_spec", dict(pi_fc_layers=1)),
                        ("brandubh_spec", dict(trunk_act="crelu")), ("connect4_dense_spec", dict(trunk_act="crelu")),
                        ("connect4_dense_spec", dict(trunk_norm="layer", trunk_act="crelu")), ("connect4_dense_spec", dict(trunk_norm="layer", pi_fc_layers=1)),
                        ("connect4_dense_spec", dict(trunk_norm="layer"))):
        spec = dataclasses.replace(getattr(torch_net, spec_fn)(), **kw)
        for precision in ("bf16x3",) if kw == dict(trunk_norm="layer") and spec.dense_net else ("bf16", "bf16x3"):
            with pytest.raises(RuntimeError) as e:
                az.HipLeafNet(torch_net.random_init(spec, seed=1), precision=precision)
            assert "precision='fp32'" in str(e.value)
    for precision in ("fp32", "bf16"):
        _reserved_word_refused(hip_net, precision)


def _reserved_word_refused(hip_net, precision):
    h = C.c_void_p()
    d2, blob = hip_net.fold(vr.fixture("c4_dense_layer")[0], precision)
    bad = hip_net.NetDesc2C(d2.base, 1)
    bad.trunk_norm = 1
    bad.reserved[3] = 1                                                       # the fourth word is still reserved
    assert hip_net.lib.azmi_net_create2(C.byref(bad), blob, len(blob), 0, C.byref(h)) == -1 and not h.value
    assert "reserved" in hip_net.lib.azmi_net_last_error().decode()
    assert hip_net.lib.azmi_net_create2(C.byref(d2), blob, len(blob), 0, C.byref(h)) == 0 and h.value
    hip_net.lib.azmi_net_destroy(h)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_search_with_a_layer_net_equals_the_step_api(az, hip, precision):     # noqa: F811
    h = hip("c4_dense_layer", precision)
    n, visits = 8, 24
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


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_the_pipeline_refuses_a_layer_net_and_self_play_takes_the_lock_step_rounds(az, hip, precision):     # noqa: F811
    from alphazero import selfplay
    params = az.PlayParams()
    params.games_to_play = params.concurrent_games = params.max_batch_size = 8
    params.mcts_visits = [16, 16]; params.model_groups = [0, 0]; params.history_enabled = True
    h = hip("c4_dense_layer", precision)
    pm = az.PlayManager(az.Connect4GS(), params, seed=5)
    assert not az.pipeline_supported(pm, h)
    result, _ = selfplay.self_play(az.Connect4GS, params, h)
    assert result.games == 8 and result.driver_used == "rounds" and result.fallbacks == 0
