"""The trunk read-out of the fp32 tier (azmi_net_trunk_channels / azmi_net_trunk_features, csrc/leafnet_f32.hip) and effective_rank
on top of it, against the package's LeafNet in float64 with a forward hook on `conv_layers` (tests/feature_rank_ref.py): the
smallest nets that take each trunk path, batches of 1, 3 and 130, at the tolerance the fp32 tier's outputs are held to
(leafnet_ref.TOL_F32).  azmi_net_forward keeps its bits around a read-out.

EFF_MARGIN is ten times the largest relative deviation of effective_rank from the float64 figure measured over EFF_NETS on an
MI355X (DESIGN.md 8.5.3 has both figures); the tests print what they measure before they assert.
"""
import numpy as np
import pytest
import torch

import feature_rank_ref as fr
import leafnet_ref as lr
from test_gpu_search_batch import az  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EFF_MEASURED = 2.07e-8      # the largest |effective_rank / float64 figure - 1| over EFF_NETS: dense_k5; res_6x7: 1.18e-8
EFF_MARGIN = 10 * EFF_MEASURED

C4 = dict(in_shape=(4, 6, 7), num_moves=7, num_players=2, head_channels=8, v_fc_hidden=16)
SP7 = dict(in_shape=(7, 7, 7), num_moves=686, num_players=2, head_channels=8, v_fc_hidden=16, v_head_convs=1, pi_head_convs=1, v_fc_layers=2,
           policy_shape=(14, 7, 7))      # torch_net.brandubh_spec(), shrunk
NETS = {
    "res_6x7": dict(C4, num_channels=8, depth=2),
    "res_7x7_spatial": dict(SP7, num_channels=8, depth=2),
    "dense_k3": dict(C4, num_channels=4, depth=2, kernel_size=3, dense_net=True),
    "dense_k5": dict(C4, num_channels=4, depth=2, kernel_size=5, dense_net=True),
    "res_layer": dict(C4, num_channels=8, depth=2, trunk_norm="layer"),
    "res_crelu": dict(C4, num_channels=8, depth=2, trunk_act="crelu"),
    "dense_layer": dict(C4, num_channels=4, depth=2, kernel_size=3, dense_net=True, trunk_norm="layer"),
    "dense_crelu": dict(C4, num_channels=4, depth=2, kernel_size=5, dense_net=True, trunk_act="crelu"),
    "dense_layer_crelu_spatial": dict(SP7, num_channels=4, depth=2, kernel_size=3, dense_net=True, trunk_norm="layer", trunk_act="crelu"),
    "res_depth0": dict(C4, num_channels=8, depth=0),              # the stem alone: conv_layers is empty and hands its input on
    "res_layer_depth0": dict(C4, num_channels=8, depth=0, trunk_norm="layer"),
    "dense_depth1": dict(C4, num_channels=4, depth=1, kernel_size=3, dense_net=True),
}
EFF_NETS = ("res_6x7", "dense_k5")
BATCHES = (1, 3, 130)


@pytest.fixture(scope="module")
def nets():
    """name -> (LeafNet, HipLeafNet fp32, inputs [130, ...], float64 features [130, CF]), built once and left unchanged"""
    import alphazero
    from alphazero import torch_net
    made = {}

    def get(name):
        if name not in made:
            net = torch_net.random_init(torch_net.NetSpec(**NETS[name]), seed=21)
            x = lr.sparse_planes(net.spec, max(BATCHES), seed=4)
            made[name] = (net, alphazero.HipLeafNet(net, precision="fp32"), x, fr.trunk_features_ref(net, x))
        return made[name]
    return get


def _features(hip, x):
    out = hip.trunk_features(x.to(DEV).contiguous())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("name", sorted(NETS))
def test_trunk_features_match_the_float64_hook(nets, name):
    net, hip, x, want = nets(name)
    spec = net.spec
    cin = spec.in_shape[0]
    cf = cin + spec.num_channels * spec.depth if spec.dense_net else spec.num_channels
    assert hip.trunk_channels == cf == want.shape[1]
    assert float(want.abs().max()) > 0.05 and float(want.std(dim=0).max()) > 0.01, "a constant answer must fail"
    for batch in BATCHES:
        got = _features(hip, x[:batch])
        err = float((got.double() - want[:batch]).abs().max())
        print(f"{name} trunk_features batch {batch}: CF {cf} max |feature| {float(want.abs().max()):.3g} |d| {err:.3g}")
        assert got.shape == (batch, cf) and got.dtype == torch.float32
        assert err <= lr.TOL_F32
        if spec.dense_net:      # a dense trunk's features begin with the input planes: their means, to float32 rounding of the sum
            planes = x[:batch].double().mean(dim=(2, 3))
            assert float((got[:, :cin].double() - planes).abs().max()) <= 1e-6


@pytest.mark.parametrize("name", ["res_6x7", "dense_layer", "dense_layer_crelu_spatial"])
def test_a_row_has_the_same_bits_alone_and_anywhere_in_a_batch(nets, name):
    _, hip, x, _ = nets(name)
    whole = _features(hip, x)
    for r in (0, 2, 64, 129):
        assert torch.equal(_features(hip, x[r:r + 1])[0], whole[r])
    perm = torch.roll(torch.arange(len(x)), 19)
    assert torch.equal(_features(hip, x[perm]), whole[perm])
    assert torch.equal(_features(hip, x[:3]), whole[:3])


def test_out_and_stream_arguments(nets):
    _, hip, x, _ = nets("res_6x7")
    xs = x[:5].to(DEV).contiguous()
    want = hip.trunk_features(xs)
    out = torch.full((5, hip.trunk_channels), -3.0, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    assert hip.trunk_features(xs, out=out, stream=side.cuda_stream) is out
    side.synchronize()
    assert torch.equal(out, want)
    assert tuple(hip.trunk_features(xs[:0]).shape) == (0, hip.trunk_channels)
    for bad, fragment in ((xs.double(), "contiguous float32"), (xs[:, :, :, :6], "contiguous float32"), (xs.cpu(), "CUDA tensor")):
        with pytest.raises(RuntimeError, match="trunk_features: canonical must be a .*" + fragment):
            hip.trunk_features(bad)
    with pytest.raises(RuntimeError, match="trunk_features: out must be a contiguous float32"):
        hip.trunk_features(xs, out=torch.empty((5, hip.trunk_channels + 1), device=DEV))


def test_forward_keeps_its_bits_around_a_read_out(nets):
    net, hip, x, _ = nets("dense_layer")
    xs = x.to(DEV).contiguous()
    v0, pi0 = hip.process(xs)
    hip.trunk_features(xs)
    v1, pi1 = hip.process(xs)
    hip.trunk_features(xs[:7])
    v2, pi2 = hip.process(xs)
    torch.cuda.synchronize()
    assert torch.equal(v0, v1) and torch.equal(pi0, pi1) and torch.equal(v0, v2) and torch.equal(pi0, pi2)
    v_ref, pi_ref, _ = lr.reference(net, x)
    ev, epi = float((v0.cpu().double() - v_ref).abs().max()), float((pi0.cpu().double() - pi_ref).abs().max())
    print(f"dense_layer forward around trunk_features: |dv| {ev:.3g} |dpi| {epi:.3g}")
    assert ev <= lr.TOL_F32 and epi <= lr.TOL_F32


@pytest.mark.parametrize("name", EFF_NETS)
def test_effective_rank_matches_the_float64_figure(az, nets, name):     # noqa: F811
    _, hip, x, feats = nets(name)
    want = fr.feature_rank_ref(feats.numpy())["rank"]
    xs = x.to(DEV).contiguous()
    chunked = az.effective_rank(xs, hip, batch_rows=64)      # 130 rows: 64 + 64 + 2
    whole = az.effective_rank(xs, hip)
    staged = az.effective_rank(x.numpy(), hip, batch_rows=64)
    dev = abs(chunked / want - 1.0)
    print(f"{name} effective_rank over 130 rows: {chunked:.9g} (float64 {want:.9g}) relative deviation {dev:.3g}")
    assert 1.0 < want < hip.trunk_channels
    assert np.float64(chunked).tobytes() == np.float64(whole).tobytes() == np.float64(staged).tobytes()
    assert dev <= EFF_MARGIN
    feats_dev = hip.trunk_features(xs)
    assert np.float64(az.feature_rank(feats_dev)["rank"]).tobytes() == np.float64(whole).tobytes()
    assert np.isnan(az.effective_rank(xs[:0], hip)) and np.isnan(az.effective_rank(None, hip))


def test_another_tier_is_refused_by_name(az):     # noqa: F811
    from alphazero import torch_net
    spec = torch_net.connect4_spec(depth=1)
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=2), precision="bf16")
    x = lr.sparse_planes(spec, 4, seed=1, bf16_exact=True).to(DEV)
    for call in (lambda: hip.trunk_channels, lambda: hip.trunk_features(x), lambda: az.effective_rank(x, hip),
                 lambda: az.effective_rank(x.cpu().numpy(), hip, batch_rows=2)):
        with pytest.raises(RuntimeError, match="precision='fp32'"):
            call()
    v, pi = hip.process(x)      # the tile itself is untouched
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(pi).all())


def test_window_effective_rank_reads_the_rows_it_names(az, nets):     # noqa: F811
    from alphazero import selfplay
    _, hip, x, _ = nets("res_6x7")

    def segment(rows):
        return (rows.to(DEV).contiguous(), torch.zeros((len(rows), 3), device=DEV), torch.zeros((len(rows), 7), device=DEV))
    window = az.SampleWindow(4, 0, 1.0, 11)
    window.append(0, segment(x[:30]))
    window.append(1, segment(x[30:]))      # the newest iteration: 100 rows
    newest = segment(x[30:])
    picked = next(az.window_batches([newest], 64, 5, pass_index=0, batches=1))[0]
    assert picked.shape[0] == 64
    got = selfplay.window_effective_rank(window, hip, rows=64, seed=5)
    assert np.float64(got).tobytes() == np.float64(az.effective_rank(picked, hip)).tobytes()
    assert got != selfplay.window_effective_rank(window, hip, rows=64, seed=6)
    everything = selfplay.window_effective_rank(window, hip)      # 512 rows asked, 100 there: all of them, in place
    assert np.float64(everything).tobytes() == np.float64(az.effective_rank(newest[0], hip)).tobytes()
