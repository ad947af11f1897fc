"""-m gpu: HipLeafNet.refresh / azmi_net_refresh - the weight image of a live leaf net rewritten on the device from a trained
LeafNet's CUDA parameters (csrc/leafnet_refresh_kernels.h), in place and on a stream.

The yardstick is the host fold: after refresh(net2) the image read back (HipLeafNet.blob) is byte for byte fold(net2, precision)[1],
so every answer is bit for bit a freshly built HipLeafNet(net2)'s and every holder of the old handle - MCTSBatch, the lock-step
engine, the pipeline's view - carries on with the new weights.  Shapes: the smallest nets of the two families that can still go
wrong - the ResNet tile with 2 blocks and with 1 block at both ends of the value FC bound (both precisions); the dense tile at the
reference default (4 x 12, k = 5: CF = 52), at the growth bound with one block (16, k = 3: CF = 20) and with an odd growth (3 x 5,
k = 3: CF = 19, 4G = 20: every padding of the image is in play)."""
import copy
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import leafnet_ref as lr

pytestmark = pytest.mark.gpu


def _specs():
    from alphazero import torch_net
    c4, dn = torch_net.connect4_spec, torch_net.connect4_dense_spec
    return {
        "resnet_d2": c4(depth=2),
        "resnet_d1_h16": dataclasses.replace(c4(depth=1), v_fc_hidden=16),
        "resnet_d1_h256": dataclasses.replace(c4(depth=1), v_fc_hidden=256),
        "dense_default": dn(),
        "dense_g16_d1_k3": dn(depth=1, channels=16, kernel_size=3),
        "dense_g5_d3_k3": dn(depth=3, channels=5, kernel_size=3),
    }


CASES = [(n, p) for n in ("resnet_d2", "resnet_d1_h16", "resnet_d1_h256") for p in ("bf16", "bf16x3")] + \
        [(n, "bf16") for n in ("dense_default", "dense_g16_d1_k3", "dense_g5_d3_k3")]


@functools.lru_cache(maxsize=None)
def _nets(name):
    """(spec, net1, net2, net2 on the GPU): built once, never changed"""
    from alphazero import torch_net
    spec = _specs()[name]
    net1, net2 = torch_net.random_init(spec, seed=1), torch_net.random_init(spec, seed=2)
    return spec, net1, net2, copy.deepcopy(net2).cuda()


@functools.lru_cache(maxsize=None)
def _folded(name, precision):
    from alphazero import hip_net
    return hip_net.fold(_nets(name)[2], precision)[1]


@functools.lru_cache(maxsize=None)
def _fresh(name, precision, which):
    import alphazero as az
    return az.HipLeafNet(_nets(name)[which], precision=precision)


def _refreshed(name, precision):
    import alphazero as az
    _, net1, _, net2_gpu = _nets(name)
    hip = az.HipLeafNet(net1, precision=precision)
    assert hip.refresh(net2_gpu) is hip
    return hip


def _answers(hip, x, stream=None):
    spec = hip.spec
    v = torch.empty((x.shape[0], spec.num_players + 1), device="cuda")
    pi = torch.empty((x.shape[0], spec.num_moves), device="cuda")
    hip.forward(x, v, pi, stream=stream)
    return v, pi


def _first_difference(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    if len(a) != len(b):
        return f"{len(a)} bytes against {len(b)}"
    bad = np.flatnonzero(a != b)
    return f"{len(bad)} of {len(a)} bytes differ, the first at {bad[0]}, the last at {bad[-1]}"


# ---- 1. byte identity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_refreshed_image_is_the_folded_blob_byte_for_byte(name, precision):
    hip = _refreshed(name, precision)
    want = _folded(name, precision)
    got = hip.blob()
    assert hip._blob is None
    assert got == want, _first_difference(got, want)
    assert got != _fresh(name, precision, 1).blob()          # (and net1's image was another one)


@pytest.mark.parametrize("name,precision", [("resnet_d2", "bf16x3"), ("dense_g5_d3_k3", "bf16")])
def test_running_var_from_denormal_to_huge_folds_as_on_the_host(name, precision):
    """running_var with a float32 denormal, a zero (a = w / sqrt(eps)) and a huge entry in every BatchNorm: the float64 divide and
    square root of the kernel give the host's bits"""
    import alphazero as az
    from alphazero import hip_net
    _, net1, net2, _ = _nets(name)
    net = copy.deepcopy(net2)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var[0], m.running_var[1], m.running_var[2], m.running_var[3] = 1e-40, 3e30, 0.0, 7e-12
    want = hip_net.fold(net, precision)[1]
    hip = az.HipLeafNet(net1, precision=precision)
    got = hip.refresh(net.cuda()).blob()
    assert got == want, _first_difference(got, want)


# ---- 2. same answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_answers_after_a_refresh_are_a_fresh_nets_bit_for_bit(name, precision):
    spec = _nets(name)[0]
    hip, fresh = _refreshed(name, precision), _fresh(name, precision, 2)
    x = lr.sparse_planes(spec, 64, seed=7).cuda()
    v, pi = _answers(hip, x)
    fv, fpi = _answers(fresh, x)
    torch.cuda.synchronize()
    assert torch.equal(v, fv) and torch.equal(pi, fpi)
    ov, opi = _answers(_fresh(name, precision, 1), x)
    assert not torch.equal(pi, opi)                          # (net1 answers otherwise)
    rows = torch.tensor([3, 60, 17, 0, 41], dtype=torch.int32, device="cuda")
    cnt = torch.tensor([5], dtype=torch.int32, device="cuda")
    outs = []
    for h in (hip, fresh):
        rv, rpi = torch.full_like(v, -7.25), torch.full_like(pi, -7.25)
        h.forward_rows(x, rv, rpi, rows, cnt)
        outs.append((rv, rpi))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][1][rows.long()], pi[rows.long()]) and int((outs[0][1] == -7.25).all(1).sum()) == 64 - 5


# ---- 3. the old handle keeps working --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resnet_d2", "dense_default"])
def test_mcts_batch_made_before_the_refresh_searches_with_the_new_weights(name):
    import alphazero as az
    _, net1, _, net2_gpu = _nets(name)
    n, visits = 16, 24
    seeds = [700 + i for i in range(n)]

    def batch():
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds)
        mb.reset([az.Connect4GS() for _ in range(n)])
        return mb
    hip = az.HipLeafNet(net1, precision="bf16")
    mb = batch()
    hip.refresh(net2_gpu)
    mb.search(visits, net=hip)
    ref = batch()
    ref.search(visits, net=_fresh(name, "bf16", 2))
    assert np.array_equal(mb.counts(), ref.counts()) and mb.counts().sum() > 0
    old = batch()
    old.search(visits, net=_fresh(name, "bf16", 1))
    assert not np.array_equal(old.counts(), ref.counts())


def test_engines_made_before_the_refresh_play_the_new_nets_games():
    """a lock-step PlayManager created before the refresh and driven after it, and one run_pipeline run after a refresh (the pipeline
    holds the tile's device pointers through azmi_net_c4_view: the image is rewritten in place, so they stay right): the games of the
    lock-step engine driven by a fresh HipLeafNet(net2)"""
    import alphazero as az
    from test_gpu_pipeline import _lockstep_games, _pipeline_games, _selfplay_params, _sorted_log
    _, net1, _, net2_gpu = _nets("resnet_d2")
    fresh = _fresh("resnet_d2", "bf16", 2)
    hip = az.HipLeafNet(net1, precision="bf16")
    S, seed = 16, 4321
    pp = _selfplay_params(az, S, 16, cache=1 << 10)
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    hip.refresh(net2_gpu)
    st = torch.cuda.Stream()
    while pm.remaining_games() > 0:
        az.run_rounds([pm], hip, 64, [st.cuda_stream])
        if pm.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    want, (rb, cb) = _lockstep_games(az, pp, seed, fresh)
    assert pm.games_completed() == want.games_completed() == S
    ra, ca = _sorted_log(*pm.move_log())
    rb, cb = _sorted_log(rb, cb)
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)
    S2, seed2 = 32, 8765
    pp2 = _selfplay_params(az, S2, 24, cache=1 << 12)
    pa, (rp, cp), stats = _pipeline_games(az, pp2, seed2, hip, sims_per_epoch=S2 * 16)
    pl, (rl, cl) = _lockstep_games(az, pp2, seed2, fresh)
    assert pa.games_completed() == pl.games_completed() == S2 and stats["tiles"] > 0
    rp, cp = _sorted_log(rp, cp)
    rl, cl = _sorted_log(rl, cl)
    assert np.array_equal(rp, rl) and np.array_equal(cp, cl)


# ---- 4. stream order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("resnet_d2", "bf16"), ("resnet_d2", "bf16x3"), ("dense_default", "bf16")])
def test_forwards_around_a_refresh_on_one_stream_see_whole_images(name, precision):
    import alphazero as az
    spec, net1, _, net2_gpu = _nets(name)
    x = lr.sparse_planes(spec, 64, seed=9).cuda()
    want1, want2 = _answers(_fresh(name, precision, 1), x), _answers(_fresh(name, precision, 2), x)
    hip = az.HipLeafNet(net1, precision=precision)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        got1 = _answers(hip, x, stream=st.cuda_stream)
        hip.refresh(net2_gpu, stream=st.cuda_stream)
        got2 = _answers(hip, x, stream=st.cuda_stream)
        hip.refresh(net2_gpu, stream=st.cuda_stream)             # (a second refresh waits for the first one's table and staging image)
        got3 = _answers(hip, x, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(got1[0], want1[0]) and torch.equal(got1[1], want1[1]), "the forward before the refresh did not see net1 whole"
    assert torch.equal(got2[0], want2[0]) and torch.equal(got2[1], want2[1]), "the forward after the refresh did not see net2 whole"
    assert torch.equal(got3[0], want2[0]) and torch.equal(got3[1], want2[1])
    assert not torch.equal(want1[1], want2[1])


# ---- 5. refusals leave the weights untouched ------------------------------------------------------------------------------------
def test_refusals_name_the_field_or_tensor_and_leave_the_weights_untouched():
    import alphazero as az
    from alphazero import torch_net
    spec, net1, _, net2_gpu = _nets("resnet_d2")
    hip = az.HipLeafNet(net1, precision="bf16")
    before = hip.blob()
    assert before == hip._blob

    def variant(change):
        net = copy.deepcopy(net2_gpu)
        change(net)
        return net

    def as_double(net):
        net.conv_layers[1].conv1.weight.data = net.conv_layers[1].conv1.weight.data.double()

    def transposed(net):
        net.conv_layers[0].conv2.weight.data = net.conv_layers[0].conv2.weight.data.transpose(2, 3)

    def six_moves(net):          # the spec still says 7 moves: the library's own check of the element counts catches it
        net.pi_fc1 = torch.nn.Linear(32 * 42, 6).cuda()
    refusals = [
        (torch_net.random_init(dataclasses.replace(spec, depth=3), seed=2).cuda(), ValueError, "depth"),
        (torch_net.random_init(dataclasses.replace(spec, v_fc_hidden=128), seed=2).cuda(), ValueError, "v_fc_hidden"),
        (variant(as_double), RuntimeError, r"conv_layers\.1\.conv1\.weight.*float64"),
        (variant(transposed), RuntimeError, r"conv_layers\.0\.conv2\.weight.*contiguous"),
        (_nets("resnet_d2")[2], RuntimeError, r"conv1\.weight.*cpu"),
        (variant(six_moves), RuntimeError, r"pi_fc1\.weight has 8064 elements"),
    ]
    for net, error, match in refusals:
        with pytest.raises(error, match=match):
            hip.refresh(net)
        assert hip.blob() == before, f"a refused refresh ({match}) changed the weights"
        assert hip._blob is not None
    # and the net still refreshes
    assert hip.refresh(net2_gpu).blob() == _folded("resnet_d2", "bf16")


def test_families_without_a_refresh_say_so_before_any_launch():
    import alphazero as az
    from alphazero import torch_net
    sp = az.HipLeafNet(torch_net.random_init(torch_net.brandubh_spec(), seed=1))
    before = sp.blob()
    with pytest.raises(RuntimeError, match="spatial-head tile.*new HipLeafNet"):
        sp.refresh(torch_net.random_init(torch_net.brandubh_spec(), seed=2).cuda())
    assert sp.blob() == before
    f32 = az.HipLeafNet(_nets("resnet_d1_h16")[1], precision="fp32")
    with pytest.raises(RuntimeError, match="fp32 tier.*new HipLeafNet"):
        f32.refresh(_nets("resnet_d1_h16")[3])
    layer_spec = dataclasses.replace(_specs()["dense_g5_d3_k3"], trunk_norm="layer")
    layer = az.HipLeafNet(torch_net.random_init(layer_spec, seed=1))
    with pytest.raises(RuntimeError, match="layer-norm instance.*new HipLeafNet"):
        layer.refresh(torch_net.random_init(layer_spec, seed=2).cuda())
    # the library's own answer, for a caller of the C entry
    from alphazero.hip_net import NetParamC, lib
    for hip in (sp, f32, layer):
        assert lib.azmi_net_refresh(hip._h, (NetParamC * 1)(), 1, None) == -1
        assert "refresh is not built for this family" in lib.azmi_net_last_error().decode()


# ---- 6. azmi_net_blob_read ---------------------------------------------------------------------------------------------------
def test_blob_read_with_a_wrong_size_is_an_error_and_writes_nothing():
    from alphazero.hip_net import blob_bytes, lib
    hip = _fresh("resnet_d1_h16", "bf16", 1)
    n = blob_bytes(hip.desc)
    for size in (n - 1, n + 1, 0):
        buf = C.create_string_buffer(b"\x5a" * (n + 1), n + 1)
        assert lib.azmi_net_blob_read(hip._h, buf, size) == -1          # AZMI_ERR_INVALID
        assert "weight image" in lib.azmi_net_last_error().decode()
        assert buf.raw == b"\x5a" * (n + 1)
    assert hip.blob() == hip._blob
    f32 = _fresh("resnet_d1_h16", "fp32", 1)
    with pytest.raises(RuntimeError, match="fp32 tier"):
        f32.blob()


def test_refresh_net_refreshes_and_clears_the_caches_it_is_given():
    import alphazero as az
    from alphazero import selfplay
    _, net1, _, net2_gpu = _nets("resnet_d1_h16")

    class Cache:
        cleared = 0

        def clear(self):
            self.cleared += 1
    hip = az.HipLeafNet(net1)
    caches = [Cache(), Cache()]
    assert selfplay.refresh_net(hip, net2_gpu, caches) is hip
    assert [c.cleared for c in caches] == [1, 1] and hip.blob() == _folded("resnet_d1_h16", "bf16")
    other = az.HipLeafNet(net1)
    with pytest.raises(TypeError, match="no clear"):
        selfplay.refresh_net(other, net2_gpu, [az.ShardedS3FIFOCache.for_engine(1024, 7, 3)])
    assert other.blob() == other._blob
