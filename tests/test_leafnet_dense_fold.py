"""No device needed: the host half of the DenseNet leaf net (alphazero/torch_net.py dense trunk, hip_net.fold_dense, the
extended hip_net.fold_fp32, azmi_net_blob_bytes2 / azmi_net_create2's validation, which runs before any device call).

The fixtures under tests/golden/ hold what the reference NNArch itself computed (tests/golden/make_nn_dense_fixture.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import leafnet_dense_ref as dr
import leafnet_ref as lr


@pytest.mark.parametrize("name", sorted(dr.FIXTURES))
def test_leafnet_loads_the_reference_state_dict_and_reproduces_it(name):
    """torch fp32 on the CPU on both sides: the existing fixtures agree to about 1e-7"""
    net, x, v, pi = dr.fixture(name)          # load_state_dict(strict=True) inside
    v2, pi2 = net.process(x)
    assert v2.shape == v.shape and pi2.shape == pi.shape
    assert float((v2 - v).abs().max()) <= 1e-6 and float((pi2 - pi).abs().max()) <= 1e-6


@pytest.mark.parametrize("name", sorted(dr.FIXTURES))
def test_fp64_reference_is_within_1e6_of_the_fixture(name):
    net, x, v, pi = dr.fixture(name)
    v64, pi64, _ = lr.reference(net, x)
    assert float((v64 - v.double()).abs().max()) <= 1e-6 and float((pi64 - pi.double()).abs().max()) <= 1e-6


def test_the_peaked_fixture_is_no_constant():
    _, _, _, pi = dr.fixture("connect4_dense_peaked")
    assert float(pi.max() - pi.min()) > 0.3


def test_dense_trunk_has_the_reference_parameter_names_and_no_stem():
    from alphazero import torch_net
    net = torch_net.LeafNet(torch_net.connect4_dense_spec())
    names = set(net.state_dict())
    assert "conv1.weight" not in names and "bn1.weight" not in names
    assert net.conv_layers[2].conv1.weight.shape == (48, 4 + 12 * 2, 1, 1) and net.conv_layers[2].conv2.weight.shape == (12, 48, 5, 5)
    assert net.v_conv.weight.shape == (32, 4 + 12 * 4, 1, 1) and net.pi_conv.weight.shape == (32, 52, 1, 1)
    with pytest.raises(ValueError):
        torch_net.connect4_dense_spec(kernel_size=4)


@pytest.mark.parametrize("name,precision", [(c.name, p) for c in dr.ACCEPTED_TILE for p in ("bf16", "fp32")] +
                         [(c.name, "fp32") for c in dr.ACCEPTED_F32])
def test_fold_gives_the_blob_the_library_expects(name, precision):
    from alphazero import hip_net
    case = dr.BY_NAME[name]
    spec = case.spec()
    desc, blob = hip_net.fold(dr.make_net(case), precision)
    second = spec.dense_net
    assert isinstance(desc, hip_net.NetDesc2C) == second
    expect = hip_net.lib.azmi_net_blob_bytes2(C.byref(desc)) if second else hip_net.lib.azmi_net_blob_bytes(C.byref(desc))
    assert len(blob) == expect and expect > 0
    assert (desc.in_channels, desc.height, desc.width) == tuple(spec.in_shape)
    assert (desc.channels, desc.depth, desc.kernel_size, desc.precision) == (spec.num_channels, spec.depth, spec.kernel_size, 0 if precision == "bf16" else 1)
    if second:
        assert desc.dense_net == int(spec.dense_net) and not any(desc.reserved)


@pytest.mark.parametrize("name", [c.name for c in dr.REFUSED_TILE])
def test_shapes_outside_the_tile_raise_with_the_reason(name):
    """by fold() and, for the same descriptor handed to the library, by azmi_net_create2 (both name precision='fp32')"""
    import alphazero as az
    from alphazero import hip_net
    case = dr.BY_NAME[name]
    with pytest.raises(RuntimeError) as e:
        az.HipLeafNet(dr.make_net(case), precision="bf16")
    assert case.refuse in str(e.value) and "precision='fp32'" in str(e.value), str(e.value)
    spec = case.spec()
    pc = spec.policy_shape[0] if spec.policy_shape else 0
    d2 = hip_net.NetDesc2C(hip_net.NetDescC(spec.in_shape[0], spec.in_shape[1], spec.in_shape[2], spec.num_channels, spec.depth, spec.kernel_size,
                                            spec.head_channels, spec.v_fc_hidden, spec.num_moves, spec.num_players, 0, 0, 1, pc, 0, 0), 1)
    h = C.c_void_p()
    assert hip_net.lib.azmi_net_blob_bytes2(C.byref(d2)) == 0
    assert hip_net.lib.azmi_net_create2(C.byref(d2), b"\0" * 16, 16, 0, C.byref(h)) == -1       # AZMI_ERR_INVALID
    msg = hip_net.lib.azmi_net_last_error().decode()
    assert case.refuse in msg and "precision='fp32'" in msg, msg


def test_bf16x3_is_refused_for_a_dense_spec():
    from alphazero import hip_net
    with pytest.raises(RuntimeError) as e:
        hip_net.fold(dr.make_net(dr.BY_NAME["dn_default"]), "bf16x3")
    assert "precision='fp32'" in str(e.value)


def test_the_old_entry_keeps_its_bounds_and_reserved_words_must_be_zero():
    from alphazero import hip_net
    d2, blob = hip_net.fold(dr.make_net(dr.BY_NAME["f32_dn_5x5_k5"]), "fp32")
    h = C.c_void_p()
    # the dense net's own descriptor without the dense flag is a 5x5 ResNet: refused by the old entry and by the new one alike
    for rc in (hip_net.lib.azmi_net_create(C.byref(d2.base), blob, len(blob), 0, C.byref(h)),
               hip_net.lib.azmi_net_create2(C.byref(hip_net.NetDesc2C(d2.base, 0)), blob, len(blob), 0, C.byref(h))):
        assert rc == -1 and not h.value and "3x3 convolutions only" in hip_net.lib.azmi_net_last_error().decode()
    bad = hip_net.NetDesc2C(d2.base, 1)
    bad.reserved[3] = 1
    assert hip_net.lib.azmi_net_blob_bytes2(C.byref(bad)) == 0
    rc = hip_net.lib.azmi_net_create2(C.byref(bad), blob, len(blob), 0, C.byref(h))
    assert rc != 0 and not h.value and "reserved" in hip_net.lib.azmi_net_last_error().decode()


def _old_fp32_blob(net):
    """the ResNet 3x3 fp32 image as csrc/leafnet_f32.hip has always read it, built here from the state_dict alone"""
    from alphazero.torch_net import bn_affine
    spec = net.spec
    sd = {k: v.detach().double() for k, v in net.state_dict().items()}
    f32 = lambda t: np.ascontiguousarray(np.asarray(t, dtype=np.float64).astype(np.float32)).tobytes()   # noqa: E731

    def conv_bn(w, bn):
        a, b = bn_affine(bn)
        return f32(sd[w] * a[:, None, None, None]) + f32(b)
    out = conv_bn("conv1.weight", net.bn1)
    for i, blk in enumerate(net.conv_layers):
        a1, b1 = bn_affine(blk.bn1)
        out += f32(a1) + f32(b1) + conv_bn(f"conv_layers.{i}.conv1.weight", blk.bn2) + f32(sd[f"conv_layers.{i}.conv2.weight"])
    out += conv_bn("v_conv.weight", net.v_bn)
    for i in range(spec.v_head_convs):
        out += conv_bn(f"v_extra_convs.{3 * i}.weight", net.v_extra_convs[3 * i + 1])
    out += f32(sd["v_fc1.weight"]) + f32(sd["v_fc1.bias"])
    for l in range(spec.v_fc_layers - 1):
        out += f32(sd[f"v_fc_extra.{2 * l}.weight"]) + f32(sd[f"v_fc_extra.{2 * l}.bias"])
    out += f32(sd["v_fc2.weight"]) + f32(sd["v_fc2.bias"]) + conv_bn("pi_conv.weight", net.pi_bn)
    for i in range(spec.pi_head_convs):
        out += conv_bn(f"pi_extra_convs.{3 * i}.weight", net.pi_extra_convs[3 * i + 1])
    if spec.policy_shape is not None:
        out += conv_bn("pi_conv2.weight", net.pi_bn2)
    else:
        out += f32(sd["pi_fc1.weight"]) + f32(sd["pi_fc1.bias"])
    return out


@pytest.mark.parametrize("spec_fn", ["connect4_spec", "tawlbwrdd_spec"])
def test_resnet_3x3_nets_fold_as_before(spec_fn):
    """first descriptor, old entry point, the same bytes: fp32 against the image built here, the matrix-core tiers through the
    functions no line of which changed (fold_spatial) or against the old blob size"""
    from alphazero import hip_net, torch_net
    net = torch_net.random_init(getattr(torch_net, spec_fn)(), seed=5)
    desc, blob = hip_net.fold(net, "fp32")
    assert type(desc) is hip_net.NetDescC and desc.kernel_size == 3
    assert blob == _old_fp32_blob(net)
    for precision in ("bf16", "bf16x3"):
        d, b = hip_net.fold(net, precision)
        assert type(d) is hip_net.NetDescC and len(b) == hip_net.lib.azmi_net_blob_bytes(C.byref(d))
        if net.spec.policy_shape is not None:
            assert b == hip_net.fold_spatial(net, precision == "bf16x3")[1]


def test_a_narrow_dense_net_folds_to_exact_zeros_in_the_padding():
    """G = 12 (the default): rows 12..15 of every block's k x k weights, rows 48..63 of the bottleneck's bias, the scales and
    biases behind each block's own input channels, and every k past the real channels are exactly zero"""
    from alphazero import hip_net
    case = dr.BY_NAME["dn_default"]
    spec = case.spec()
    desc, blob = hip_net.fold(dr.make_net(case), "bf16")
    cin, G, D, K = spec.in_shape[0], spec.num_channels, spec.depth, spec.kernel_size
    CF = cin + G * D
    CFP = (CF + 31) // 32 * 32
    lanes = np.arange(64)
    off = 0
    for i in range(D):
        Ci = cin + G * i
        prm = np.frombuffer(blob, np.float32, count=2 * CFP + 64, offset=off)
        a1, b1, c1 = prm[:CFP], prm[CFP:2 * CFP], prm[2 * CFP:]
        assert np.all(a1[Ci:] == 0) and np.all(b1[Ci:] == 0) and a1[:Ci].all(), "bn1's affine stops at the block's own inputs"
        assert np.all(c1[4 * G:] == 0) and c1[:4 * G].any()
        off += (2 * CFP + 64) * 4
        ks1 = (Ci + 31) // 32
        w1 = np.frombuffer(blob, np.int16, count=ks1 * 3 * 512, offset=off).reshape(ks1, 3, 64, 8)
        kidx = 32 * np.arange(ks1)[:, None, None, None] + 8 * (lanes >> 4)[None, None, :, None] + np.arange(8)[None, None, None, :]
        assert np.all(w1[np.broadcast_to(kidx, w1.shape) >= Ci] == 0) and np.count_nonzero(w1) <= 4 * G * Ci
        off += w1.size * 2
        w2 = np.frombuffer(blob, np.int16, count=K * K * 2 * 512, offset=off).reshape(K * K, 2, 64, 8)
        rows = np.broadcast_to((lanes & 15)[None, None, :, None], w2.shape)
        k2 = np.broadcast_to(32 * np.arange(2)[None, :, None, None] + 8 * (lanes >> 4)[None, None, :, None] + np.arange(8)[None, None, None, :], w2.shape)
        assert np.all(w2[rows >= G] == 0) and np.all(w2[k2 >= 4 * G] == 0)
        assert 0 < np.count_nonzero(w2) <= G * 4 * G * K * K
        off += w2.size * 2
    bh = np.frombuffer(blob, np.float32, count=64, offset=off)
    assert bh.all()
    off += 256
    wh = np.frombuffer(blob, np.int16, count=(CFP // 32) * 4 * 512, offset=off).reshape(CFP // 32, 4, 64, 8)
    kh = np.broadcast_to(32 * np.arange(CFP // 32)[:, None, None, None] + 8 * (lanes >> 4)[None, None, :, None] + np.arange(8)[None, None, None, :], wh.shape)
    assert np.all(wh[kh >= CF] == 0) and 0 < np.count_nonzero(wh) <= 64 * CF
    off += wh.size * 2
    hd, p1, m = spec.v_fc_hidden, spec.num_players + 1, spec.num_moves
    assert len(blob) - off == 4 * (hd * 32 + hd + p1 * hd + p1 + m * 32 * 42 + m)
