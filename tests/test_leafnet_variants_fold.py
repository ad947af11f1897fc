"""No device needed: the host half of the trunk variants - trunk_norm="layer", trunk_act="crelu", pi_fc_layers > 0 - in
alphazero/torch_net.py, hip_net.fold_fp32 and the validation of azmi_net_blob_bytes2 / azmi_net_create2, which runs before
any device call.

The fixtures under tests/golden/ hold what the reference NNArch itself computed (tests/golden/make_nn_variants_fixture.py).
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import leafnet_variants_ref as vr


@pytest.mark.parametrize("name", sorted(vr.FIXTURES))
def test_leafnet_loads_the_reference_state_dict_and_reproduces_it(name):
    """torch fp32 on the CPU on both sides: 1e-6 is the margin the other fixture tests give this comparison"""
    net, x, v, pi = vr.fixture(name)          # load_state_dict(strict=True) inside
    assert len(x) == 64
    v2, pi2 = net.process(x)
    assert v2.shape == v.shape and pi2.shape == pi.shape
    assert float((v2 - v).abs().max()) <= 1e-6 and float((pi2 - pi).abs().max()) <= 1e-6
    v64, pi64 = vr.reference(net, x)
    assert float((v64 - v.double()).abs().max()) <= 1e-6 and float((pi64 - pi.double()).abs().max()) <= 1e-6
    assert float(pi.max() - pi.min()) > 0.05, "a constant answer must fail"


@pytest.mark.parametrize("dense,norm,act,fc", list(itertools.product((False, True), ("batch", "layer"), ("relu", "crelu"), (0, 2))))
def test_modules_and_parameter_names_follow_the_reference(dense, norm, act, fc):
    from alphazero import torch_net
    spec = torch_net.NetSpec(in_shape=(3, 5, 5), num_moves=30, num_players=2, num_channels=8, depth=2, head_channels=4, dense_net=dense,
                             trunk_norm=norm, trunk_act=act, pi_fc_layers=fc, pi_fc_hidden=12)
    net = torch_net.LeafNet(spec)
    sd = net.state_dict()
    kind = torch.nn.GroupNorm if norm == "layer" else torch.nn.BatchNorm2d
    a = 2 if act == "crelu" else 1
    blk = net.conv_layers[1]
    assert type(blk.bn1) is kind and type(blk.bn2) is kind
    assert ("conv_layers.1.bn1.running_mean" in sd) == (norm == "batch")
    if dense:
        assert "conv1.weight" not in sd and blk.conv1.weight.shape == (32, a * 11, 1, 1) and blk.conv2.weight.shape == (8, a * 32, 3, 3)
    else:
        assert type(net.bn1) is kind and net.conv1.weight.shape == (8, 3, 3, 3)
        assert blk.conv1.weight.shape == (8, a * 8, 3, 3) and blk.conv2.weight.shape == (8, a * 8, 3, 3)
    assert type(net.v_bn) is torch.nn.BatchNorm2d and type(net.pi_bn) is torch.nn.BatchNorm2d, "the heads keep BatchNorm"
    if fc:
        assert sd["pi_fc1.weight"].shape == (12, 100) and sd["pi_fc_extra.0.weight"].shape == (12, 12) and sd["pi_fc_out.weight"].shape == (30, 12)
        assert "pi_fc_extra.2.weight" not in sd
    else:
        assert sd["pi_fc1.weight"].shape == (30, 100) and "pi_fc_out.weight" not in sd
    rnd = torch_net.random_init(spec, seed=4)
    if norm == "layer":
        g = rnd.conv_layers[0].bn1
        assert not torch.equal(g.weight, torch.ones_like(g.weight)) and bool(g.bias.abs().max() > 0), "no identity affine"
    v, pi = rnd.process(torch.rand(3, 3, 5, 5))
    assert v.shape == (3, 3) and pi.shape == (3, 30) and bool(torch.isfinite(pi).all())


def test_netspec_argument_errors():
    from alphazero import torch_net
    base = dict(in_shape=(3, 5, 5), num_moves=50, num_players=2)
    for kw in (dict(trunk_norm="group"), dict(trunk_norm="Layer"), dict(trunk_act="gelu"), dict(pi_fc_layers=-1),
               dict(pi_fc_layers=1, policy_shape=(2, 5, 5))):
        with pytest.raises(ValueError):
            torch_net.NetSpec(**base, **kw)
    torch_net.NetSpec(**base, pi_fc_layers=1)       # the flat head: the caller leaves policy_shape out
    torch_net.NetSpec(**base, policy_shape=(2, 5, 5), trunk_norm="layer", trunk_act="crelu")


def _parent_fp32_blob(net):
    """the fp32 image of a batch / relu net as csrc/leafnet_f32.hip read it before the variants, both trunks, from the state_dict alone"""
    from alphazero.torch_net import bn_affine
    spec = net.spec
    sd = {k: v.detach().double() for k, v in net.state_dict().items()}
    f32 = lambda t: np.ascontiguousarray(np.asarray(t, dtype=np.float64).astype(np.float32)).tobytes()   # noqa: E731

    def conv_bn(w, bn):
        a, b = bn_affine(bn)
        return f32(sd[w] * a[:, None, None, None]) + f32(b)
    out = b"" if spec.dense_net else conv_bn("conv1.weight", net.bn1)
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
        if spec.num_moves > spec.policy_shape[0] * spec.in_shape[1] * spec.in_shape[2]:
            for k in ("pi_global.0.weight", "pi_global.0.bias", "pi_global.2.weight", "pi_global.2.bias", "pi_global.3.weight", "pi_global.3.bias"):
                out += f32(sd[k])
    else:
        out += f32(sd["pi_fc1.weight"]) + f32(sd["pi_fc1.bias"])
    return out


@pytest.mark.parametrize("spec_fn", ["connect4_spec", "brandubh_spec", "stargambit_spec", "connect4_dense_spec", "stargambit_dense_spec"])
def test_batch_relu_nets_fold_byte_for_byte_as_before(spec_fn):
    from alphazero import hip_net, torch_net
    kw = dict(depth=1) if spec_fn.startswith("stargambit") else {}
    net = torch_net.random_init(getattr(torch_net, spec_fn)(**kw), seed=5)
    desc, blob = hip_net.fold(net, "fp32")
    assert isinstance(desc, hip_net.NetDesc2C) == net.spec.dense_net
    assert blob == _parent_fp32_blob(net) and hip_net.blob_bytes(desc) == len(blob)
    if net.spec.dense_net:
        assert not any(desc.reserved) and (desc.trunk_norm, desc.trunk_act, desc.pi_fc_layers) == (0, 0, 0)


@pytest.mark.parametrize("name", sorted(vr.FIXTURES) + [c.name for c in vr.SHAPES])
def test_fold_gives_the_blob_the_library_expects(name):
    from alphazero import hip_net
    net = vr.fixture(name)[0] if name in vr.FIXTURES else vr.make_net(vr.BY_NAME[name])
    spec = net.spec
    desc, blob = hip_net.fold(net, "fp32")
    assert type(desc) is hip_net.NetDesc2C and desc.precision == 1 and desc.dense_net == int(spec.dense_net)
    assert hip_net.blob_bytes(desc) == len(blob) > 0
    assert (desc.trunk_norm, desc.trunk_act, desc.pi_fc_layers) == (int(spec.trunk_norm == "layer"), int(spec.trunk_act == "crelu"), spec.pi_fc_layers)
    assert list(desc.reserved[:3]) == [desc.trunk_norm, desc.trunk_act, desc.pi_fc_layers] and not any(desc.reserved[3:])
    assert desc.pi_hidden == (spec.pi_fc_hidden if spec.pi_fc_layers or (spec.policy_shape and spec.num_moves > np.prod(spec.policy_shape)) else 0)
    # the image is no longer than the parameters it holds (BatchNorms fold four tensors into two)
    assert len(blob) <= 4 * sum(p.numel() for p in net.parameters())
    # the other activation's image has another size (a net without blocks has no CReLU)
    other = hip_net.NetDesc2C(desc.base, desc.dense_net)
    other.trunk_norm, other.trunk_act, other.pi_fc_layers = desc.trunk_norm, 1 - desc.trunk_act, desc.pi_fc_layers
    assert hip_net.blob_bytes(other) != len(blob) or spec.depth == 0


def test_the_named_words_are_the_first_three_reserved_ones():
    from alphazero import hip_net
    d = hip_net.NetDesc2C(hip_net.NetDescC(), 1)
    d.trunk_norm, d.trunk_act, d.pi_fc_layers = 1, 1, 3
    words = np.frombuffer(bytes(d), np.int32)
    assert C.sizeof(d) == 24 * 4 and hip_net.NetDesc2C.dense_net.offset == 16 * 4
    assert list(words[16:]) == [1, 1, 1, 3, 0, 0, 0, 0]
    d.reserved[6] = 9
    assert np.frombuffer(bytes(d), np.int32)[23] == 9


VARIANT_KW = [dict(trunk_norm="layer"), dict(trunk_act="crelu"), dict(pi_fc_layers=1), dict(trunk_norm="layer", trunk_act="crelu", pi_fc_layers=2)]


# (a spatial head has no FC stack to ask for: Brandubh takes the two trunk words alone)
REFUSALS = [(fn, kw) for fn in ("connect4_spec", "brandubh_spec", "connect4_dense_spec") for kw in VARIANT_KW
            if not (fn == "brandubh_spec" and "pi_fc_layers" in kw)]


def test_the_dense_tile_takes_layer_norm_alone():
    """trunk_norm="layer" with relu and no FC stack folds for the dense tile: 256 bytes more per block than the batch image (g2
    beside b2), the raw 1x1 weights, and exact zeros in every padding a statistic or a product could meet"""
    import dataclasses
    from alphazero import hip_net, torch_net
    spec = dataclasses.replace(torch_net.connect4_dense_spec(), trunk_norm="layer")
    net = torch_net.random_init(spec, seed=5)
    desc, blob = hip_net.fold(net, "bf16")
    assert type(desc) is hip_net.NetDesc2C and (desc.dense_net, desc.precision, desc.trunk_norm, desc.trunk_act, desc.pi_fc_layers) == (1, 0, 1, 0, 0)
    assert hip_net.blob_bytes(desc) == len(blob)
    batch = hip_net.NetDesc2C(desc.base, 1)
    assert len(blob) - hip_net.blob_bytes(batch) == 256 * spec.depth
    cin, G, CFP = 4, 12, 64
    prm = np.frombuffer(blob, np.float32, count=2 * CFP + 128)           # block 0: g1 b1 g2 b2
    g1, b1, g2, b2 = prm[:CFP], prm[CFP:2 * CFP], prm[2 * CFP:2 * CFP + 64], prm[2 * CFP + 64:]
    sd = net.state_dict()
    assert np.array_equal(g1[:cin], sd["conv_layers.0.bn1.weight"].numpy()) and np.all(g1[cin:] == 0) and np.all(b1[cin:] == 0)
    assert np.array_equal(g2[:4 * G], sd["conv_layers.0.bn2.weight"].numpy()) and np.array_equal(b2[:4 * G], sd["conv_layers.0.bn2.bias"].numpy())
    assert np.all(g2[4 * G:] == 0) and np.all(b2[4 * G:] == 0)
    for kw, precision in ((dict(trunk_act="crelu"), "bf16"), (dict(pi_fc_layers=1), "bf16"), ({}, "bf16x3")):
        with pytest.raises(RuntimeError) as e:
            hip_net.fold(torch_net.random_init(dataclasses.replace(spec, **kw), seed=5), precision)
        assert "precision='fp32'" in str(e.value)
    for case in vr.TILE_LAYER:
        d, b = hip_net.fold(vr.make_net(case), "bf16")
        assert d.trunk_norm == 1 and hip_net.blob_bytes(d) == len(b) > 0


# on every tile precision, but for the one variant a tile takes (test_the_dense_tile_takes_layer_norm_alone)
REFUSED_RUNS = [(fn, kw, p) for fn, kw in REFUSALS for p in ("bf16", "bf16x3")
                if not (fn == "connect4_dense_spec" and kw == dict(trunk_norm="layer") and p == "bf16")]


@pytest.mark.parametrize("spec_fn,kw,precision", REFUSED_RUNS,
                         ids=lambda a: a if isinstance(a, str) else "+".join(f"{k}={v}" for k, v in a.items()))
def test_the_matrix_core_tiles_refuse_a_variant_by_name(spec_fn, kw, precision):
    """before any device call: fold() raises, and so does azmi_net_create2 for the same words on precision 0 / 2"""
    import dataclasses
    import alphazero as az
    from alphazero import hip_net, torch_net
    spec = dataclasses.replace(getattr(torch_net, spec_fn)(), **kw)
    with pytest.raises(RuntimeError) as e:
        az.HipLeafNet(torch_net.random_init(spec, seed=1), precision=precision)
    assert "precision='fp32'" in str(e.value), str(e.value)
    d32, blob = hip_net.fold(torch_net.random_init(spec, seed=1), "fp32")
    d32.base.precision = 0 if precision == "bf16" else 2
    h = C.c_void_p()
    assert hip_net.lib.azmi_net_blob_bytes2(C.byref(d32)) == 0
    assert hip_net.lib.azmi_net_create2(C.byref(d32), blob, len(blob), 0, C.byref(h)) == -1 and not h.value      # AZMI_ERR_INVALID
    assert "precision='fp32'" in hip_net.lib.azmi_net_last_error().decode()


def test_words_out_of_range_are_invalid_with_a_message():
    from alphazero import hip_net
    d32, blob = hip_net.fold(vr.make_net(vr.BY_NAME["res_layer_spatial_glob"]), "fp32")
    flat, fblob = hip_net.fold(vr.make_net(vr.BY_NAME["res_crelu_fc2"]), "fp32")
    h = C.c_void_p()

    def refused(desc, data, fragment):
        assert hip_net.lib.azmi_net_blob_bytes2(C.byref(desc)) == 0
        assert hip_net.lib.azmi_net_create2(C.byref(desc), data, len(data), 0, C.byref(h)) == -1 and not h.value
        assert fragment in hip_net.lib.azmi_net_last_error().decode(), hip_net.lib.azmi_net_last_error().decode()

    for word, value in (("trunk_norm", 2), ("trunk_norm", -1), ("trunk_act", 2), ("trunk_act", -1), ("pi_fc_layers", -1)):
        bad = hip_net.NetDesc2C(d32.base, d32.dense_net)
        bad.trunk_norm = d32.trunk_norm
        setattr(bad, word, value)
        refused(bad, blob, word)
    bad = hip_net.NetDesc2C(d32.base, d32.dense_net)
    bad.trunk_norm, bad.pi_fc_layers = 1, 1                    # a spatial head (policy_channels > 0) with an FC stack
    refused(bad, blob, "pi_fc_layers")
    bad = hip_net.NetDesc2C(flat.base, 0)
    bad.trunk_act, bad.pi_fc_layers = 1, 2
    bad.base.pi_hidden = 0                                     # the stack's width is missing
    refused(bad, fblob, "pi_hidden")
    for word in (3, 6):                                        # the fourth and the last reserved word
        bad = hip_net.NetDesc2C(flat.base, 0)
        bad.trunk_act, bad.pi_fc_layers = 1, 2
        bad.reserved[word] = 1
        refused(bad, fblob, "reserved")
    # a blob of the wrong mode's size is refused by size: crelu's image against the relu words
    bad = hip_net.NetDesc2C(flat.base, 0)
    bad.pi_fc_layers = 2
    assert hip_net.lib.azmi_net_create2(C.byref(bad), fblob, len(fblob), 0, C.byref(h)) == -1 and not h.value
    assert "bytes, expected" in hip_net.lib.azmi_net_last_error().decode()
