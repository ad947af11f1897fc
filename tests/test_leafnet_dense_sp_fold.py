"""No device needed: the host half of the dense spatial-head tile - hip_net.fold_dense_spatial, the validation of
azmi_net_blob_bytes2 / azmi_net_create2 (refusal in csrc/leafnet_dense_sp_host.hip), which runs before any device call, and
torch_net.stargambit_variant_dense_spec.
"""
import ctypes as C

import numpy as np
import pytest

import leafnet_dense_sp_ref as sr


def _desc_of(spec, precision=0):
    """the second descriptor of a dense spatial spec, word by word from the spec"""
    from alphazero import hip_net
    cin, h, w = spec.in_shape
    pc = spec.policy_shape[0]
    glob = spec.num_moves - pc * h * w
    return hip_net.NetDesc2C(hip_net.NetDescC(cin, h, w, spec.num_channels, spec.depth, spec.kernel_size, spec.head_channels, spec.v_fc_hidden,
                                              spec.num_moves, spec.num_players, spec.v_head_convs, spec.pi_head_convs, spec.v_fc_layers, pc,
                                              precision, spec.pi_fc_hidden if glob > 0 else 0), 1)


def _frag_index(shape):
    """(row, k) of every element of a fragment array [k-steps][m-tiles][64 lanes][8]"""
    ks, mt, _, _ = shape
    lanes = np.arange(64)
    rows = 16 * np.arange(mt)[None, :, None, None] + (lanes & 15)[None, None, :, None]
    k = 32 * np.arange(ks)[:, None, None, None] + 8 * (lanes >> 4)[None, None, :, None] + np.arange(8)[None, None, None, :]
    return np.broadcast_to(rows, shape), np.broadcast_to(k, shape)


@pytest.mark.parametrize("name", [c.name for c in sr.ACCEPTED])
def test_fold_gives_the_blob_the_library_expects_with_exact_zeros_in_every_padding(name):
    from alphazero import hip_net
    case = sr.BY_NAME[name]
    spec = case.spec()
    net = sr.make_net(case)
    desc, blob = hip_net.fold(net, "bf16")
    assert type(desc) is hip_net.NetDesc2C and bytes(desc) == bytes(_desc_of(spec)) and not any(desc.reserved)
    assert len(blob) == hip_net.lib.azmi_net_blob_bytes2(C.byref(desc)) > 0
    assert blob == hip_net.fold_dense_spatial(net)[1]
    cin, G, D, K = spec.in_shape[0], spec.num_channels, spec.depth, spec.kernel_size
    pc = spec.policy_shape[0]
    glob = spec.num_moves - pc * spec.in_shape[1] * spec.in_shape[2]
    CF = cin + G * D
    CFP, MT1, KS2 = (CF + 31) // 32 * 32, (4 * G + 15) // 16, (4 * G + 31) // 32
    off = 0
    for i in range(D):
        Ci = cin + G * i
        prm = np.frombuffer(blob, np.float32, count=2 * CFP + 64, offset=off)
        a1, b1, c1 = prm[:CFP], prm[CFP:2 * CFP], prm[2 * CFP:]
        assert np.all(a1[Ci:] == 0) and np.all(b1[Ci:] == 0) and a1[:Ci].all(), "bn1's affine stops at the block's own inputs"
        assert np.all(c1[4 * G:] == 0) and c1[:4 * G].any()
        off += (2 * CFP + 64) * 4
        ks1 = (Ci + 31) // 32
        w1 = np.frombuffer(blob, np.int16, count=ks1 * MT1 * 512, offset=off).reshape(ks1, MT1, 64, 8)
        rows, k = _frag_index(w1.shape)
        assert np.all(w1[k >= Ci] == 0) and np.all(w1[rows >= 4 * G] == 0) and 0 < np.count_nonzero(w1) <= 4 * G * Ci
        off += w1.size * 2
        w2 = np.frombuffer(blob, np.int16, count=K * K * KS2 * 512, offset=off).reshape(K * K * KS2, 1, 64, 8)
        rows, k = _frag_index((KS2, 1, 64, 8))
        rows, k = np.tile(rows, (K * K, 1, 1, 1)), np.tile(k, (K * K, 1, 1, 1))
        assert np.all(w2[rows >= G] == 0) and np.all(w2[k >= 4 * G] == 0) and 0 < np.count_nonzero(w2) <= G * 4 * G * K * K
        off += w2.size * 2
    assert np.frombuffer(blob, np.float32, count=64, offset=off).all()
    off += 256
    for part in ("high", "low"):       # the heads' 1x1 has split operands: the bf16 high parts of Wh, then the low parts
        wh = np.frombuffer(blob, np.int16, count=(CFP // 32) * 4 * 512, offset=off).reshape(CFP // 32, 4, 64, 8)
        _, k = _frag_index(wh.shape)
        assert np.all(wh[k >= CF] == 0) and 0 < np.count_nonzero(wh) <= 64 * CF, part
        off += wh.size * 2
    hd, p1, hp = spec.v_fc_hidden, spec.num_players + 1, spec.pi_fc_hidden
    off += 4 * (hd * 32 + hd + p1 * hd + p1)
    pol = np.frombuffer(blob, np.float32, count=32 * 32 + 32, offset=off)
    wpol, bpol = pol[:1024].reshape(32, 32), pol[1024:]
    assert np.all(wpol[pc:] == 0) and np.all(bpol[pc:] == 0) and wpol[:pc].all() and bpol[:pc].all()
    off += 4 * (32 * 32 + 32)
    assert len(blob) - off == (4 * (hp * 32 + hp + glob * hp + 3 * glob) if glob else 0)
    if glob:      # the tail is pi_global and its LayerNorm as torch holds them
        sd = net.state_dict()
        tail = np.concatenate([sd[k].numpy().ravel() for k in ("pi_global.0.weight", "pi_global.0.bias", "pi_global.2.weight",
                                                               "pi_global.2.bias", "pi_global.3.weight", "pi_global.3.bias")])
        assert np.array_equal(np.frombuffer(blob, np.float32, offset=off), tail)


@pytest.mark.parametrize("name", [c.name for c in sr.REFUSED])
def test_shapes_outside_the_tile_raise_with_the_reason(name):
    """by HipLeafNet(...) and, for the same descriptor handed to the library, by azmi_net_create2 (both name precision='fp32')"""
    import alphazero as az
    from alphazero import hip_net
    case = sr.BY_NAME[name]
    with pytest.raises(RuntimeError) as e:
        az.HipLeafNet(sr.make_net(case), precision="bf16")
    assert case.refuse in str(e.value) and "precision='fp32'" in str(e.value), str(e.value)
    d2 = _desc_of(case.spec())
    h = C.c_void_p()
    assert hip_net.lib.azmi_net_blob_bytes2(C.byref(d2)) == 0
    assert hip_net.lib.azmi_net_create2(C.byref(d2), b"\0" * 16, 16, 0, C.byref(h)) == -1 and not h.value       # AZMI_ERR_INVALID
    msg = hip_net.lib.azmi_net_last_error().decode()
    assert case.refuse in msg and "precision='fp32'" in msg, msg


def test_variants_and_bf16x3_stay_refused_by_name_on_this_tile():
    import dataclasses
    import alphazero as az
    from alphazero import hip_net, torch_net
    spec = sr.BY_NAME["dsp_b7"].spec()
    for kw, precision in ((dict(trunk_norm="layer"), "bf16"), (dict(trunk_act="crelu"), "bf16"), ({}, "bf16x3")):
        with pytest.raises(RuntimeError) as e:
            az.HipLeafNet(torch_net.random_init(dataclasses.replace(spec, **kw), seed=1), precision=precision)
        assert "precision='fp32'" in str(e.value), str(e.value)
    flat = dataclasses.replace(spec, policy_shape=None, num_moves=9, pi_fc_layers=1)      # (the FC stack is the flat head's)
    with pytest.raises(RuntimeError) as e:
        az.HipLeafNet(torch_net.random_init(flat, seed=1), precision="bf16")
    assert "precision='fp32'" in str(e.value), str(e.value)
    h = C.c_void_p()
    for word in ("trunk_norm", "trunk_act"):
        d2 = _desc_of(spec)
        setattr(d2, word, 1)
        assert hip_net.lib.azmi_net_blob_bytes2(C.byref(d2)) == 0
        assert hip_net.lib.azmi_net_create2(C.byref(d2), b"\0" * 16, 16, 0, C.byref(h)) == -1 and not h.value
        assert "precision='fp32'" in hip_net.lib.azmi_net_last_error().decode()
    d2 = _desc_of(spec, precision=2)
    assert hip_net.lib.azmi_net_blob_bytes2(C.byref(d2)) == 0
    assert hip_net.lib.azmi_net_create2(C.byref(d2), b"\0" * 16, 16, 0, C.byref(h)) == -1 and "precision='fp32'" in hip_net.lib.azmi_net_last_error().decode()


def _fp32_blob_from_the_state_dict(net):
    """the fp32 image of a dense batch / relu net with a spatial head and global actions, from the state_dict alone"""
    from alphazero.torch_net import bn_affine
    sd = {k: v.detach().double() for k, v in net.state_dict().items()}
    f32 = lambda t: np.ascontiguousarray(np.asarray(t, dtype=np.float64).astype(np.float32)).tobytes()   # noqa: E731

    def conv_bn(w, bn):
        a, b = bn_affine(bn)
        return f32(sd[w] * a[:, None, None, None]) + f32(b)
    out = b""
    for i, blk in enumerate(net.conv_layers):
        a1, b1 = bn_affine(blk.bn1)
        out += f32(a1) + f32(b1) + conv_bn(f"conv_layers.{i}.conv1.weight", blk.bn2) + f32(sd[f"conv_layers.{i}.conv2.weight"])
    out += conv_bn("v_conv.weight", net.v_bn) + f32(sd["v_fc1.weight"]) + f32(sd["v_fc1.bias"]) + f32(sd["v_fc2.weight"]) + f32(sd["v_fc2.bias"])
    out += conv_bn("pi_conv.weight", net.pi_bn) + conv_bn("pi_conv2.weight", net.pi_bn2)
    for k in ("pi_global.0.weight", "pi_global.0.bias", "pi_global.2.weight", "pi_global.2.bias", "pi_global.3.weight", "pi_global.3.bias"):
        out += f32(sd[k])
    return out


def test_the_fp32_image_of_the_stargambit_dense_net_is_what_it_was():
    from alphazero import hip_net, torch_net
    net = torch_net.random_init(torch_net.stargambit_dense_spec(), seed=5)
    desc, blob = hip_net.fold(net, "fp32")
    assert type(desc) is hip_net.NetDesc2C and desc.precision == 1 and desc.dense_net == 1 and not any(desc.reserved)
    assert blob == _fp32_blob_from_the_state_dict(net) and hip_net.blob_bytes(desc) == len(blob)


def test_the_single_variant_specs_have_the_games_shapes():
    from alphazero import games, hip_net, torch_net
    classes = (games.StarGambitSkirmishGS, games.StarGambitShowdownGS, games.StarGambitClashGS, games.StarGambitBattleGS)
    for variant, cls in enumerate(classes):
        spec = torch_net.stargambit_variant_dense_spec(variant)
        assert tuple(spec.in_shape) == tuple(cls.CANONICAL_SHAPE()) == (32, 13 if variant == 3 else 11, 13 if variant == 3 else 11)
        assert spec.num_moves == cls.NUM_MOVES() and tuple(spec.policy_shape) == tuple(cls.POLICY_SHAPE()) and spec.num_players == cls.NUM_PLAYERS()
        assert spec.dense_net and (spec.depth, spec.num_channels, spec.kernel_size, spec.head_channels) == (4, 16, 3, 32)
        assert spec.num_moves - int(np.prod(spec.policy_shape)) == 19
        desc, blob = hip_net.fold(torch_net.random_init(spec, seed=variant), "bf16")
        assert desc.policy_channels == 10 and desc.pi_hidden == 256 and len(blob) == hip_net.blob_bytes(desc) > 0
    with pytest.raises(ValueError):
        torch_net.stargambit_variant_dense_spec(4)
