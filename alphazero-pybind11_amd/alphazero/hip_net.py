"""Host side of the fused MFMA leaf net (csrc/leafnet.hip and its family units leafnet_*_host.hip): BatchNorm folding, bf16 conversion and
the MFMA-fragment weight layout, plus the ctypes wrapper `HipLeafNet`.

Weight blob layout (little-endian, in this order; `frag` = [k-step][m-tile][lane 0..63][8 bf16] where
element j of lane l is  W[co = 16*mt + (l & 15)][k = 32*ks + 8*(l >> 4) + j]):
  stem    frag[2][4]   W[co][k = tap*C_in + ci] (k >= 9*C_in zero)      + bias[64] f32   (bn1 folded)
  block i a1[64] b1[64] c1[64] f32 | conv1 frag[18][4] (bn2 folded, k = tap*64 + ci) | conv2 frag[18][4]
  heads   frag[2][4]   rows 0-31 = v_conv * v_bn, rows 32-63 = pi_conv * pi_bn + bias[64] f32
  v_fc1 W^T[32][hidden] b[hidden] | v_fc2 W[P+1][hidden] b[P+1]  (f32) | pi_fc1: per pixel p frag hi(W[m][c*HW+p]) frag lo | b[M] f32
"""
import ctypes as C
import dataclasses

import numpy as np
import torch

from . import _capi
from ._capi import lib
from .torch_net import bn_affine


class NetDescC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_channels", "height", "width", "channels", "depth", "kernel_size",
                                         "head_channels", "v_hidden", "num_moves", "num_players", "v_head_convs",
                                         "pi_head_convs", "v_fc_layers", "policy_channels", "precision", "pi_hidden")]


class NetDesc2C(C.Structure):
    """azmi_net_desc2 (include/azmi.h): the first descriptor, then what came later.  Reads of the first one's fields pass through.
    `reserved` keeps the seven words behind dense_net under their old indices: words 0..2 have names now (trunk_norm, trunk_act,
    pi_fc_layers, the properties below), reserved[3..6] are the ones that must still be zero."""
    _fields_ = [("base", NetDescC), ("dense_net", C.c_int32), ("reserved", C.c_int32 * 7)]

    def __getattr__(self, name):      # (only reached for names the class does not have: the properties below come first)
        return getattr(self.base, name)

    @property
    def trunk_norm(self):
        return self.reserved[0]

    @trunk_norm.setter
    def trunk_norm(self, v):
        self.reserved[0] = v

    @property
    def trunk_act(self):
        return self.reserved[1]

    @trunk_act.setter
    def trunk_act(self, v):
        self.reserved[1] = v

    @property
    def pi_fc_layers(self):
        return self.reserved[2]

    @pi_fc_layers.setter
    def pi_fc_layers(self, v):
        self.reserved[2] = v


def is_variant(spec):
    """what only the second descriptor can say: layer norm, crelu, the policy FC stack.  The fp32 tier runs them all; the dense
    Connect4 tile has a layer-norm instance (relu, no FC stack), no other tile - the dense spatial one included - takes any."""
    return spec.trunk_norm != "batch" or spec.trunk_act != "relu" or spec.pi_fc_layers > 0


def blob_bytes(desc):
    """azmi_net_blob_bytes / azmi_net_blob_bytes2 of a descriptor of either kind."""
    fn = lib.azmi_net_blob_bytes2 if isinstance(desc, NetDesc2C) else lib.azmi_net_blob_bytes
    return fn(C.byref(desc))


lib.azmi_net_blob_bytes2.restype = C.c_size_t
lib.azmi_net_blob_bytes2.argtypes = [C.POINTER(NetDesc2C)]
lib.azmi_net_create2.restype = C.c_int
lib.azmi_net_create2.argtypes = [C.POINTER(NetDesc2C), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
lib.azmi_net_blob_bytes.restype = C.c_size_t
lib.azmi_net_blob_bytes.argtypes = [C.POINTER(NetDescC)]
lib.azmi_net_create.restype = C.c_int
lib.azmi_net_create.argtypes = [C.POINTER(NetDescC), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
lib.azmi_net_destroy.restype = None
lib.azmi_net_destroy.argtypes = [C.c_void_p]
lib.azmi_net_forward.restype = C.c_int
lib.azmi_net_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
lib.azmi_net_forward_rows.restype = C.c_int
lib.azmi_net_forward_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
lib.azmi_net_last_error.restype = C.c_char_p


class NetParamC(C.Structure):
    """azmi_net_param (include/azmi.h): one tensor of the table azmi_net_refresh reads."""
    _fields_ = [("data", C.c_void_p), ("count", C.c_uint64), ("kind", C.c_uint32), ("reserved", C.c_uint32), ("eps", C.c_double)]


lib.azmi_net_refresh.restype = C.c_int
lib.azmi_net_refresh.argtypes = [C.c_void_p, C.POINTER(NetParamC), C.c_uint32, C.c_void_p]
lib.azmi_net_blob_read.restype = C.c_int
lib.azmi_net_blob_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]


def _bf16_bits(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(torch.bfloat16).view(torch.int16).numpy()


def _frags(wmat):
    """wmat [16*MT][K] float -> bf16 fragments [K/32][MT][64][8] as bytes."""
    co, K = wmat.shape
    assert co % 16 == 0 and K % 32 == 0
    nmt = co // 16
    lanes = np.arange(64)
    out = np.zeros((K // 32, nmt, 64, 8), np.int16)
    bits = _bf16_bits(wmat)
    for ks in range(K // 32):
        for mt in range(nmt):
            rows = 16 * mt + (lanes & 15)
            cols = 32 * ks + 8 * (lanes >> 4)
            out[ks, mt] = np.stack([bits[rows, cols + j] for j in range(8)], axis=1)
    return out.tobytes()


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)).tobytes()


def _f32_frags(w):
    """w [N][K] (rows = outputs, N % 16 == 0, K % 16 == 0) -> f32 MFMA A-fragments [N/16][K/16][64 lanes][4]:
    element j of lane l = w[16*tile + (l & 15)][16*group + 4*j + (l >> 4)] (v_mfma_f32_16x16x4_f32, k-step j)."""
    w = np.asarray(w, dtype=np.float64)
    N, K = w.shape
    assert N % 16 == 0 and K % 16 == 0
    lanes = np.arange(64)
    out = np.zeros((N // 16, K // 16, 64, 4), np.float32)
    for t in range(N // 16):
        rows = 16 * t + (lanes & 15)
        for g in range(K // 16):
            for j in range(4):
                out[t, g, :, j] = w[rows, 16 * g + 4 * j + (lanes >> 4)]
    return out.tobytes()


def _pad(t, *shape):
    """t zero-padded (at the high end of every axis) to `shape`, float64."""
    t = torch.as_tensor(t, dtype=torch.float64)
    out = torch.zeros(shape, dtype=torch.float64)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


def _conv_frags(w):
    """conv weight [co][ci][3][3] (BatchNorm scale already folded) -> 9 chunks of 8 KB: k = tap*64 + ci, channels zero-padded to 64."""
    return _frags(_pad(w.permute(0, 2, 3, 1), 64, 3, 3, 64).reshape(64, 576).numpy())


def fold_spatial(net, x3=False):
    """Spatial-policy-head nets (Tafl family, StarGambit: one extra conv per head, v_fc_layers >= 1; trunk and head widths up
    to 64 channels - narrower ones (configs/brandubh.yaml: 32) are zero-padded: the padded channels have zero weights, scales
    and biases, so they stay exactly 0 through every affine / ReLU / conv).  Image read by csrc/leafnet_sp.h:
      stream of 8 KB chunks frag[2 k-steps][4 m-tiles]: stem (2: k = tap*8 + ci for <= 8 input planes; else 9: one more 64-channel
        conv) | per block conv1 (9) conv2 (9) | value-head 1x1 (1) |
        policy-head 1x1 (1) | value extra conv (9) | policy extra conv (9) | policy 1x1 (1, rows >= policy channels zero)
      fp32: stem_b[64] | per block a1 b1 c1 | head_b[128] | vx_b[64] | px_b[64] | pol_b[32]
      value FC: fc1 f32-frag[Hd/16][4] b | extra FC (f32-frag[Hd/16][Hd/16])* then (b[Hd])* | fc2 f32-frag[1][Hd/16] b[16]
      pi_global (StarGambit): W1 f32-frag[Hp/16][4] b1 | W2 f32-frag[2][Hp/16] b2[32] | LayerNorm g[32] b[32]."""
    spec = net.spec
    Cin, H, W = spec.in_shape
    if not (spec.num_channels <= 64 and spec.head_channels <= 64 and spec.kernel_size == 3 and spec.head_pool and Cin <= 64
            and spec.v_head_convs == 1 and spec.pi_head_convs == 1 and (H, W) in ((11, 11), (7, 7), (13, 13))):
        raise RuntimeError("the bf16 MFMA spatial-head kernel covers the configs/tawlbwrdd.yaml, configs/open_tafl.yaml, "
                           "configs/brandubh.yaml and configs/star_gambit_unified.yaml nets (11x11, 7x7 or 13x13, <= 64 trunk / head "
                           "channels, one extra conv per head); use precision='fp32' for other shapes")
    pc = spec.policy_shape[0]
    Hd, L, P1 = spec.v_fc_hidden, spec.v_fc_layers, spec.num_players + 1
    # the bounds of azmi_net_create (csrc/leafnet_sp_host.hip refusal) that the paddings below rely on, with its messages
    if pc > 32 or not 0 <= spec.num_moves - pc * H * W <= 32:
        raise RuntimeError("spatial head: policy channels <= 32, 0..32 global actions")
    if spec.num_moves > pc * H * W and (spec.pi_fc_hidden < 64 or spec.pi_fc_hidden > 1024 or spec.pi_fc_hidden % 64):
        raise RuntimeError("spatial head with global actions: pi_hidden must be a multiple of 64 in [64, 1024]")
    if Hd > 512 or Hd % 128 or Hd < 128 or L < 1 or P1 > 16 or P1 < 2:
        raise RuntimeError("value head sizes out of range")
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    stream, prm = bytearray(), bytearray()
    # x3 (precision "bf16x3", csrc/leafnet_sp.h Geo<.., SPLIT>): every 8 KB chunk three times - high parts, high parts, low parts
    _frags = _split_frags if x3 else globals()["_frags"]
    _conv_frags = (lambda w_: _split_frags(_pad(w_.permute(0, 2, 3, 1), 64, 3, 3, 64).reshape(64, 576).numpy())) if x3 else globals()["_conv_frags"]
    a, b = (t.cpu() for t in bn_affine(net.bn1))
    w = sd["conv1.weight"] * a[:, None, None, None]
    if Cin <= 8:    # k = tap * 8 + ci, K = 72 padded to 128 (csrc/leafnet_sp.h stem_chunks)
        stream += _frags(_pad(_pad(w.permute(0, 2, 3, 1), 64, 3, 3, 8).reshape(64, 72), 64, 128).numpy())
    else:
        stream += _conv_frags(w)
    prm += _f32(_pad(b, 64))
    for i, blk in enumerate(net.conv_layers):
        a1, b1 = (t.cpu() for t in bn_affine(blk.bn1))
        a2, b2 = (t.cpu() for t in bn_affine(blk.bn2))
        stream += _conv_frags(sd[f"conv_layers.{i}.conv1.weight"] * a2[:, None, None, None])
        stream += _conv_frags(sd[f"conv_layers.{i}.conv2.weight"])
        prm += _f32(_pad(a1, 64)) + _f32(_pad(b1, 64)) + _f32(_pad(b2, 64))
    av, bv = (t.cpu() for t in bn_affine(net.v_bn))
    ap, bp = (t.cpu() for t in bn_affine(net.pi_bn))
    stream += _frags(_pad(sd["v_conv.weight"][:, :, 0, 0] * av[:, None], 64, 64).numpy())
    stream += _frags(_pad(sd["pi_conv.weight"][:, :, 0, 0] * ap[:, None], 64, 64).numpy())
    prm += _f32(torch.cat([_pad(bv, 64), _pad(bp, 64)]))
    for seq, name in ((net.v_extra_convs, "v_extra_convs"), (net.pi_extra_convs, "pi_extra_convs")):
        a, b = (t.cpu() for t in bn_affine(seq[1]))
        stream += _conv_frags(sd[f"{name}.0.weight"] * a[:, None, None, None])
        prm += _f32(_pad(b, 64))
    a2, b2 = (t.cpu() for t in bn_affine(net.pi_bn2))
    stream += _frags(_pad(sd["pi_conv2.weight"][:, :, 0, 0] * a2[:, None], 64, 64).numpy())
    prm += _f32(_pad(b2, 32))
    assert len(stream) == (3 if x3 else 1) * ((2 if Cin <= 8 else 9) + 18 * spec.depth + 2 + 18 + 1) * 8192
    blob = stream + prm
    blob += _f32_frags(_pad(sd["v_fc1.weight"], Hd, 64).numpy()) + _f32(sd["v_fc1.bias"])
    for l in range(L - 1):
        blob += _f32_frags(sd[f"v_fc_extra.{2 * l}.weight"].numpy())
    for l in range(L - 1):
        blob += _f32(sd[f"v_fc_extra.{2 * l}.bias"])
    blob += _f32_frags(_pad(sd["v_fc2.weight"], 16, Hd).numpy()) + _f32(_pad(sd["v_fc2.bias"], 16))
    G = spec.num_moves - pc * H * W
    Hp = spec.pi_fc_hidden if G > 0 else 0
    if G > 0:   # pi_global (neural_net.py:421-426): head channels zero-padded to 64, outputs to 32
        blob += _f32_frags(_pad(sd["pi_global.0.weight"], Hp, 64).numpy()) + _f32(sd["pi_global.0.bias"])
        blob += _f32_frags(_pad(sd["pi_global.2.weight"], 32, Hp).numpy()) + _f32(_pad(sd["pi_global.2.bias"], 32))
        blob += _f32(_pad(sd["pi_global.3.weight"], 32)) + _f32(_pad(sd["pi_global.3.bias"], 32))
    desc = NetDescC(Cin, H, W, 64, spec.depth, 3, 64, Hd, spec.num_moves, spec.num_players, 1, 1, L, pc, 2 if x3 else 0, Hp)
    assert len(blob) == lib.azmi_net_blob_bytes(C.byref(desc)), (len(blob), lib.azmi_net_blob_bytes(C.byref(desc)))
    return desc, bytes(blob)


def fold_fp32(net):
    """fp32 path (csrc/leafnet_f32.hip): torch layouts, BatchNorms folded in double, no bf16 anywhere.  A ResNet trunk (3x3 only, as
    before) gets the first descriptor and azmi_net_create; a dense trunk (kernel sizes 1 / 3 / 5 / 7, its extra head convolutions
    included) the second one (NetDesc2C) and azmi_net_create2, and so does every net with trunk_norm="layer", trunk_act="crelu" or
    pi_fc_layers > 0, either trunk (the image of those: csrc/leafnet_f32.hip, "variants").  A batch / relu net without the FC stack
    gets byte for byte the image it always got."""
    spec = net.spec
    Cin, H, W = spec.in_shape
    if not ((spec.kernel_size == 3 or spec.dense_net) and spec.head_pool):
        raise RuntimeError("fp32 leaf net: 3x3 convolutions (dense trunks: 1, 3, 5 or 7) and pooled value / global-action heads only")
    if spec.dense_net and spec.depth < 1:
        raise RuntimeError("fp32 leaf net: a dense trunk needs at least one block")
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    blob = bytearray()

    def conv_bn(wname, bn):
        a, b = (t.cpu() for t in bn_affine(bn))
        return _f32(sd[wname] * a[:, None, None, None]) + _f32(b)

    def conv_gn(wname, gname):      # layer norm folds into nothing: the raw weight, then the norm's weight and bias
        return _f32(sd[wname]) + _f32(sd[gname + ".weight"]) + _f32(sd[gname + ".bias"])

    if spec.trunk_norm == "layer":  # g1 b1 | W1 | g2 b2 | W2 (crelu: the weights have their 2 * Cin input channels as they are)
        if not spec.dense_net:
            blob += conv_gn("conv1.weight", "bn1")
        for i in range(spec.depth):
            pre = f"conv_layers.{i}."
            blob += _f32(sd[pre + "bn1.weight"]) + _f32(sd[pre + "bn1.bias"]) + conv_gn(pre + "conv1.weight", pre + "bn2") + _f32(sd[pre + "conv2.weight"])
    else:
        if not spec.dense_net:
            blob += conv_bn("conv1.weight", net.bn1)
        for i, blk in enumerate(net.conv_layers):   # both kinds of block: bn1's affine as it is, bn2 folded into conv1, conv2 raw
            a1, b1 = (t.cpu() for t in bn_affine(blk.bn1))
            blob += _f32(a1) + _f32(b1) + conv_bn(f"conv_layers.{i}.conv1.weight", blk.bn2) + _f32(sd[f"conv_layers.{i}.conv2.weight"])
    blob += conv_bn("v_conv.weight", net.v_bn)
    for i in range(spec.v_head_convs):
        blob += conv_bn(f"v_extra_convs.{3 * i}.weight", net.v_extra_convs[3 * i + 1])
    blob += _f32(sd["v_fc1.weight"]) + _f32(sd["v_fc1.bias"])
    for l in range(spec.v_fc_layers - 1):
        blob += _f32(sd[f"v_fc_extra.{2 * l}.weight"]) + _f32(sd[f"v_fc_extra.{2 * l}.bias"])
    blob += _f32(sd["v_fc2.weight"]) + _f32(sd["v_fc2.bias"])
    blob += conv_bn("pi_conv.weight", net.pi_bn)
    for i in range(spec.pi_head_convs):
        blob += conv_bn(f"pi_extra_convs.{3 * i}.weight", net.pi_extra_convs[3 * i + 1])
    pc = 0
    if spec.policy_shape is not None:
        pc = spec.policy_shape[0]
        blob += conv_bn("pi_conv2.weight", net.pi_bn2)
        if spec.num_moves > pc * H * W:   # pi_global: torch layouts
            for k in ("pi_global.0.weight", "pi_global.0.bias", "pi_global.2.weight", "pi_global.2.bias", "pi_global.3.weight", "pi_global.3.bias"):
                blob += _f32(sd[k])
    else:
        blob += _f32(sd["pi_fc1.weight"]) + _f32(sd["pi_fc1.bias"])
        if spec.pi_fc_layers > 0:
            for l in range(spec.pi_fc_layers - 1):
                blob += _f32(sd[f"pi_fc_extra.{2 * l}.weight"]) + _f32(sd[f"pi_fc_extra.{2 * l}.bias"])
            blob += _f32(sd["pi_fc_out.weight"]) + _f32(sd["pi_fc_out.bias"])
    desc = NetDescC(Cin, H, W, spec.num_channels, spec.depth, spec.kernel_size, spec.head_channels, spec.v_fc_hidden, spec.num_moves,
                    spec.num_players, spec.v_head_convs, spec.pi_head_convs, spec.v_fc_layers, pc, 1,
                    spec.pi_fc_hidden if ((pc and spec.num_moves > pc * H * W) or spec.pi_fc_layers > 0) else 0)
    if spec.dense_net or is_variant(spec):
        desc = NetDesc2C(desc, int(spec.dense_net))
        desc.trunk_norm, desc.trunk_act, desc.pi_fc_layers = int(spec.trunk_norm == "layer"), int(spec.trunk_act == "crelu"), spec.pi_fc_layers
    assert len(blob) == blob_bytes(desc), (len(blob), blob_bytes(desc))
    return desc, bytes(blob)


def _up(x, m):
    return (x + m - 1) // m * m


def fold_dense(net):
    """The dense Connect4 family on the matrix cores (csrc/leafnet_dense.h; bf16 operands): 6x7, flat policy head, kernel_size 3 or
    5, growth G <= 16, C_in + G*depth <= 128, head_channels 32.  Narrower widths are zero-padded: the padded channels have zero
    scale, bias and weights and stay exactly 0.  Image (`frag` = hip_net._frags: [k-step][m-tile][64 lanes][8 bf16]; CF = C_in +
    G*depth, CFP = CF rounded up to 32, C_i = C_in + G*i):
      block i  a1[CFP] b1[CFP] (bn1 of the block over the raw features, zero behind C_i) c1[64] (bn2's bias) f32 |
               W1 frag[roundup32(C_i)/32][ceil(4G/16)] (rows = bn2-scaled conv1, k = input channel) |
               W2: per tap (dy, dx) row-major frag[ceil(4G/32)][1] (rows = the G outputs, rows >= G zero; k = bottleneck channel)
      heads    bh[64] f32 | Wh frag[CFP/32][4] (rows 0-31 = v_conv * v_bn, rows 32-63 = pi_conv * pi_bn)
      v_fc1 W[Hd][32] b[Hd] | v_fc2 W[P+1][Hd] b[P+1] | pi_fc1 W[M][32*42] b[M]   (f32, torch layouts)
    trunk_norm="layer" (the kernel's LAYER instance; trunk_act relu, no policy FC stack): nothing folds -
      block i  g1[CFP] b1[CFP] (bn1's weight and bias, zero behind C_i) g2[64] b2[64] (bn2's, zero behind 4G) f32 | W1 (raw rows) | W2"""
    spec = net.spec
    Cin, H, W = spec.in_shape
    G, D, K = spec.num_channels, spec.depth, spec.kernel_size
    tail = "; use precision='fp32' for other shapes"
    # the bounds of azmi_net_create2 (csrc/leafnet_dense_host.hip refusal), with its messages
    layer = spec.trunk_norm == "layer"
    if spec.trunk_act != "relu" or spec.pi_fc_layers > 0:   # (crelu would double K beyond the LDS plan; no tile has the policy FC stack)
        raise RuntimeError("dense leaf net kernel: trunk_act='relu' and pi_fc_layers=0 only; use precision='fp32' for crelu and the policy FC stack")
    if spec.policy_shape is not None or (H, W) != (6, 7):
        raise RuntimeError("dense leaf net kernel covers the 6x7 board with the flat policy head" + tail)
    if K not in (3, 5):
        raise RuntimeError("dense leaf net kernel: kernel_size 3 or 5" + tail)
    if not 1 <= G <= 16:
        raise RuntimeError("dense leaf net kernel: growth rate (channels) 1..16" + tail)
    if D < 1 or Cin < 1:
        raise RuntimeError("dense leaf net kernel: at least one block and one input plane" + tail)
    if Cin + G * D > 128:
        raise RuntimeError("dense leaf net kernel: in_channels + channels * depth <= 128" + tail)
    if not (spec.head_channels == 32 and spec.head_pool and spec.v_head_convs == 0 and spec.pi_head_convs == 0 and spec.v_fc_layers == 1):
        raise RuntimeError("dense leaf net kernel: 32 head channels, pooled value head, no extra head convolutions, one value FC layer" + tail)
    if not (16 <= spec.v_fc_hidden <= 256 and spec.v_fc_hidden % 16 == 0 and 1 <= spec.num_players <= 3 and 1 <= spec.num_moves <= 16):
        raise RuntimeError("dense leaf net kernel: head sizes out of range (v_hidden: a multiple of 16, at most 256; 1..3 players; "
                           "1..16 moves)" + tail)
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    CF = Cin + G * D
    CFP, M1, K2 = _up(CF, 32), _up(4 * G, 16), _up(4 * G, 32)
    blob = bytearray()
    for i, blk in enumerate(net.conv_layers):
        Ci = Cin + G * i
        if layer:
            pre = f"conv_layers.{i}."
            blob += _f32(_pad(sd[pre + "bn1.weight"], CFP)) + _f32(_pad(sd[pre + "bn1.bias"], CFP))
            blob += _f32(_pad(sd[pre + "bn2.weight"], 64)) + _f32(_pad(sd[pre + "bn2.bias"], 64))
            blob += _frags(_pad(sd[pre + "conv1.weight"][:, :, 0, 0], M1, _up(Ci, 32)).numpy())
        else:
            a1, b1 = (t.cpu() for t in bn_affine(blk.bn1))
            a2, b2 = (t.cpu() for t in bn_affine(blk.bn2))
            blob += _f32(_pad(a1, CFP)) + _f32(_pad(b1, CFP)) + _f32(_pad(b2, 64))
            blob += _frags(_pad(sd[f"conv_layers.{i}.conv1.weight"][:, :, 0, 0] * a2[:, None], M1, _up(Ci, 32)).numpy())
        w2 = sd[f"conv_layers.{i}.conv2.weight"]                     # [G][4G][K][K]
        for dy in range(K):
            for dx in range(K):
                blob += _frags(_pad(w2[:, :, dy, dx], 16, K2).numpy())
    av, bv = (t.cpu() for t in bn_affine(net.v_bn))
    ap, bp = (t.cpu() for t in bn_affine(net.pi_bn))
    wh = torch.cat([sd["v_conv.weight"][:, :, 0, 0] * av[:, None], sd["pi_conv.weight"][:, :, 0, 0] * ap[:, None]], 0)
    blob += _f32(torch.cat([bv, bp])) + _frags(_pad(wh, 64, CFP).numpy())
    blob += _f32(sd["v_fc1.weight"]) + _f32(sd["v_fc1.bias"]) + _f32(sd["v_fc2.weight"]) + _f32(sd["v_fc2.bias"])
    blob += _f32(sd["pi_fc1.weight"]) + _f32(sd["pi_fc1.bias"])
    desc = NetDesc2C(NetDescC(Cin, H, W, G, D, K, 32, spec.v_fc_hidden, spec.num_moves, spec.num_players, 0, 0, 1, 0, 0, 0), 1)
    desc.trunk_norm = int(layer)
    assert len(blob) == blob_bytes(desc), (len(blob), blob_bytes(desc))
    return desc, bytes(blob)


def fold_dense_spatial(net):
    """The dense spatial-head family on the matrix cores (csrc/leafnet_dense_sp.h; bf16 operands): the single-variant StarGambit
    configs and their neighbours - 7x7, 11x11 or 13x13, spatial policy head with up to 32 channels and up to 32 global actions,
    kernel_size 3 or 5, growth G <= 16, C_in + G*depth <= 128, head_channels 32.  The blocks are laid out exactly as fold_dense
    lays them out (the same fragments, the same exact zeros in every padding).  The heads' 1x1 has split operands:
      heads    bh[64] f32 | frag[CFP/32][4] of the bf16 high parts of Wh | frag[CFP/32][4] of the low parts (Wh - high, in bf16)
    and behind it, all f32:
      v_fc1 W[Hd][32] b[Hd] | v_fc2 W[P+1][Hd] b[P+1] | pi_conv2 W[32][32] b[32] (pi_bn2 folded; rows >= policy channels zero)
      with global actions: pi_global.0 W[Hp][32] b[Hp] | pi_global.2 W[NG][Hp] b[NG] | LayerNorm g[NG] b[NG]   (torch layouts)"""
    spec = net.spec
    Cin, H, W = spec.in_shape
    G, D, K = spec.num_channels, spec.depth, spec.kernel_size
    tail = "; use precision='fp32' for other shapes"
    # the bounds of azmi_net_create2 (csrc/leafnet_dense_sp_host.hip refusal), with its messages
    if spec.trunk_act != "relu" or spec.pi_fc_layers > 0:
        raise RuntimeError("dense leaf net kernel: trunk_act='relu' and pi_fc_layers=0 only; use precision='fp32' for crelu and the policy FC stack")
    if spec.trunk_norm != "batch":
        raise RuntimeError("dense spatial leaf net kernel: trunk_norm='batch' only (the layer-norm instance is the dense Connect4 tile's); "
                           "use precision='fp32' for layer-norm nets")
    pc = spec.policy_shape[0]
    NG = spec.num_moves - pc * H * W
    if (H, W) not in ((7, 7), (11, 11), (13, 13)):
        raise RuntimeError("dense spatial leaf net kernel covers 7x7, 11x11 and 13x13 boards" + tail)
    if K not in (3, 5):
        raise RuntimeError("dense spatial leaf net kernel: kernel_size 3 or 5" + tail)
    if not 1 <= G <= 16:
        raise RuntimeError("dense spatial leaf net kernel: growth rate (channels) 1..16" + tail)
    if D < 1 or Cin < 1:
        raise RuntimeError("dense spatial leaf net kernel: at least one block and one input plane" + tail)
    if Cin + G * D > 128:
        raise RuntimeError("dense spatial leaf net kernel: in_channels + channels * depth <= 128" + tail)
    if not (spec.head_channels == 32 and spec.head_pool and spec.v_head_convs == 0 and spec.pi_head_convs == 0 and spec.v_fc_layers == 1):
        raise RuntimeError("dense spatial leaf net kernel: 32 head channels, pooled heads, no extra head convolutions, one value FC layer" + tail)
    if not (1 <= pc <= 32 and 0 <= NG <= 32):
        raise RuntimeError("dense spatial leaf net kernel: policy channels 1..32, 0..32 global actions" + tail)
    Hp = spec.pi_fc_hidden if NG > 0 else 0
    if NG > 0 and not (16 <= Hp <= 256 and Hp % 16 == 0):
        raise RuntimeError("dense spatial leaf net kernel: pi_hidden must be a multiple of 16 in 16..256 with global actions" + tail)
    if not (16 <= spec.v_fc_hidden <= 256 and spec.v_fc_hidden % 16 == 0 and 1 <= spec.num_players <= 3):
        raise RuntimeError("dense spatial leaf net kernel: head sizes out of range (v_hidden: a multiple of 16, at most 256; 1..3 players)" + tail)
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    CF = Cin + G * D
    CFP, M1, K2 = _up(CF, 32), _up(4 * G, 16), _up(4 * G, 32)
    blob = bytearray()
    for i, blk in enumerate(net.conv_layers):
        Ci = Cin + G * i
        a1, b1 = (t.cpu() for t in bn_affine(blk.bn1))
        a2, b2 = (t.cpu() for t in bn_affine(blk.bn2))
        blob += _f32(_pad(a1, CFP)) + _f32(_pad(b1, CFP)) + _f32(_pad(b2, 64))
        blob += _frags(_pad(sd[f"conv_layers.{i}.conv1.weight"][:, :, 0, 0] * a2[:, None], M1, _up(Ci, 32)).numpy())
        w2 = sd[f"conv_layers.{i}.conv2.weight"]                     # [G][4G][K][K]
        for dy in range(K):
            for dx in range(K):
                blob += _frags(_pad(w2[:, :, dy, dx], 16, K2).numpy())
    av, bv = (t.cpu() for t in bn_affine(net.v_bn))
    ap, bp = (t.cpu() for t in bn_affine(net.pi_bn))
    wh = torch.cat([sd["v_conv.weight"][:, :, 0, 0] * av[:, None], sd["pi_conv.weight"][:, :, 0, 0] * ap[:, None]], 0)
    wh = _pad(wh, 64, CFP)
    wh_hi = wh.float().to(torch.bfloat16).double()
    blob += _f32(torch.cat([bv, bp])) + _frags(wh_hi.numpy()) + _frags((wh - wh_hi).numpy())
    blob += _f32(sd["v_fc1.weight"]) + _f32(sd["v_fc1.bias"]) + _f32(sd["v_fc2.weight"]) + _f32(sd["v_fc2.bias"])
    a2, b2 = (t.cpu() for t in bn_affine(net.pi_bn2))
    blob += _f32(_pad(sd["pi_conv2.weight"][:, :, 0, 0] * a2[:, None], 32, 32)) + _f32(_pad(b2, 32))
    if NG > 0:
        for k in ("pi_global.0.weight", "pi_global.0.bias", "pi_global.2.weight", "pi_global.2.bias", "pi_global.3.weight", "pi_global.3.bias"):
            blob += _f32(sd[k])
    desc = NetDesc2C(NetDescC(Cin, H, W, G, D, K, 32, spec.v_fc_hidden, spec.num_moves, spec.num_players, 0, 0, 1, pc, 0, Hp), 1)
    assert len(blob) == blob_bytes(desc), (len(blob), blob_bytes(desc))
    return desc, bytes(blob)


def _split_frags(wmat, passes=("hi", "hi", "lo")):
    """wmat [64][K] (K = 64 * taps) -> the bf16x3 weight stream of one convolution: per tap (two k-steps = one 8 KB chunk) the
    high parts' fragments, the high parts' again, the low parts' (w = hi + lo; csrc/leafnet_c4.h SPLIT: the three chunks meet
    the activations' high, low and high planes)."""
    w = torch.as_tensor(np.ascontiguousarray(wmat), dtype=torch.float64)
    hi = w.float().to(torch.bfloat16).double()
    lo = w - hi
    fh = np.frombuffer(_frags(hi.numpy()), np.int16).reshape(-1, 2, 4, 64, 8)     # [tap][2 k-steps][4 m-tiles][64 lanes][8]
    fl = np.frombuffer(_frags(lo.numpy()), np.int16).reshape(-1, 2, 4, 64, 8)
    out = bytearray()
    for t in range(fh.shape[0]):
        for which in passes:
            out += (fh if which == "hi" else fl)[t].tobytes()
    return bytes(out)


def fold(net, precision="bf16"):
    """LeafNet (reference NNArch parameter names) -> (NetDescC or NetDesc2C, blob bytes).  precision: "bf16" (bf16 MFMA operands),
    "bf16x3" (weights and activations as bf16 high + low parts, three MFMAs per product - the 1e-5 tier on the matrix cores; the
    Connect4 family and, since round 4, the spatial-head nets) or "fp32" (plain fp32 kernels, any shape).  A dense trunk
    (spec.dense_net) has the "bf16" tiles of fold_dense (6x7, flat policy head) and fold_dense_spatial (7x7 / 11x11 / 13x13, spatial
    policy head) and "fp32".  trunk_norm="layer", trunk_act="crelu" and pi_fc_layers > 0
    have "fp32"; a dense trunk with trunk_norm="layer" alone also has the "bf16" tile; everything else raises RuntimeError naming
    precision='fp32'."""
    if precision == "fp32":
        return fold_fp32(net)
    spec = net.spec
    x3 = precision == "bf16x3"
    if precision not in ("bf16", "bf16x3"):
        raise ValueError("precision must be 'bf16', 'bf16x3' or 'fp32'")
    tile_layer = spec.dense_net and not x3 and spec.trunk_norm == "layer" and spec.trunk_act == "relu" and spec.pi_fc_layers == 0
    if is_variant(spec) and not tile_layer:    # azmi_net_create2's refusal (csrc/leafnet.hip resolve2, kVariantOnTile), before anything is laid out
        raise RuntimeError("the matrix-core tiles cover trunk_act='relu' and pi_fc_layers=0, with trunk_norm='batch' or, on the dense "
                           "Connect4 tile (precision 'bf16'), 'layer'; use precision='fp32' for the other layer-norm nets, crelu and "
                           "the policy FC stack")
    if spec.dense_net:
        if x3:
            raise RuntimeError("dense leaf net: no bf16x3 tier; the 1e-5 tier of dense nets is precision='fp32'")
        if spec.policy_shape is not None and tuple(spec.in_shape[1:]) != (6, 7):   # (a spatial head ON 6x7: the Connect4 tile's refusal)
            return fold_dense_spatial(net)
        return fold_dense(net)
    if spec.policy_shape is not None:
        return fold_spatial(net, x3)
    Cin, H, W = spec.in_shape
    if not (spec.num_channels == 64 and spec.head_channels == 32 and spec.kernel_size == 3 and spec.policy_shape is None
            and spec.head_pool and spec.v_head_convs == 0 and spec.pi_head_convs == 0 and spec.v_fc_layers == 1
            and 9 * Cin <= 64 and (H, W) == (6, 7)):
        raise RuntimeError("the bf16 MFMA flat-head kernel covers the Connect4 net family (6x7, 64 trunk / 32 head channels, "
                           "flat policy head); use precision='fp32' for other shapes")
    if not (16 <= spec.v_fc_hidden <= 256 and 1 <= spec.num_players <= 3 and 1 <= spec.num_moves <= 16) and spec.v_fc_hidden % 16 == 0:
        raise RuntimeError("head sizes out of range (v_hidden: a multiple of 16, at most 256)")      # azmi_net_create's bound and message
    sd ={k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    blob = bytearray()
    # stem: conv1 * bn1
    a, b = bn_affine(net.bn1)
    a, b = a.cpu(), b.cpu()
    w = sd["conv1.weight"] * a[:, None, None, None]                  # [64][Cin][3][3]
    wm = np.zeros((64, 64))
    wm[:, : 9 * Cin] = w.permute(0, 2, 3, 1).reshape(64, 9 * Cin).numpy()  # k = tap*Cin + ci
    blob += (_split_frags(wm, ("hi", "lo")) if x3 else _frags(wm)) + _f32(b)       # (inputs are 0 / 1: only the weights split)
    conv = (lambda m: _split_frags(m)) if x3 else _frags
    for i, blk in enumerate(net.conv_layers):
        a1, b1 = (t.cpu() for t in bn_affine(blk.bn1))
        a2, b2 = (t.cpu() for t in bn_affine(blk.bn2))
        w1 = sd[f"conv_layers.{i}.conv1.weight"] * a2[:, None, None, None]
        w2 = sd[f"conv_layers.{i}.conv2.weight"]
        blob += _f32(a1) + _f32(b1) + _f32(b2)
        blob += conv(w1.permute(0, 2, 3, 1).reshape(64, 576).numpy())   # k = tap*64 + ci
        blob += conv(w2.permute(0, 2, 3, 1).reshape(64, 576).numpy())
    av, bv = (t.cpu() for t in bn_affine(net.v_bn))
    ap, bp = (t.cpu() for t in bn_affine(net.pi_bn))
    wh = torch.cat([sd["v_conv.weight"][:, :, 0, 0] * av[:, None], sd["pi_conv.weight"][:, :, 0, 0] * ap[:, None]], 0)
    blob += conv(wh.numpy()) + _f32(torch.cat([bv, bp]))
    # value fc1 for v_mfma_f32_16x16x4_f32 (csrc/leafnet_c4.h): A-fragments [hidden / 16][2][64 lanes][4]
    if spec.v_fc_hidden % 16:
        raise RuntimeError("the Connect4-family tile wants v_fc_hidden to be a multiple of 16")
    blob += _f32_frags(sd["v_fc1.weight"].numpy()) + _f32(sd["v_fc1.bias"])
    blob += _f32(sd["v_fc2.weight"]) + _f32(sd["v_fc2.bias"])
    # flat policy head: the reference's feature order is (c, h, w) -> c*HW + p.  The kernel contracts one pixel position p at
    # a time on the bf16 matrix pipe, logits[m] += W_p[m][c] h[c][p], with W and h split into bf16 high + low parts:
    # per p one A-fragment of the high parts of W_p (16 rows, rows >= num_moves zero), then one of the low parts
    wp = torch.zeros((16, 32, H * W), dtype=torch.float64)
    wp[: spec.num_moves] = sd["pi_fc1.weight"].reshape(spec.num_moves, 32, H * W)
    hi = wp.float().to(torch.bfloat16).double()
    lo = wp - hi
    for p_ in range(H * W):
        blob += _frags(hi[:, :, p_].numpy()) + _frags(lo[:, :, p_].numpy())
    blob += _f32(sd["pi_fc1.bias"])
    desc = NetDescC(Cin, H, W, 64, spec.depth, 3, 32, spec.v_fc_hidden, spec.num_moves, spec.num_players, 0, 0, 1, 0, 2 if x3 else 0, 0)
    assert len(blob) == lib.azmi_net_blob_bytes(C.byref(desc)), (len(blob), lib.azmi_net_blob_bytes(C.byref(desc)))
    return desc, bytes(blob)


# AZMI_PARAM_* (include/azmi.h)
PARAM_CONV_W, PARAM_BN_WEIGHT, PARAM_BN_BIAS, PARAM_BN_MEAN, PARAM_BN_VAR, PARAM_FC_W, PARAM_FC_B = range(7)
_BN_TENSORS = (("weight", PARAM_BN_WEIGHT), ("bias", PARAM_BN_BIAS), ("running_mean", PARAM_BN_MEAN), ("running_var", PARAM_BN_VAR))


def _refresh_family(spec, precision):
    """Which of the two families HipLeafNet.refresh is built for a (spec, precision) belongs to: "resnet" (the Connect4 ResNet
    flat-head tile, fold lines for "bf16" / "bf16x3") or "dense" (the dense Connect4 tile's batch-norm instance, fold_dense).  The
    decision tree is fold()'s; every other family raises RuntimeError naming itself."""
    if precision == "fp32":
        other = "the fp32 tier"
    elif precision not in ("bf16", "bf16x3"):
        raise ValueError("precision must be 'bf16', 'bf16x3' or 'fp32'")
    elif spec.dense_net and spec.policy_shape is not None and tuple(spec.in_shape[1:]) != (6, 7):
        other = "the dense spatial-head tile"
    elif spec.dense_net and spec.trunk_norm == "layer":
        other = "the dense tile's layer-norm instance"
    elif is_variant(spec):
        other = "a layer-norm / crelu / policy-FC-stack net"
    elif spec.dense_net:
        return "dense"
    elif spec.policy_shape is not None:
        other = "the spatial-head tile"
    else:
        return "resnet"
    raise RuntimeError(f"refresh is built for the Connect4 ResNet flat-head tile and the dense Connect4 tile (batch norm), not for {other}: "
                       "build a new HipLeafNet from the trained model")


def refresh_names(spec, precision="bf16"):
    """The ordered tensor names (state_dict keys) of the table HipLeafNet.refresh hands to azmi_net_refresh: every tensor fold() /
    fold_dense() reads for this family, each once - the table order of csrc/leafnet_c4_host.hip / leafnet_dense_host.hip
    (refresh_plan).  Pure Python, no device.  Families refresh is not built for raise RuntimeError naming the family."""
    family = _refresh_family(spec, precision)

    def bn(prefix):
        return [f"{prefix}.{t}" for t, _ in _BN_TENSORS]
    names = (["conv1.weight"] + bn("bn1")) if family == "resnet" else []      # (a dense trunk has no stem)
    for i in range(spec.depth):
        pre = f"conv_layers.{i}."
        names += bn(pre + "bn1") + [pre + "conv1.weight"] + bn(pre + "bn2") + [pre + "conv2.weight"]
    names += ["v_conv.weight"] + bn("v_bn") + ["pi_conv.weight"] + bn("pi_bn")
    return names + ["v_fc1.weight", "v_fc1.bias", "v_fc2.weight", "v_fc2.bias", "pi_fc1.weight", "pi_fc1.bias"]


def _param_kind(module, tensor):
    if isinstance(module, torch.nn.BatchNorm2d):
        return dict(_BN_TENSORS)[tensor]
    if isinstance(module, torch.nn.Linear):
        return PARAM_FC_W if tensor == "weight" else PARAM_FC_B
    return PARAM_CONV_W


class HipLeafNet:
    """The fused MFMA kernel as an evaluator: forward(canonical, v_out, pi_out) on device tensors."""

    def __init__(self, net, spec=None, max_batch=None, device=0, precision="bf16"):
        """precision: "bf16" = MFMA fast path (bf16 operands, fp32 accumulate); "bf16x3" = the same tile with split operands
        (hi + lo bf16 parts, three MFMAs per product; Connect4 family): the 1e-5 tier on the matrix cores; "fp32" = plain fp32
        kernels for any shape."""
        self.desc, blob = fold(net, precision)
        self.precision, self.device = precision, int(device)
        self.spec = dataclasses.replace(net.spec)      # what refresh() compares a model against
        self._blob = blob
        h = C.c_void_p()
        create = lib.azmi_net_create2 if isinstance(self.desc, NetDesc2C) else lib.azmi_net_create    # dense trunk
        rc = create(C.byref(self.desc), blob, len(blob), int(device), C.byref(h))
        if rc != 0:
            raise RuntimeError(lib.azmi_net_last_error().decode())
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.azmi_net_destroy(self._h)
            self._h = None

    def forward(self, canonical, v_out, pi_out, stream=None):
        n = canonical.shape[0]
        assert canonical.dtype == torch.float32 and canonical.is_contiguous() and v_out.is_contiguous() and pi_out.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        rc = lib.azmi_net_forward(self._h, canonical.data_ptr(), v_out.data_ptr(), pi_out.data_ptr(), n, C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(lib.azmi_net_last_error().decode())

    def forward_rows(self, canonical, v_out, pi_out, rows, row_count, max_rows=None, stream=None):
        """azmi_net_forward_rows: evaluate the slots rows[0 .. row_count[0]) of `canonical` into the same slots of v_out / pi_out
        and touch no other slot.  `rows` (int32 / uint32, at least max_rows entries, every one a valid slot) and `row_count`
        (one element) are DEVICE tensors read when the kernels run; max_rows (default len(rows)) bounds the count and
        sizes the launch."""
        if max_rows is None:
            max_rows = rows.numel()
        assert canonical.dtype == torch.float32 and canonical.is_contiguous() and v_out.is_contiguous() and pi_out.is_contiguous()
        assert v_out.dtype == torch.float32 and pi_out.dtype == torch.float32
        assert rows.is_cuda and row_count.is_cuda and rows.is_contiguous() and rows.element_size() == 4 and row_count.element_size() == 4
        assert not rows.dtype.is_floating_point and not row_count.dtype.is_floating_point
        assert 0 <= max_rows <= rows.numel() and row_count.numel() >= 1
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        rc = lib.azmi_net_forward_rows(self._h, canonical.data_ptr(), v_out.data_ptr(), pi_out.data_ptr(), rows.data_ptr(),
                                       row_count.data_ptr(), int(max_rows), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(lib.azmi_net_last_error().decode())

    def refresh(self, net, stream=None):
        """The weights of the trained `net` (a torch_net.LeafNet on this net's GPU) written into THIS net in place
        (azmi_net_refresh): HIP kernels read the float32 parameters and buffers where they are, fold the BatchNorms in float64 and
        lay the image out, byte for byte the blob fold(net, precision) makes; nothing is copied to the host, nothing waits for the
        device, the handle and every engine, MCTSBatch or pipeline view holding it stay valid.  Returns self.
        Order: enqueued on `stream` (a raw HIP stream handle, default the current one).  A forward enqueued on that stream before the
        call sees the old weights whole, one enqueued after it the new ones whole; a forward on ANOTHER stream is the caller's to
        order against the refresh.  The model's tensors are read when the stream gets there: an optimiser step on another stream
        must be ordered behind it too.
        Refusals, all before any launch (the weights stay what they were): a spec that differs from the one this net was built with
        (ValueError naming the first differing field); a tensor that is missing, not float32, not contiguous or not on this net's
        device (RuntimeError naming it); a family refresh is not built for - the spatial-head tiles, the dense spatial tile, the dense
        layer-norm instance, the fp32 tier - (RuntimeError naming it: build a new HipLeafNet).
        A position cache filled under the old weights keeps serving the old answers: start a new one (selfplay.refresh_net)."""
        names = refresh_names(self.spec, self.precision)
        spec = getattr(net, "spec", None)
        if spec is None:
            raise ValueError("refresh: the model has no spec (a torch_net.LeafNet is expected)")
        for f in dataclasses.fields(self.spec):
            old, new = getattr(self.spec, f.name), getattr(spec, f.name)
            if (tuple(old) if isinstance(old, (list, tuple)) else old) != (tuple(new) if isinstance(new, (list, tuple)) else new):
                raise ValueError(f"refresh: the model's spec differs from the one this net was built with in {f.name}: {new!r}, built with {old!r}")
        tensors = dict(net.named_parameters())
        tensors.update(net.named_buffers())
        table = (NetParamC * len(names))()
        for rec, name in zip(table, names):
            t = tensors.get(name)
            if t is None:
                raise RuntimeError(f"refresh: the model has no tensor {name}")
            if not t.is_cuda or t.device.index != self.device:
                raise RuntimeError(f"refresh: {name} is on {t.device}, this net is on cuda:{self.device}")
            if t.dtype != torch.float32:
                raise RuntimeError(f"refresh: {name} is {t.dtype}, float32 is expected")
            if not t.is_contiguous():
                raise RuntimeError(f"refresh: {name} is not contiguous")
            prefix, _, leaf = name.rpartition(".")
            module = net.get_submodule(prefix)
            rec.data, rec.count, rec.kind = t.data_ptr(), t.numel(), _param_kind(module, leaf)
            rec.eps = float(module.eps) if leaf == "running_var" else 0.0
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if lib.azmi_net_refresh(self._h, table, len(names), C.c_void_p(int(stream))) != 0:
            raise RuntimeError(lib.azmi_net_last_error().decode())
        self._blob = None      # (the image of the constructor's model: no longer what the device holds)
        return self

    def blob(self):
        """The live weight image read back from the device (azmi_net_blob_read; synchronises: tests and debugging).  The fp32 tier
        keeps its image to itself and raises RuntimeError."""
        n = blob_bytes(self.desc)
        out = C.create_string_buffer(n)
        if lib.azmi_net_blob_read(self._h, out, n) != 0:
            raise RuntimeError(lib.azmi_net_last_error().decode())
        return out.raw

    @property
    def trunk_channels(self):
        """CF, the channels of the trunk's output (azmi_net_trunk_channels): num_channels for a ResNet trunk, in_channels +
        num_channels * depth for a dense one, whose features begin with the input planes.  precision="fp32" only: every other tier
        raises RuntimeError naming precision='fp32'."""
        cf = C.c_uint32()
        if lib.azmi_net_trunk_channels(self._h, C.byref(cf)) != 0:
            raise RuntimeError(lib.azmi_net_last_error().decode())
        return int(cf.value)

    def trunk_features(self, canonical, out=None, stream=None):
        """The pooled trunk activations NNWrapper.effective_rank reads (neural_net.py:848-866: the output of nnet.conv_layers, then
        mean(dim=(2, 3))): the stem and trunk launches of forward(), nothing of the heads, and one pooling launch
        (azmi_net_trunk_features).  canonical: contiguous float32 CUDA tensor [n, C, H, W]; -> float32 [n, trunk_channels] (`out`, or
        a new tensor), enqueued on `stream` (a raw HIP stream handle, default the current one) with no synchronisation.  A row's bits
        do not depend on n or on its place in the batch.  precision="fp32" only: every other tier raises RuntimeError naming
        precision='fp32', before any launch."""
        what = "trunk_features"
        cf = self.trunk_channels
        if not (hasattr(canonical, "is_cuda") and canonical.is_cuda):
            raise RuntimeError(f"{what}: canonical must be a CUDA tensor, got {type(canonical).__name__}")
        shape = (self.desc.in_channels, self.desc.height, self.desc.width)
        if canonical.dtype != torch.float32 or not canonical.is_contiguous() or tuple(canonical.shape[1:]) != shape or canonical.dim() != 4:
            raise RuntimeError(f"{what}: canonical must be a contiguous float32 [n, {shape[0]}, {shape[1]}, {shape[2]}] tensor, got "
                               f"{'contiguous' if canonical.is_contiguous() else 'non-contiguous'} {canonical.dtype} {tuple(canonical.shape)}")
        n = int(canonical.shape[0])
        if out is None:
            out = torch.empty((n, cf), dtype=torch.float32, device=canonical.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, cf) and out.device == canonical.device):
            raise RuntimeError(f"{what}: out must be a contiguous float32 [{n}, {cf}] tensor on {canonical.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        if stream is None:
            stream = torch.cuda.current_stream(canonical.device).cuda_stream
        if lib.azmi_net_trunk_features(self._h, canonical.data_ptr(), out.data_ptr(), n, C.c_void_p(int(stream))) != 0:
            raise RuntimeError(lib.azmi_net_last_error().decode())
        return out

    def process(self, canonical):
        """NNWrapper.process signature: returns (v, pi) probabilities as new float32 tensors."""
        n = canonical.shape[0]
        v = torch.empty((n, self.desc.num_players + 1), dtype=torch.float32, device=canonical.device)
        pi = torch.empty((n, self.desc.num_moves), dtype=torch.float32, device=canonical.device)
        self.forward(canonical.contiguous().float(), v, pi)
        return v, pi
