"""Shared by the leaf-net tests: the fp64 reference forward and the table of net descriptors.

The reference is the package's own `LeafNet` (the restated inference forward of the reference NNArch) run in float64 on
the CPU: torch's fp32 forward of the same nets stays within 5e-8 of it, 200 times inside the 1e-5 tier the fp32 / bf16x3
kernels are held to, so its own error is no part of any bound asserted against it.

The table: every bound `azmi_net_create` states, at both ends and once inside; shapes only the fp32 path takes; shapes
the MFMA tiers must refuse, each with a fragment of the message expected.  Boards are the smallest instantiated one
(7x7) and nets one block deep unless the case is about something else: the cases are about loop bounds, paddings and
offsets, not about throughput.
"""
import copy
from dataclasses import dataclass

import torch

TOL = 1e-3        # the project's bf16 figure (tests/test_gpu_leafnet.py)
TOL_F32 = 1e-5    # BASELINE.json north_star: 1e-5 on policy / value tensors


@torch.no_grad()
def reference(net, x):
    """fp64 CPU forward of a deep copy of `net`: (v, pi) = exp(log_softmax) as float64 tensors, and the raw policy logits."""
    ref = copy.deepcopy(net).cpu().double().eval()
    seen = {}
    spatial = ref.spec.policy_shape is not None
    names = (["pi_bn2"] + (["pi_global"] if ref.num_global_actions > 0 else [])) if spatial else ["pi_fc1"]
    hooks = [getattr(ref, n).register_forward_hook(lambda m, i, o, n=n: seen.__setitem__(n, o)) for n in names]
    lv, lpi = ref(x.detach().cpu().double())
    for h in hooks:
        h.remove()
    if spatial:     # LeafNet.forward: the spatial block as (h, w, c), the global actions behind it
        logits = seen["pi_bn2"].permute(0, 2, 3, 1).reshape(lpi.shape[0], -1)
        if "pi_global" in seen:
            logits = torch.cat([logits, seen["pi_global"]], dim=1)
    else:
        logits = seen["pi_fc1"]
    assert torch.allclose(torch.log_softmax(logits, dim=1), lpi, rtol=0, atol=1e-12)
    return torch.exp(lv), torch.exp(lpi), logits


def sparse_planes(spec, batch, seed, density=0.2, bf16_exact=False):
    """0 / 1 planes with the last plane fractional and constant per board (turn / max_turns of the Tafl family).
    bf16_exact: the fraction is a multiple of 1/64.  The Connect4-family tile takes its input planes as ONE bf16 value on
    every tier (csrc/leafnet_c4.h: "the input planes are 0 / 1 (exact in bf16): only the stem's weights have a low part"),
    so an input that bf16 cannot hold is outside what that tile promises; the spatial tile splits its inputs too."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((batch,) + tuple(spec.in_shape), generator=g) < density).float()
    frac = torch.rand((batch, 1, 1), generator=g)
    x[:, -1] = torch.floor(frac * 64) / 64 if bf16_exact else frac
    return x


@dataclass(frozen=True)
class Case:
    name: str
    kernel: str            # "sp" (csrc/leafnet_sp.h), "c4" (csrc/leafnet_c4.h) or "f32" (csrc/leafnet_f32.hip only)
    kw: tuple              # NetSpec keyword arguments, as sorted items
    refuse: str = None     # MFMA tiers must refuse the shape with this fragment in the message
    tbw: int = 0           # boards per workgroup of the tile the case runs on (0: no tile)

    def spec(self):
        from alphazero import torch_net
        return torch_net.NetSpec(**dict(self.kw))

    def tiers(self):
        return ("fp32",) if self.kernel == "f32" else ("bf16", "bf16x3", "fp32")


SP_TBW = {7: 5, 11: 2, 13: 1}      # csrc/leafnet_sp.h Geo7 / Geo11 / Geo13
C4_TBW = 3                         # csrc/leafnet_c4.h TileSmall (the tile of every batch below 3072 / 769 rows)


def _sp(name, board=7, cin=7, depth=1, ch=64, hc=64, vh=256, vl=2, players=2, pc=4, glob=0, ph=512, vconvs=1, piconvs=1,
        kernel="sp", refuse=None, hw=None):
    h, w = hw or (board, board)
    kw = dict(in_shape=(cin, h, w), num_moves=pc * h * w + glob, num_players=players, num_channels=ch, depth=depth, kernel_size=3,
              head_channels=hc, v_fc_hidden=vh, v_head_convs=vconvs, pi_head_convs=piconvs, v_fc_layers=vl, policy_shape=(pc, h, w),
              pi_fc_hidden=ph)
    return Case(name, kernel, tuple(sorted(kw.items())), refuse, SP_TBW.get(h, 0) if kernel == "sp" else 0)


def _c4(name, cin=4, depth=1, vh=64, players=2, moves=7, ch=64, hc=32, hw=(6, 7), kernel="c4", refuse=None):
    kw = dict(in_shape=(cin,) + tuple(hw), num_moves=moves, num_players=players, num_channels=ch, depth=depth, kernel_size=3,
              head_channels=hc, v_fc_hidden=vh)
    return Case(name, kernel, tuple(sorted(kw.items())), refuse, C4_TBW if kernel == "c4" else 0)


ACCEPTED_SP = [
    # input planes: the two-chunk stem up to 8, the full convolution from 9
    _sp("sp_cin1", cin=1), _sp("sp_cin4", cin=4), _sp("sp_cin8_b11", board=11, cin=8), _sp("sp_cin9", cin=9),
    _sp("sp_cin36_b11", board=11, cin=36), _sp("sp_cin64", cin=64),
    # depth
    _sp("sp_depth1_b13", board=13), _sp("sp_depth3", depth=3), _sp("sp_depth6_b11", board=11, depth=6),
    # value head: hidden width (fc_split flips above 256), FC layers, players
    _sp("sp_vh128", vh=128), _sp("sp_vh384", vh=384), _sp("sp_vh512_vl1", vh=512, vl=1), _sp("sp_vl1", vl=1), _sp("sp_vl3", vl=3),
    _sp("sp_vh384_vl3", vh=384, vl=3),
    _sp("sp_players1", players=1), _sp("sp_players3", players=3), _sp("sp_players15", players=15),
    _sp("sp_players15_vh512_b11", board=11, players=15, vh=512),
    # policy channels
    _sp("sp_pc1", pc=1), _sp("sp_pc17", pc=17), _sp("sp_pc32_b11", board=11, pc=32), _sp("sp_pc32_b7", pc=32),
    # global actions on the three boards, both ends
    _sp("sp_g1_b7", glob=1), _sp("sp_g32_b7", glob=32, pc=32), _sp("sp_g1_b11", board=11, glob=1), _sp("sp_g32_b11", board=11, glob=32, pc=32),
    _sp("sp_g7_b13", board=13, glob=7, cin=9),
    # pi_hidden: both ends; above v_hidden it sets the FC kernels' LDS
    _sp("sp_ph64", glob=5, ph=64), _sp("sp_ph320", glob=5, ph=320), _sp("sp_ph1024_vh128", glob=5, ph=1024, vh=128),
    # narrow trunk / heads, zero-padded to 64
    _sp("sp_narrow48_16", ch=48, hc=16), _sp("sp_narrow16_48_g3", ch=16, hc=48, glob=3, ph=128),
]

ACCEPTED_C4 = [
    _c4("c4_depth1"), _c4("c4_depth3", depth=3), _c4("c4_depth6", depth=6),
    _c4("c4_vh16", vh=16), _c4("c4_vh144", vh=144), _c4("c4_vh256", vh=256),
    _c4("c4_players1", players=1), _c4("c4_players3", players=3),
    _c4("c4_moves1", moves=1), _c4("c4_moves9", moves=9), _c4("c4_moves16", moves=16),
    _c4("c4_players3_moves16_vh256", players=3, moves=16, vh=256),
]

ACCEPTED_F32 = [
    _sp("f32_3x8", hw=(3, 8), kernel="f32", ch=32, hc=32), _sp("f32_5x5", hw=(5, 5), kernel="f32", ch=32, hc=32),
    _sp("f32_9x9", hw=(9, 9), kernel="f32", ch=32, hc=32),
    _sp("f32_ch24", kernel="f32", ch=24, hc=24), _sp("f32_ch100", kernel="f32", ch=100, hc=40, hw=(5, 5)),
    _sp("f32_vconvs0", kernel="f32", ch=32, hc=32, vconvs=0), _sp("f32_vconvs2", kernel="f32", ch=32, hc=32, vconvs=2),
    _sp("f32_piconvs0", kernel="f32", ch=32, hc=32, piconvs=0), _sp("f32_piconvs2", kernel="f32", ch=32, hc=32, piconvs=2),
    _sp("f32_glob_ph100", kernel="f32", ch=32, hc=32, glob=9, ph=100, hw=(5, 5)),
    _sp("f32_players15_vl3_vh40", kernel="f32", ch=32, hc=24, players=15, vl=3, vh=40, hw=(3, 8)),
    # policy channels above the trunk and head widths: the widest activation is the policy block
    _sp("f32_pc32_ch8", kernel="f32", ch=8, hc=8, pc=32, glob=32, ph=100, hw=(5, 5)),
    _c4("f32_flat_5x5", kernel="f32", cin=3, hw=(5, 5), moves=30, ch=32, hc=16, vh=48),
    _c4("f32_flat_3x8_ch100", kernel="f32", cin=5, hw=(3, 8), moves=11, ch=100, hc=12, vh=20, players=3),
]

REFUSED = [
    _sp("no_9x9", hw=(9, 9), refuse="11x11, 7x7 or 13x13"),
    _sp("no_pc33", pc=33, refuse="policy channels <= 32"),
    _sp("no_g33", glob=33, refuse="0..32 global actions"),
    _sp("no_vh192", vh=192, refuse="value head sizes out of range"),
    _sp("no_players16", players=16, refuse="value head sizes out of range"),
    _sp("no_depth7", depth=7, refuse="residual blocks"),
    _sp("no_ph96", glob=3, ph=96, refuse="pi_hidden must be a multiple of 64"),
    _sp("no_cin65", cin=65, refuse="use precision='fp32'"),
    _c4("no_c4_cin5", cin=5, refuse="5 input planes not instantiated"),
    _c4("no_c4_depth7", depth=7, refuse="residual blocks"),
    # 17 logits per board do not fit the Connect4 tile's logits ring ([TBW][4 + 16] floats, one softmax thread per entry)
    _c4("no_c4_moves17", moves=17, refuse="head sizes out of range"),
    _c4("no_c4_players4", players=4, refuse="head sizes out of range"),
    _c4("no_c4_vh24", vh=24, refuse="multiple of 16"),
    _c4("no_c4_5x5", hw=(5, 5), moves=5, refuse="use precision='fp32'"),
]

ACCEPTED = ACCEPTED_SP + ACCEPTED_C4 + ACCEPTED_F32
BY_NAME = {c.name: c for c in ACCEPTED + REFUSED}
assert len(BY_NAME) == len(ACCEPTED) + len(REFUSED), "case names are unique"
# the accepted part may not shrink under the counts the suite was written for: a case that starts to fail is fixed or
# moved to REFUSED together with a tightened azmi_net_create, never dropped
assert len(ACCEPTED_SP) >= 12 and len(ACCEPTED_C4) >= 6 and len(ACCEPTED_F32) >= 10


def accepted_runs():
    """(case name, precision) for every accepted case on every tier that takes it."""
    return [(c.name, t) for c in ACCEPTED for t in c.tiers()]


def refused_runs():
    return [(c.name, t) for c in REFUSED for t in ("bf16", "bf16x3")]


def make_net(case, seed=7):
    from alphazero import torch_net
    return torch_net.random_init(case.spec(), seed=seed)


def case_inputs(case, batch, seed=1):
    return sparse_planes(case.spec(), batch, seed, bf16_exact=case.kernel == "c4")


# ---- extreme logits: output layers scaled until the reference's max |logit| is past fp32 exp overflow (88.7) ------------
EXTREME = {"connect4": ("connect4_spec", 400.0, 2, 64), "tawlbwrdd": ("tawlbwrdd_spec", 400.0, 2, 48)}   # spec, factor, seed, batch


def extreme_net(which):
    """random_init with the last layer of both heads scaled: the policy's pi_fc1 (flat) / pi_bn2 (spatial), the value's v_fc2."""
    from alphazero import torch_net
    spec_fn, factor, seed, batch = EXTREME[which]
    spec = getattr(torch_net, spec_fn)()
    net = torch_net.random_init(spec, seed=seed)
    with torch.no_grad():
        last = net.pi_bn2 if spec.policy_shape is not None else net.pi_fc1
        last.weight.mul_(factor); last.bias.mul_(factor)
        net.v_fc2.weight.mul_(factor); net.v_fc2.bias.mul_(factor)
    x = (torch.rand((batch,) + tuple(spec.in_shape), generator=torch.Generator().manual_seed(seed)) < 0.25).float()
    return net, x


def decided_rows(pi_ref):
    """rows whose reference top-two ratio is >= 2: the argmax there is no coin toss at any of the tiers' precisions"""
    top = torch.topk(pi_ref, 2, dim=1).values if pi_ref.shape[1] > 1 else torch.cat([pi_ref, torch.zeros_like(pi_ref)], 1)
    return top[:, 0] >= 2 * top[:, 1]
