"""Shared by the tests of the dense spatial-head tile (csrc/leafnet_dense_sp.h, hip_net.fold_dense_spatial): the table of shapes
at both ends of every bound `refusal` states (csrc/leafnet_dense_sp_host.hip), the shapes it must refuse with a fragment of the
message expected, and the nets with scaled output layers.

Nets are one block deep with growth 8 on the 7x7 board unless the case is about something else; the fp64 forward of
tests/leafnet_ref.py is the reference for them, the reference NNArch's own outputs (tests/golden/nn_sg_dense_4x16_k3.npz through
leafnet_dense_ref.fixture("sg_dense")) for the fixture.
"""
import copy

import torch

import leafnet_ref as lr
from leafnet_dense_ref import Case

DSP_TBW = {7: 1, 11: 1, 13: 1}        # csrc/leafnet_dense_sp.h: boards per workgroup of Geo7 / Geo11 / Geo13


def _sp(name, board=7, cin=4, g=8, depth=1, k=3, hc=32, vh=64, players=2, pc=4, glob=3, ph=64, vconvs=0, piconvs=0, vl=1, refuse=None):
    kw = dict(in_shape=(cin, board, board), num_moves=pc * board * board + glob, num_players=players, num_channels=g, depth=depth,
              kernel_size=k, head_channels=hc, v_fc_hidden=vh, v_head_convs=vconvs, pi_head_convs=piconvs, v_fc_layers=vl,
              policy_shape=(pc, board, board), pi_fc_hidden=ph, dense_net=True)
    return Case(name, tuple(sorted(kw.items())), refuse)


ACCEPTED = [
    _sp("dsp_b7"), _sp("dsp_b11", board=11), _sp("dsp_b13", board=13),
    _sp("dsp_k5_b7", k=5), _sp("dsp_k5_b11", board=11, k=5),
    _sp("dsp_g1", g=1), _sp("dsp_g16_b7", g=16), _sp("dsp_g16_b11", board=11, g=16), _sp("dsp_g16_b13", board=13, g=16),
    _sp("dsp_128_b13_k5", board=13, cin=32, g=16, depth=6, k=5),          # the LDS corner: 128 features, the widest halo
    _sp("dsp_cin1", cin=1), _sp("dsp_cin36_b13", board=13, cin=36),
    _sp("dsp_pc1", pc=1), _sp("dsp_pc32_b13", board=13, pc=32, glob=32),   # (the most logits a board can have: 5440)
    _sp("dsp_glob0", glob=0), _sp("dsp_glob1", glob=1), _sp("dsp_glob32_pc32_b7", glob=32, pc=32),
    _sp("dsp_ph16", ph=16), _sp("dsp_ph256", ph=256),
    _sp("dsp_vh16", vh=16), _sp("dsp_vh256", vh=256),
    _sp("dsp_players1", players=1), _sp("dsp_players3", players=3),
]

REFUSED = [
    _sp("no_dsp_9x9", board=9, refuse="7x7, 11x11 and 13x13"),
    _sp("no_dsp_g17", g=17, refuse="growth rate (channels) 1..16"),
    _sp("no_dsp_129", cin=1, g=16, depth=8, refuse="in_channels + channels * depth <= 128"),
    _sp("no_dsp_k7", k=7, refuse="kernel_size 3 or 5"),
    _sp("no_dsp_hc64", hc=64, vh=256, refuse="32 head channels"),
    _sp("no_dsp_headconv", vconvs=1, refuse="no extra head convolutions"),
    _sp("no_dsp_vl2", vl=2, refuse="one value FC layer"),
    _sp("no_dsp_pc33", pc=33, refuse="policy channels 1..32"),
    _sp("no_dsp_ph24", ph=24, refuse="pi_hidden must be a multiple of 16"),
]

BY_NAME = {c.name: c for c in ACCEPTED + REFUSED}
assert len(BY_NAME) == len(ACCEPTED) + len(REFUSED), "case names are unique"


def make_net(case, seed=11):
    from alphazero import torch_net
    return torch_net.random_init(case.spec(), seed=seed)


def case_inputs(case, batch, seed=2, bf16_exact=True):
    return lr.sparse_planes(case.spec(), batch, seed, bf16_exact=bf16_exact)


def peaked(net, factor):
    """a deep copy of `net` (which is left as it is) with the last layer of each output scaled: pi_bn2, the LayerNorm behind
    pi_global, v_fc2"""
    out = copy.deepcopy(net)
    with torch.no_grad():
        layers = [out.pi_bn2, out.v_fc2] + ([out.pi_global[3]] if out.num_global_actions > 0 else [])
        for m in layers:
            m.weight.mul_(factor)
            m.bias.mul_(factor)
    return out.eval()
