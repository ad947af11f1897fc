"""Shared by the DenseNet leaf-net tests: the reference's own outputs (tests/golden/nn_*dense*.npz, written by
tests/golden/make_nn_dense_fixture.py) and the table of dense net shapes.  (ResNet trunks stay 3x3 on every tier:
tests/test_leafnet_shapes_fold.py holds fold(net, "fp32") to refusing kernel_size 5 there.)

The table: every bound the dense matrix-core tile states (csrc/leafnet_dense.h, azmi_net_create2) at both ends, the shapes
it must refuse with a fragment of the message expected, and shapes only the fp32 path takes.  Nets are one block deep
and narrow unless the case is about something else; the fp64 forward of tests/leafnet_ref.py is the reference for them.
"""
import functools
import os
from dataclasses import dataclass

import numpy as np
import torch

import leafnet_ref as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DENSE_TBW = 4        # csrc/leafnet_dense.h: boards (wavefronts) per workgroup

FIXTURES = {         # name -> (file, torch_net spec function)
    "connect4_dense": ("nn_connect4_dense_4x12_k5.npz", "connect4_dense_spec"),
    "connect4_dense_peaked": ("nn_connect4_dense_4x12_k5_peaked.npz", "connect4_dense_spec"),
    "sg_dense": ("nn_sg_dense_4x16_k3.npz", "stargambit_dense_spec"),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(LeafNet with the fixture's state_dict loaded strictly, inputs, reference v, reference pi) - shared, not to be changed"""
    from alphazero import torch_net
    fname, spec_fn = FIXTURES[name]
    z = np.load(os.path.join(GOLDEN, fname))
    net = torch_net.LeafNet(getattr(torch_net, spec_fn)())
    net.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}, strict=True)
    return net.eval(), torch.from_numpy(z["input"]), torch.from_numpy(z["v"]), torch.from_numpy(z["pi"])


@dataclass(frozen=True)
class Case:
    name: str
    kw: tuple              # NetSpec keyword arguments, as sorted items
    refuse: str = None     # the bf16 tier must refuse the shape with this fragment in the message

    def spec(self):
        from alphazero import torch_net
        return torch_net.NetSpec(**dict(self.kw))


def _dn(name, cin=4, hw=(6, 7), g=8, depth=1, k=5, hc=32, vh=64, players=2, moves=7, pc=0, glob=0, ph=64, vconvs=0, piconvs=0, vl=1,
        dense=True, refuse=None):
    h, w = hw
    kw = dict(in_shape=(cin, h, w), num_moves=pc * h * w + glob if pc else moves, num_players=players, num_channels=g, depth=depth,
              kernel_size=k, head_channels=hc, v_fc_hidden=vh, v_head_convs=vconvs, pi_head_convs=piconvs, v_fc_layers=vl,
              policy_shape=(pc, h, w) if pc else None, pi_fc_hidden=ph, dense_net=dense)
    return Case(name, tuple(sorted(kw.items())), refuse)


ACCEPTED_TILE = [
    _dn("dn_default", g=12, depth=4, vh=256),              # the reference's TrainConfig defaults
    _dn("dn_g1", g=1), _dn("dn_g16", g=16),
    _dn("dn_depth1_k3", k=3), _dn("dn_deepest_128", cin=8, g=15, depth=8), _dn("dn_g16_depth7_k3", g=16, depth=7, k=3),
    _dn("dn_cin1", cin=1), _dn("dn_cin8", cin=8, depth=2),
    _dn("dn_vh16", vh=16), _dn("dn_vh256", vh=256),
    _dn("dn_players1", players=1), _dn("dn_players3", players=3),
    _dn("dn_moves1", moves=1), _dn("dn_moves16", moves=16, players=3, vh=256, k=3),
]

REFUSED_TILE = [
    _dn("no_dn_5x5", hw=(5, 5), moves=5, refuse="6x7 board"),
    _dn("no_dn_g17", g=17, refuse="growth rate (channels) 1..16"),
    _dn("no_dn_129", cin=1, g=16, depth=8, refuse="in_channels + channels * depth <= 128"),
    _dn("no_dn_k7", k=7, refuse="kernel_size 3 or 5"),
    _dn("no_dn_hc64", hc=64, vh=256, refuse="32 head channels"),
    _dn("no_dn_spatial", pc=2, refuse="flat policy head"),
]

ACCEPTED_F32 = (
    # dense trunks on boards no tile has, every kernel size; k = 7 on 3x8: the halo is wider than the board
    [_dn(f"f32_dn_3x8_k{k}", hw=(3, 8), cin=3, k=k, moves=11) for k in (1, 3, 5, 7)] +
    [_dn(f"f32_dn_5x5_k{k}", hw=(5, 5), cin=3, k=k, pc=2) for k in (1, 3, 5, 7)] +
    [_dn("f32_dn_g1", hw=(5, 5), g=1, moves=9), _dn("f32_dn_g24", hw=(5, 5), g=24, moves=9), _dn("f32_dn_g100", hw=(3, 8), g=100, k=3, moves=9),
     _dn("f32_dn_depth6", hw=(5, 5), g=5, depth=6, k=3, moves=9),
     _dn("f32_dn_cin1", hw=(5, 5), cin=1, moves=9), _dn("f32_dn_cin36", hw=(5, 5), cin=36, k=3, pc=3, glob=4, ph=40),
     _dn("f32_dn_spatial", hw=(5, 5), pc=4, hc=16), _dn("f32_dn_spatial_glob", hw=(3, 8), pc=2, glob=7, ph=48, hc=24, vl=2),
     _dn("f32_dn_headconvs2_k5", hw=(5, 5), pc=2, vconvs=2, piconvs=2, hc=16, vl=3),
     _dn("f32_dn_headconvs2_flat", hw=(3, 8), moves=11, vconvs=2, piconvs=2, hc=8, k=5),
     _dn("f32_dn_6x7_k7_hc64", k=7, hc=64, g=17, depth=2)])

BY_NAME = {c.name: c for c in ACCEPTED_TILE + REFUSED_TILE + ACCEPTED_F32}
assert len(BY_NAME) == len(ACCEPTED_TILE) + len(REFUSED_TILE) + len(ACCEPTED_F32), "case names are unique"


def make_net(case, seed=11):
    from alphazero import torch_net
    return torch_net.random_init(case.spec(), seed=seed)


def case_inputs(case, batch, seed=2):
    return lr.sparse_planes(case.spec(), batch, seed, bf16_exact=True)
