"""Shared by the tests of the trunk variants (trunk_norm="layer", trunk_act="crelu", pi_fc_layers > 0): the reference's own
outputs (tests/golden/nn_*layer*.npz, written by tests/golden/make_nn_variants_fixture.py), an fp64 forward that does not
care which layer yields the logits (leafnet_ref.reference asserts on pi_fc1 being them, which the FC stack breaks), and the
table of shapes the fp32 tier is held to.

The table's nets are one block deep on a 5x5 board unless the case is about something else: the cases are about which
statistics a norm spans, the doubled input channels, offsets into the weight image and the heads behind them.
"""
import copy
import functools
import os
from dataclasses import dataclass

import numpy as np
import torch

import leafnet_ref as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

C4 = dict(in_shape=(4, 6, 7), num_moves=7, num_players=2)
FIXTURES = {         # name -> (file, NetSpec keyword arguments)
    "c4_dense_layer": ("nn_connect4_dense_layer.npz",
                       dict(C4, num_channels=12, depth=4, kernel_size=5, dense_net=True, trunk_norm="layer")),
    "c4_dense_layer_crelu": ("nn_connect4_dense_layer_crelu.npz",
                             dict(C4, num_channels=12, depth=4, kernel_size=5, dense_net=True, trunk_norm="layer", trunk_act="crelu")),
    "c4_res_layer_crelu_fc2": ("nn_connect4_2b32c_layer_crelu_fc2.npz",
                               dict(C4, num_channels=32, depth=2, head_channels=8, trunk_norm="layer", trunk_act="crelu", pi_fc_layers=2,
                                    pi_fc_hidden=32)),
    "brandubh_res_layer": ("nn_brandubh_1b32c_layer.npz",
                           dict(in_shape=(7, 7, 7), num_moves=686, num_players=2, num_channels=32, depth=1, policy_shape=(14, 7, 7),
                                trunk_norm="layer")),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(LeafNet with the fixture's state_dict loaded strictly, inputs, reference v, reference pi) - shared, not to be changed"""
    from alphazero import torch_net
    fname, kw = FIXTURES[name]
    z = np.load(os.path.join(GOLDEN, fname))
    net = torch_net.LeafNet(torch_net.NetSpec(**kw))
    net.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}, strict=True)
    return net.eval(), torch.from_numpy(z["input"]), torch.from_numpy(z["v"]), torch.from_numpy(z["pi"])


@torch.no_grad()
def reference(net, x):
    """fp64 CPU forward of a deep copy of `net`: (v, pi) = exp(log_softmax) as float64 tensors"""
    ref = copy.deepcopy(net).cpu().double().eval()
    lv, lpi = ref(x.detach().cpu().double())
    return torch.exp(lv), torch.exp(lpi)


@dataclass(frozen=True)
class Case:
    name: str
    kw: tuple              # NetSpec keyword arguments, as sorted items

    def spec(self):
        from alphazero import torch_net
        return torch_net.NetSpec(**dict(self.kw))


def _v(name, norm="batch", act="relu", dense=False, hw=(5, 5), cin=3, ch=8, depth=1, k=3, hc=8, vh=24, moves=9, pc=0, glob=0, fc=0, ph=20):
    h, w = hw
    kw = dict(in_shape=(cin, h, w), num_moves=pc * h * w + glob if pc else moves, num_players=2, num_channels=ch, depth=depth, kernel_size=k,
              head_channels=hc, v_fc_hidden=vh, policy_shape=(pc, h, w) if pc else None, pi_fc_hidden=ph, dense_net=dense, trunk_norm=norm,
              trunk_act=act, pi_fc_layers=fc)
    return Case(name, tuple(sorted(kw.items())))


MODES = [("layer", "relu"), ("batch", "crelu"), ("layer", "crelu")]
SHAPES = (
    # every norm x activation the first descriptor cannot say, on both trunks
    [_v(f"{'dn' if dense else 'res'}_{n}_{a}", n, a, dense) for dense in (False, True) for n, a in MODES] +
    # one case per policy head: the FC stack one and two layers deep (and behind an untouched batch / relu trunk), the spatial
    # head on 7x7, the spatial head with global actions
    [_v("dn_layer_fc1", "layer", dense=True, fc=1), _v("res_crelu_fc2", act="crelu", fc=2), _v("res_plain_fc3", fc=3, depth=2),
     _v("dn_layer_crelu_spatial7", "layer", "crelu", dense=True, hw=(7, 7), pc=3),
     _v("res_layer_spatial_glob", "layer", hw=(5, 5), pc=2, glob=5, ph=16),
     # dense widths off every tile size: C_i = 3, 6, 9 / 3, 16, 29 (no multiple of 32), 4G = 12 / 52 (no multiple of 16); two and
     # three blocks, so that bn1 of a later block spans the planes and the appended channels but not the row's tail
     _v("dn_layer_g3", "layer", dense=True, ch=3, depth=3), _v("dn_layer_crelu_g13", "layer", "crelu", dense=True, ch=13, depth=2),
     # depth 0: the stem's norm alone, straight into the heads
     _v("res_layer_depth0", "layer", depth=0), _v("res_layer_crelu_depth2", "layer", "crelu", depth=2),
     # dense kernel sizes
     _v("dn_layer_crelu_k1", "layer", "crelu", dense=True, k=1), _v("dn_layer_crelu_k7", "layer", "crelu", dense=True, k=7),
     _v("dn_crelu_k5_depth2", act="crelu", dense=True, k=5, depth=2)])


def _tile_layer_cases():
    """the dense tile's layer-norm instance at both ends of every bound dense_refusal states (the batch instance's own cases of
    tests/leafnet_dense_ref.py with trunk_norm="layer"): G 1 and 16, 128 features, v_hidden 16 and 256, 3x3 and 5x5"""
    import leafnet_dense_ref as dr
    names = ("dn_default", "dn_g1", "dn_g16", "dn_depth1_k3", "dn_deepest_128", "dn_g16_depth7_k3", "dn_vh16", "dn_vh256", "dn_moves16")
    return [Case(n + "_layer", tuple(sorted(dict(dr.BY_NAME[n].kw, trunk_norm="layer").items()))) for n in names]


TILE_LAYER = _tile_layer_cases()
BY_NAME = {c.name: c for c in SHAPES + TILE_LAYER}
assert len(BY_NAME) == len(SHAPES) + len(TILE_LAYER), "case names are unique"


def make_net(case, seed=13):
    from alphazero import torch_net
    return torch_net.random_init(case.spec(), seed=seed)


def case_inputs(case, batch, seed=3, bf16_exact=False):
    return lr.sparse_planes(case.spec(), batch, seed, bf16_exact=bf16_exact)
