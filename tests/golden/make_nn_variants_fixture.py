"""Generates the leaf-net fixtures of the trunk variants (trunk_norm="layer", trunk_act="crelu", pi_fc_layers > 0) by importing
the REFERENCE's own neural_net.py where the reference tree is available; only the .npz outputs are committed.  Each holds
the random-init state_dict (torch.manual_seed(0); BatchNorm statistics, BatchNorm and GroupNorm weights and biases randomised,
so that neither a fold nor an identity affine can hide), 64 canonical inputs and the outputs of the reference NNArch (eval mode,
fp32, CPU; probabilities = exp(log_softmax) as NNWrapper.process returns them).

  nn_connect4_dense_layer.npz         the TrainConfig defaults (dense_net, growth 12, 4 blocks, 5x5) with trunk_norm="layer"
  nn_connect4_dense_layer_crelu.npz   the same with trunk_act="crelu" as well.  CReLU doubles the convolutions' input channels and
                                      the file may not outgrow nn_connect4_dense_4x12_k5.npz, so the convolution weights are rounded
                                      to values bf16 can hold BEFORE the reference runs (they are fp32 tensors whose low mantissa bits
                                      are zero and compress away); the reference computed its outputs from exactly these weights
  nn_connect4_2b32c_layer_crelu_fc2.npz   Connect4 ResNet, 2 blocks x 32 channels, layer + crelu, pi_fc_layers=2 (head_channels 8,
                                      pi_fc_hidden 32); convolution weights rounded in the same way, for the same reason
  nn_brandubh_1b32c_layer.npz         Brandubh (7x7, spatial head 14 x 7 x 7), ResNet 1 block x 32 channels, layer

`alphazero` and `zstandard` are stubbed for the import as in make_nn_fixture.py.
Run:  python tests/golden/make_nn_variants_fixture.py [REFERENCE_SRC]
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = next((a for a in sys.argv[1:] if not a.startswith("--")), "/root/reference/src")

stub = types.ModuleType("alphazero")
stub.tracy_is_enabled = lambda: False
stub._tracy_zone_begin = lambda *a: None
stub._tracy_zone_end = lambda: None
stub.tracy_frame_mark = lambda: None
stub._tracy_set_thread_name = lambda n: None
sys.modules["alphazero"] = stub
sys.modules["zstandard"] = types.ModuleType("zstandard")
sys.path.insert(0, REF)
import neural_net as ref_nn  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_api as orc  # noqa: E402  (only to produce realistic canonical inputs)

LIMIT = os.path.getsize(os.path.join(HERE, "nn_connect4_dense_4x12_k5.npz"))


def _game_class(name, **statics):
    return type(name, (), {k: staticmethod((lambda v: (lambda: v))(v)) for k, v in statics.items()})


def _randomise_norms(net):
    g = torch.Generator().manual_seed(1)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.0 + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.8 + 0.6)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
        elif isinstance(m, torch.nn.GroupNorm):
            m.weight.data.copy_(torch.rand(m.num_channels, generator=g) * 0.8 + 0.6)
            m.bias.data.copy_(torch.randn(m.num_channels, generator=g) * 0.1)


def _positions(make_game, count, max_plies, seed):
    rng = np.random.default_rng(seed)
    xs = []
    while len(xs) < count:
        game = make_game(len(xs))
        for _ in range(int(rng.integers(0, max_plies))):
            if game.scores() is not None:
                break
            game.play(int(rng.choice(np.flatnonzero(game.valid()))))
        xs.append(game.canonical())
    return torch.from_numpy(np.stack(xs))


def _write(name, net, x):
    net.eval()
    with torch.no_grad():
        v, pi = net(x)
        v, pi = torch.exp(v), torch.exp(pi)
    out = {"input": x.numpy(), "v": v.numpy(), "pi": pi.numpy()}
    for k, t in net.state_dict().items():
        out["sd." + k] = t.numpy()
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes;", sum(p.numel() for p in net.parameters()), "params;", "pi span", float(pi.max() - pi.min()))
    assert size <= LIMIT, (size, LIMIT)
    return v, pi


def main():
    c4 = _game_class("C4", CANONICAL_SHAPE=(4, 6, 7), NUM_PLAYERS=2, NUM_MOVES=7)
    bd = _game_class("Brandubh", CANONICAL_SHAPE=(7, 7, 7), NUM_PLAYERS=2, NUM_MOVES=686, POLICY_SHAPE=(14, 7, 7))
    x4 = _positions(lambda i: orc.Game(orc.GAME_CONNECT4), 64, 30, seed=3)
    xb = _positions(lambda i: orc.Game(orc.GAME_BRANDUBH), 64, 50, seed=6)
    cases = [
        ("nn_connect4_dense_layer.npz", c4, x4, False,
         dict(num_channels=12, depth=4, kernel_size=5, dense_net=True, head_channels=32, trunk_norm="layer")),
        ("nn_connect4_dense_layer_crelu.npz", c4, x4, True,
         dict(num_channels=12, depth=4, kernel_size=5, dense_net=True, head_channels=32, trunk_norm="layer", trunk_act="crelu")),
        ("nn_connect4_2b32c_layer_crelu_fc2.npz", c4, x4, True,
         dict(num_channels=32, depth=2, kernel_size=3, dense_net=False, head_channels=8, trunk_norm="layer", trunk_act="crelu",
              pi_fc_layers=2, pi_fc_hidden=32)),
        ("nn_brandubh_1b32c_layer.npz", bd, xb, False,
         dict(num_channels=32, depth=1, kernel_size=3, dense_net=False, head_channels=32, trunk_norm="layer", spatial_policy="on")),
    ]
    made = []
    for name, game, x, round_convs, kw in cases:
        torch.manual_seed(0)
        net = ref_nn.NNArch(game, ref_nn.NNArgs(**kw))
        _randomise_norms(net)
        with torch.no_grad():
            if round_convs:
                for m in net.modules():
                    if isinstance(m, torch.nn.Conv2d):
                        m.weight.copy_(m.weight.to(torch.bfloat16).float())
            net.v_fc2.weight.mul_(4.0)      # a random-init net is nearly uniform: spread the outputs a little
            last = net.pi_fc_out if hasattr(net, "pi_fc_out") else net.pi_fc1 if hasattr(net, "pi_fc1") else net.pi_bn2
            last.weight.mul_(4.0)
        made.append((name, kw, net, x) + _write(name, net, x))

    # the package's own LeafNet must accept these state_dicts and reproduce the reference
    sys.modules.pop("alphazero")
    sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
    import leafnet_variants_ref as vr
    for name, kw, net, inp, v, pi in made:
        mine, _, _, _ = vr.fixture(next(k for k, f in vr.FIXTURES.items() if f[0] == name))
        v2, pi2 = mine.process(inp)
        print(f"LeafNet({name}) vs reference NNArch: max |dv| =", float((v2 - v).abs().max()), " max |dpi| =", float((pi2 - pi).abs().max()))


if __name__ == "__main__":
    main()
