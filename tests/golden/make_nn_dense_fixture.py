"""Generates the DenseNet leaf-net fixtures by importing the REFERENCE's own neural_net.py in a container that has the
reference tree; only the .npz outputs are committed.  Each holds the random-init state_dict (torch.manual_seed(0),
BatchNorm statistics randomised so that folding is exercised), the canonical inputs and the outputs of the reference
NNArch (eval mode, fp32, CPU; probabilities = exp(log_softmax) as NNWrapper.process returns them).

  nn_connect4_dense_4x12_k5.npz          the TrainConfig defaults (dense_net, growth 12, 4 blocks, 5x5, head_channels 32), 64 positions
  nn_connect4_dense_4x12_k5_peaked.npz   the same net with the last layer of both heads x8 (a random-init net is nearly uniform)
  nn_sg_dense_4x16_k3.npz                configs/star_gambit_skirmish.yaml: 36 planes, 13x13, growth 16, 4 blocks, 3x3, spatial head
                                         with 19 global actions, 8 positions

`alphazero` and `zstandard` are stubbed for the import as in make_nn_fixture.py.
Run:  python tests/golden/make_nn_dense_fixture.py [REFERENCE_SRC]
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


def _game_class(name, **statics):
    return type(name, (), {k: staticmethod((lambda v: (lambda: v))(v)) for k, v in statics.items()})


def _randomise_bn(net):
    g = torch.Generator().manual_seed(1)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.0 + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.8 + 0.6)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)


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
    print("wrote", path, os.path.getsize(path), "bytes;", sum(p.numel() for p in net.parameters()), "params;",
          "pi span", float(pi.max() - pi.min()))
    return v, pi


def main():
    c4 = _game_class("C4", CANONICAL_SHAPE=(4, 6, 7), NUM_PLAYERS=2, NUM_MOVES=7)
    x = _positions(lambda i: orc.Game(orc.GAME_CONNECT4), 64, 30, seed=3)
    made = []
    for peaked in (False, True):
        torch.manual_seed(0)
        net = ref_nn.NNArch(c4, ref_nn.NNArgs(num_channels=12, depth=4, kernel_size=5, dense_net=True, head_channels=32))
        _randomise_bn(net)
        if peaked:
            with torch.no_grad():
                net.v_fc2.weight.mul_(8.0)
                net.pi_fc1.weight.mul_(8.0)
        name = "nn_connect4_dense_4x12_k5_peaked.npz" if peaked else "nn_connect4_dense_4x12_k5.npz"
        made.append(("connect4_dense_spec", net, x) + _write(name, net, x))

    sg = _game_class("SG", CANONICAL_SHAPE=(36, 13, 13), NUM_PLAYERS=2, NUM_MOVES=1709, POLICY_SHAPE=(10, 13, 13))
    xs = _positions(lambda i: orc.Game.sg_unified(pinned=i % 4), 8, 50, seed=6)
    torch.manual_seed(0)
    net = ref_nn.NNArch(sg, ref_nn.NNArgs(num_channels=16, depth=4, kernel_size=3, dense_net=True, head_channels=32, spatial_policy="on"))
    _randomise_bn(net)
    made.append(("stargambit_dense_spec", net, xs) + _write("nn_sg_dense_4x16_k3.npz", net, xs))

    # the package's own LeafNet must accept these state_dicts and reproduce the reference
    sys.modules.pop("alphazero")
    sys.path.insert(0, os.path.join(ROOT, "alphazero-pybind11_amd"))
    from alphazero import torch_net
    for spec_fn, net, inp, v, pi in made:
        mine = torch_net.LeafNet(getattr(torch_net, spec_fn)())
        mine.load_state_dict(net.state_dict(), strict=True)
        v2, pi2 = mine.process(inp)
        print(f"LeafNet({spec_fn}) vs reference NNArch: max |dv| =", float((v2 - v).abs().max()), " max |dpi| =", float((pi2 - pi).abs().max()))


if __name__ == "__main__":
    main()
