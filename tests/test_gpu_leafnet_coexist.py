"""Several leaf nets alive in one process (csrc/leafnet_host.h: one record per net, kernel instances and their LDS attributes
shared between the nets of a family): what a net computes must not depend on which other nets exist, were created after it or
were destroyed before it.  Every comparison is bit for bit against the same net's outputs from a run alone.

Smallest accepted shapes, batch 33 (a ragged last tile on every instance): the whole module takes a few seconds.
"""
import dataclasses

import pytest
import torch

from test_gpu_search_batch import az  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH = 33


def _specs():
    from alphazero import torch_net
    sp7 = torch_net.NetSpec(in_shape=(7, 7, 7), num_moves=14 * 49, num_players=2, num_channels=64, depth=1, kernel_size=3, head_channels=64,
                            v_head_convs=1, pi_head_convs=1, v_fc_layers=1, v_fc_hidden=128, policy_shape=(14, 7, 7))
    dsp7 = torch_net.NetSpec(in_shape=(4, 7, 7), num_moves=4 * 49 + 3, num_players=2, num_channels=8, depth=1, kernel_size=3, head_channels=32,
                             v_fc_hidden=64, pi_fc_hidden=64, policy_shape=(4, 7, 7), dense_net=True)
    return {
        # family: (spec, precision)
        "c4": (torch_net.connect4_spec(depth=1), "bf16"),
        "spatial": (sp7, "bf16"),
        "dense": (torch_net.connect4_dense_spec(depth=1, channels=8, kernel_size=3), "bf16"),
        "dense_sp": (dsp7, "bf16"),
        "fp32": (torch_net.connect4_spec(depth=1), "fp32"),
        # the widest nets of two shared instances: the dense tile at in_channels + channels * depth = 100 of 128 (the LDS of a
        # board grows with it), the 7x7 spatial tile with v_hidden 512 (the FC kernels' LDS grows with it)
        "dense_wide": (torch_net.connect4_dense_spec(depth=6, channels=16, kernel_size=3), "bf16"),
        "spatial_wide": (dataclasses.replace(sp7, v_fc_hidden=512), "bf16"),
    }


FAMILIES = ("c4", "spatial", "dense", "dense_sp", "fp32")


def _make(name, seed=5):
    import alphazero
    from alphazero import torch_net
    spec, precision = _specs()[name]
    return alphazero.HipLeafNet(torch_net.random_init(spec, seed=seed), precision=precision)


def _destroy(net):
    net.__del__()      # azmi_net_destroy now, not when the collector gets to it


def _inputs(net):
    d = net.desc
    g = torch.Generator().manual_seed(d.in_channels * 100 + d.height)
    x = torch.randint(0, 2, (BATCH, d.in_channels, d.height, d.width), generator=g).float().to(DEV)
    rows = torch.arange(BATCH - 1, -1, -2, dtype=torch.int32).to(DEV)      # every other slot, last one first: 17 of 33
    count = torch.tensor([rows.numel() - 2], dtype=torch.int32).to(DEV)    # ... of which the list holds 15
    return x, rows, count


def _outputs(net):
    d = net.desc
    return (torch.full((BATCH, d.num_players + 1), -1.0, device=DEV), torch.full((BATCH, d.num_moves), -1.0, device=DEV))


def _run(net, inputs, outs=None, stream=None, rows_stream=None):
    """-> (v, pi of forward, v, pi of forward_rows over slots prefilled with -1), enqueued only.  On streams of the caller's the
    outputs are the caller's too (`outs`), filled before the streams start"""
    x, rows, count = inputs
    v, pi, vr, pir = outs if outs is not None else _outputs(net) + _outputs(net)
    net.forward(x, v, pi, stream=stream)
    net.forward_rows(x, vr, pir, rows, count, stream=rows_stream if rows_stream is not None else stream)
    return v, pi, vr, pir


def _same_bits(got, want):
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want))


@pytest.fixture(scope="module")
def alone():
    """name -> (inputs, the four outputs) of each net created, run and destroyed with no other net of this module alive - shared, not
    to be changed"""
    out = {}
    for name in _specs():
        net = _make(name)
        inputs = _inputs(net)
        res = _run(net, inputs)
        torch.cuda.synchronize()
        v, pi, vr, pir = res
        listed = inputs[1][:int(inputs[2])].long()
        assert torch.isfinite(v).all() and torch.isfinite(pi).all() and (pi >= 0).all()
        assert _same_bits((vr[listed], pir[listed]), (v[listed], pi[listed])), name
        untouched = torch.ones(BATCH, dtype=torch.bool, device=DEV)
        untouched[listed] = False
        assert (vr[untouched] == -1).all() and (pir[untouched] == -1).all(), name
        out[name] = (inputs, res)
        _destroy(net)
    return out


@pytest.mark.parametrize("wide, narrow", [("dense_wide", "dense"), ("spatial_wide", "spatial")])
def test_a_narrow_net_created_later_takes_nothing_from_a_wide_one_of_the_same_instance(alone, wide, narrow):
    w = _make(wide)
    n = _make(narrow)
    inputs, want = alone[wide]
    got = _run(w, inputs)
    torch.cuda.synchronize()
    assert _same_bits(got, want)
    inputs, want = alone[narrow]
    got = _run(n, inputs)
    torch.cuda.synchronize()
    assert _same_bits(got, want)
    _destroy(w)
    _destroy(n)


def test_one_net_of_every_family_interleaved_on_two_streams(alone):
    nets = {name: _make(name) for name in FAMILIES}
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    outs = [[_outputs(nets[name]) + _outputs(nets[name]) for name in FAMILIES] for _ in range(2)]
    torch.cuda.synchronize()
    got = []
    for turn in range(2):
        for i, name in enumerate(FAMILIES):
            a, b = streams[(i + turn) % 2].cuda_stream, streams[(i + turn + 1) % 2].cuda_stream
            got.append((name, _run(nets[name], alone[name][0], outs[turn][i], stream=a, rows_stream=b)))
    torch.cuda.synchronize()
    for name, res in got:
        assert _same_bits(res, alone[name][1]), name
    for net in nets.values():
        _destroy(net)


@pytest.mark.parametrize("order", ["creation", "reverse"])
def test_nets_destroyed_in_either_order_leave_the_next_one_whole(alone, order):
    nets = [_make(name) for name in FAMILIES]
    for net, name in zip(nets, FAMILIES):
        _run(net, alone[name][0])
    torch.cuda.synchronize()
    for net in (nets if order == "creation" else nets[::-1]):
        _destroy(net)
    for name in ("spatial", "c4"):
        again = _make(name)
        got = _run(again, alone[name][0])
        torch.cuda.synchronize()
        assert _same_bits(got, alone[name][1]), name
        _destroy(again)
