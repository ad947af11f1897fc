"""CPU: hip_net.refresh_names, the ordered table HipLeafNet.refresh hands to azmi_net_refresh.  For the two families refresh is built
for it lists every tensor fold() / fold_dense() reads, each once (found by moving each tensor of the state_dict and folding
again); every family outside the scope raises RuntimeError naming itself and the way out (a new HipLeafNet)."""
import dataclasses

import pytest


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    from alphazero import hip_net, torch_net
    return hip_net, torch_net


def _tensors_fold_reads(hip_net, torch_net, spec, precision):
    """the state_dict keys whose values the folded image depends on: each is moved in turn and the fold repeated"""
    import torch
    net = torch_net.random_init(spec, seed=1)
    base = hip_net.fold(net, precision)[1]
    read = set()
    for key, t in net.state_dict().items():
        keep = t.clone()
        with torch.no_grad():
            t.add_(1 if not t.dtype.is_floating_point else 0.5)
        if hip_net.fold(net, precision)[1] != base:
            read.add(key)
        with torch.no_grad():
            t.copy_(keep)
    assert hip_net.fold(net, precision)[1] == base
    return read, set(net.state_dict().keys())


def _cases(torch_net):
    """small nets of both families (the fold is repeated once per tensor): the names do not depend on the widths"""
    c4 = torch_net.connect4_spec
    return [(dataclasses.replace(c4(depth=1), v_fc_hidden=16), "bf16"), (dataclasses.replace(c4(depth=1), v_fc_hidden=16), "bf16x3"),
            (dataclasses.replace(torch_net.connect4_dense_spec(depth=2, channels=4, kernel_size=3), v_fc_hidden=16), "bf16")]


def test_refresh_names_lists_every_tensor_fold_reads_once(mods):
    hip_net, torch_net = mods
    for spec, precision in _cases(torch_net):
        names = hip_net.refresh_names(spec, precision)
        assert len(names) == len(set(names)), "a tensor is listed twice"
        read, every = _tensors_fold_reads(hip_net, torch_net, spec, precision)
        assert set(names) == read, (sorted(read - set(names)), sorted(set(names) - read))
        # and that is the whole state_dict but the BatchNorms' step counters
        assert set(names) == {k for k in every if not k.endswith("num_batches_tracked")}
    for spec, precision in ((torch_net.connect4_spec(), "bf16"), (torch_net.connect4_spec(), "bf16x3"), (torch_net.connect4_dense_spec(), "bf16")):
        names = hip_net.refresh_names(spec, precision)      # the full-size nets: the same rule, depth times
        every = torch_net.LeafNet(spec).state_dict().keys()
        assert len(names) == len(set(names)) and set(names) == {k for k in every if not k.endswith("num_batches_tracked")}


def test_refresh_names_order_is_the_table_order_of_the_family(mods):
    hip_net, torch_net = mods
    names = hip_net.refresh_names(torch_net.connect4_spec(depth=1), "bf16")
    bn = ["weight", "bias", "running_mean", "running_var"]
    assert names == (["conv1.weight"] + [f"bn1.{t}" for t in bn]
                     + [f"conv_layers.0.bn1.{t}" for t in bn] + ["conv_layers.0.conv1.weight"]
                     + [f"conv_layers.0.bn2.{t}" for t in bn] + ["conv_layers.0.conv2.weight"]
                     + ["v_conv.weight"] + [f"v_bn.{t}" for t in bn] + ["pi_conv.weight"] + [f"pi_bn.{t}" for t in bn]
                     + ["v_fc1.weight", "v_fc1.bias", "v_fc2.weight", "v_fc2.bias", "pi_fc1.weight", "pi_fc1.bias"])
    dense = hip_net.refresh_names(torch_net.connect4_dense_spec(), "bf16")
    assert dense[0] == "conv_layers.0.bn1.weight" and "conv1.weight" not in dense and len(dense) == 4 * 10 + 16
    assert hip_net.refresh_names(torch_net.connect4_spec(), "bf16x3") == hip_net.refresh_names(torch_net.connect4_spec(), "bf16")


def test_families_outside_the_scope_raise_naming_themselves(mods):
    hip_net, torch_net = mods
    dense = torch_net.connect4_dense_spec()
    outside = [
        (torch_net.tawlbwrdd_spec(), "bf16", "spatial-head tile"),
        (torch_net.brandubh_spec(), "bf16x3", "spatial-head tile"),
        (torch_net.stargambit_spec(), "bf16", "spatial-head tile"),
        (torch_net.stargambit_variant_dense_spec(0), "bf16", "dense spatial-head tile"),
        (torch_net.stargambit_dense_spec(), "bf16", "dense spatial-head tile"),
        (dataclasses.replace(dense, trunk_norm="layer"), "bf16", "layer-norm instance"),
        (torch_net.connect4_spec(), "fp32", "fp32 tier"),
        (dense, "fp32", "fp32 tier"),
        (dataclasses.replace(torch_net.connect4_spec(), trunk_act="crelu"), "bf16", "crelu"),
    ]
    for spec, precision, family in outside:
        with pytest.raises(RuntimeError, match="new HipLeafNet") as e:
            hip_net.refresh_names(spec, precision)
        assert family in str(e.value), (family, str(e.value))
    with pytest.raises(ValueError, match="precision"):
        hip_net.refresh_names(dense, "fp16")
