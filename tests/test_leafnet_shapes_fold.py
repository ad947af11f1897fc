"""No device needed: the host half of the leaf-net shape table (tests/leafnet_ref.py).

fold() must produce exactly the image azmi_net_create expects for every accepted descriptor on every tier, keep the
zero-padded channels of a narrow net exactly zero (the kernels rely on them staying 0 through every affine / ReLU /
conv), and refuse what it refuses with a RuntimeError that says why - azmi_net_create validates the descriptor before
it looks for a device, so the refusals of the C side are checked here as well.
"""
import ctypes as C

import numpy as np
import pytest

import leafnet_ref as lr


def test_the_table_keeps_its_size():
    assert len(lr.ACCEPTED_SP) >= 12 and len(lr.ACCEPTED_C4) >= 6 and len(lr.ACCEPTED_F32) >= 10
    assert all(c.refuse for c in lr.REFUSED) and not any(c.refuse for c in lr.ACCEPTED)


@pytest.mark.parametrize("name,precision", lr.accepted_runs())
def test_fold_gives_the_blob_the_library_expects(name, precision):
    from alphazero import hip_net
    case = lr.BY_NAME[name]
    desc, blob = hip_net.fold(lr.make_net(case), precision)
    assert len(blob) == hip_net.lib.azmi_net_blob_bytes(C.byref(desc))
    spec = case.spec()
    assert (desc.in_channels, desc.height, desc.width) == tuple(spec.in_shape)
    assert (desc.num_moves, desc.num_players, desc.depth, desc.v_hidden) == (spec.num_moves, spec.num_players, spec.depth, spec.v_fc_hidden)
    assert desc.precision == {"bf16": 0, "fp32": 1, "bf16x3": 2}[precision]


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["sp_narrow48_16", "sp_narrow16_48_g3"])
def test_narrow_nets_fold_to_exact_zeros_in_the_padded_channels(name, precision):
    """fp32 parameter block of a spatial image (csrc/leafnet_sp.h SpPtrs::prm): stem_b[64] | per block a1 b1 c1 [3][64] |
    head_b[128] (value, policy) | vx_b[64] | px_b[64] | pol_b[32]"""
    from alphazero import hip_net
    case = lr.BY_NAME[name]
    spec = case.spec()
    desc, blob = hip_net.fold(lr.make_net(case), precision)
    chunks = (3 if precision == "bf16x3" else 1) * ((2 if spec.in_shape[0] <= 8 else 9) + 18 * spec.depth + 2 + 18 + 1)
    nprm = 64 + spec.depth * 3 * 64 + 128 + 64 + 64 + 32
    prm = np.frombuffer(blob, np.float32, count=nprm, offset=chunks * 8192)
    ch, hc, pc = spec.num_channels, spec.head_channels, spec.policy_shape[0]
    trunk = prm[:64 + spec.depth * 3 * 64].reshape(-1, 64)
    heads = prm[64 + spec.depth * 3 * 64:nprm - 32].reshape(-1, 64)          # value, policy, value extra, policy extra
    assert trunk.shape[0] == 1 + 3 * spec.depth and heads.shape[0] == 4
    assert np.all(trunk[:, ch:] == 0) and np.all(trunk[:, :ch].any(axis=1)), "padded trunk channels: scale and bias exactly 0"
    assert np.all(heads[:, hc:] == 0) and np.all(heads[:, :hc].any(axis=1))
    assert np.all(prm[nprm - 32 + pc:] == 0) and prm[nprm - 32:nprm - 32 + pc].any()
    # and the weights: every fragment element whose output or input channel is padding is zero, so the image holds no more
    # non-zero bf16 values than the net has convolution weights (x3: high parts twice, low parts once)
    w16 = np.frombuffer(blob, np.int16, count=chunks * 4096)
    cin = spec.in_shape[0]
    real = 9 * cin * ch + spec.depth * 2 * 9 * ch * ch + 2 * ch * hc + 2 * 9 * hc * hc + hc * pc
    assert np.count_nonzero(w16) <= (3 if precision == "bf16x3" else 1) * real


@pytest.mark.parametrize("name,precision", lr.refused_runs())
def test_refused_shapes_raise_runtime_error_with_the_reason(name, precision):
    """Python-side refusals are RuntimeErrors (never an AssertionError or a KeyError from half-way through the fold); what the
    fold accepts and the library refuses is refused by azmi_net_create's validation, which runs before any device call"""
    import alphazero as az
    case = lr.BY_NAME[name]
    with pytest.raises(RuntimeError) as e:
        az.HipLeafNet(lr.make_net(case), precision=precision)
    assert case.refuse in str(e.value), (case.refuse, str(e.value))


def test_fp32_fold_refuses_what_it_cannot_lay_out():
    from alphazero import hip_net, torch_net
    for kw in (dict(kernel_size=5), dict(head_pool=False)):
        spec = torch_net.NetSpec(in_shape=(3, 5, 5), num_moves=25, num_players=2, num_channels=16, depth=1, head_channels=8, **kw)
        with pytest.raises(RuntimeError):
            hip_net.fold(torch_net.random_init(spec, seed=1), "fp32")
