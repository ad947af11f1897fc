"""-m gpu: every descriptor azmi_net_create accepts, at both ends of every bound it states, against an fp64 reference.

The table lives in tests/leafnet_ref.py.  An accepted case runs on every tier that takes it - the spatial and
Connect4-family cases on bf16, bf16x3 and fp32, the rest on fp32 - at batches 1, tile width + 1 and 53.  A case may pass
by being refused only if it sits in the REFUSED part of the table and the constructor's RuntimeError carries its
fragment; a RuntimeError from an accepted case fails its test like any other exception.

Bounds, all against the fp64 CPU forward of the same weights (whose distance from torch's fp32 forward is 5e-8):
  fp32, bf16x3   max |dv|, max |dpi| <= 1e-5 (the project's tier), relative error <= 1e-3 on entries >= 1e-6, rows sum to 1
                 within 1e-5
  bf16           err <= max(1e-3, 2 * e16): the project's 1e-3 where it holds, and where torch's own bf16-autocast forward
                 of the same net on the same device is further than that from fp64 (e16), twice ITS error - the margin
                 tests/test_gpu_leafnet.py gives that comparison.  err and e16 are printed per case.
  every tier     finite outputs; on the MFMA tiers a row's bits do not depend on its batch; argmax(pi) equals the
                 reference's on rows whose reference top-two ratio is >= 2
"""
import functools

import pytest
import torch

import leafnet_ref as lr

BATCH = 53


@functools.lru_cache(maxsize=None)
def _case(name):
    case = lr.BY_NAME[name]
    net = lr.make_net(case)
    x = lr.case_inputs(case, BATCH)
    return case, net, x, lr.reference(net, x)


def _errors(v, pi, rv, rpi):
    v, pi = v.double().cpu(), pi.double().cpu()
    dv, dpi = (v - rv).abs().max().item(), (pi - rpi).abs().max().item()
    rel = 0.0
    for got, want in ((v, rv), (pi, rpi)):
        big = want >= 1e-6
        if bool(big.any()):
            rel = max(rel, ((got - want).abs()[big] / want[big]).max().item())
    return dv, dpi, rel


def _check_tier(precision, v, pi, rv, rpi, e16, what):
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(pi).all()), f"{what}: non-finite output"
    dv, dpi, rel = _errors(v, pi, rv, rpi)
    sums = max((v.double().sum(1) - 1).abs().max().item(), (pi.double().sum(1) - 1).abs().max().item())
    if precision == "bf16":
        print("%s: err |dv| %.3e |dpi| %.3e rel %.3e | e16 %.3e" % (what, dv, dpi, rel, e16))
        assert max(dv, dpi) <= max(lr.TOL, 2 * e16), (what, dv, dpi, e16)
        assert sums <= 1e-4, (what, sums)
    else:
        print("%s: err |dv| %.3e |dpi| %.3e rel %.3e" % (what, dv, dpi, rel))
        assert dv <= lr.TOL_F32 and dpi <= lr.TOL_F32, (what, dv, dpi)
        assert rel <= 1e-3, (what, rel)
        assert sums <= 1e-5, (what, sums)
    decided = lr.decided_rows(rpi)
    assert torch.equal(pi.cpu().argmax(1)[decided], rpi.argmax(1)[decided]), f"{what}: argmax differs on a decided row"


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", lr.accepted_runs())
def test_accepted_shape_matches_the_fp64_reference(name, precision):
    import alphazero as az
    case, net, x, (rv, rpi, _) = _case(name)
    hip = az.HipLeafNet(net, precision=precision)       # a refusal here fails the test: the case is in the accepted part
    xd = x.cuda()
    e16 = 0.0
    if precision == "bf16":
        v16, pi16 = net.cuda().process(xd, amp_dtype=torch.bfloat16)
        net.cpu()
        e16 = max((v16.double().cpu() - rv).abs().max().item(), (pi16.double().cpu() - rpi).abs().max().item())
    v, pi = hip.process(xd)
    small = sorted({1, (case.tbw or 3) + 1})
    parts = {n: hip.process(xd[:n].contiguous()) for n in small}
    torch.cuda.synchronize()
    assert v.shape == (BATCH, case.spec().num_players + 1) and pi.shape == (BATCH, case.spec().num_moves)
    _check_tier(precision, v, pi, rv, rpi, e16, f"{name} {precision} batch {BATCH}")
    for n, (vn, pn) in parts.items():
        if precision != "fp32":
            assert torch.equal(vn, v[:n]) and torch.equal(pn, pi[:n]), f"{name} {precision}: rows of a batch of {n} differ from the batch of {BATCH}"
        else:
            _check_tier(precision, vn, pn, rv[:n], rpi[:n], e16, f"{name} {precision} batch {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", lr.refused_runs())
def test_refused_shape_is_refused_by_the_constructor(name, precision):
    """with a device present too, the refusal comes from the constructor, with the message; never from forward, never as another tier"""
    import alphazero as az
    case = lr.BY_NAME[name]
    with pytest.raises(RuntimeError) as e:
        az.HipLeafNet(lr.make_net(case), precision=precision)
    assert case.refuse in str(e.value), (case.refuse, str(e.value))


@pytest.mark.gpu
def test_fp32_policy_block_wider_than_the_trunk_past_the_first_reservation():
    """fp32 path, 32 policy channels over an 8-channel trunk, more rows than the 4096 reserved at creation: the activation
    buffers are sized by the widest layer (the policy block [32][HW]), not by the trunk"""
    import alphazero as az
    case = lr.BY_NAME["f32_pc32_ch8"]
    net = lr.make_net(case)
    x = lr.case_inputs(case, 4200, seed=3)
    rv, rpi, _ = lr.reference(net, x)
    v, pi = az.HipLeafNet(net, precision="fp32").process(x.cuda())
    torch.cuda.synchronize()
    _check_tier("fp32", v, pi, rv, rpi, 0.0, "f32_pc32_ch8 batch 4200")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "fp32"])
@pytest.mark.parametrize("which", sorted(lr.EXTREME))
def test_extreme_logits_stay_finite_and_keep_the_argmax(which, precision):
    """output layers scaled until the fp64 reference's largest |logit| is past 100 (fp32 exp overflows at 88.7): a softmax
    that does not subtract the row maximum, or subtracts it after the exponent, gives inf / NaN here"""
    import alphazero as az
    net, x = lr.extreme_net(which)
    rv, rpi, logits = lr.reference(net, x)
    assert logits.abs().max().item() > 100, logits.abs().max().item()
    decided = lr.decided_rows(rpi)
    assert int(decided.sum()) * 2 >= x.shape[0], "the seed must leave at least half the batch with a top-two ratio >= 2"
    v, pi = az.HipLeafNet(net, precision=precision).process(x.cuda())
    torch.cuda.synchronize()
    v, pi = v.cpu(), pi.cpu()
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(pi).all())
    sv, spi = (v.double().sum(1) - 1).abs().max().item(), (pi.double().sum(1) - 1).abs().max().item()
    print("%s %s: max |logit| %.1f decided rows %d / %d, row sums off by %.2e / %.2e"
          % (which, precision, logits.abs().max().item(), int(decided.sum()), x.shape[0], sv, spi))
    assert sv <= 1e-5 and spi <= 1e-5, (sv, spi)
    assert torch.equal(pi.argmax(1)[decided], rpi.argmax(1)[decided])
