"""-m gpu: azmi_net_forward_rows, the entry point the engine and the device search evaluate their leaves through.

It evaluates the slots named in a device-side list of device-side length and must touch no other slot: other slots hold
another model group's answers or cache hits that were already delivered.  Four implementations sit behind it - the
Connect4 tiles and k_leafnet_sp read and write through the list themselves, the heads' FC kernels (k_heads_fc, or
k_heads_fc_a + _b for big FC stacks) clip to the count, the fp32 path stages through k_gather_rows / k_scatter_rows -
and every one is run here on its own, at the list lengths around each tile width and FC group.

What a listed slot must hold: on the MFMA tiers the bits of `process()` of the same rows as a dense batch (a row's bits
do not depend on its batch: tests/test_gpu_leafnet.py); on fp32 the fp64 reference within the project's 1e-5.
Every index in `rows`, behind the count too, is a valid slot: a kernel that follows a stale entry shows as an overwritten
sentinel, never as a memory fault.
"""
import functools

import pytest
import torch

import leafnet_ref as lr

pytestmark = pytest.mark.gpu
SENTINEL = -7.25          # no probability
S = 300                   # slots

# kernel behind the entry point -> (spec function, boards per workgroup of the tile that S slots run on)
NETS = {"connect4": ("connect4_spec", 3), "tawlbwrdd": ("tawlbwrdd_spec", 2), "brandubh": ("brandubh_spec", 5), "stargambit": ("stargambit_spec", 1)}
KERNELS = [("connect4", "bf16"), ("connect4", "bf16x3"), ("connect4", "fp32"),
           ("tawlbwrdd", "bf16"), ("tawlbwrdd", "bf16x3"), ("tawlbwrdd", "fp32"),      # v_hidden 512: k_heads_fc_a / _b
           ("brandubh", "bf16"),                                                       # v_hidden 256, no global head: k_heads_fc
           ("stargambit", "bf16"), ("stargambit", "fp32")]                             # the global head


def _counts(tbw):
    return sorted({0, 1, tbw - 1, tbw, tbw + 1, 15, 16, 17, 211, S} - {-1})


@functools.lru_cache(maxsize=None)
def _setup(game, precision):
    import alphazero as az
    from alphazero import torch_net
    spec = getattr(torch_net, NETS[game][0])()
    net = torch_net.random_init(spec, seed=17)
    hip = az.HipLeafNet(net, precision=precision)
    x = lr.sparse_planes(spec, S, seed=len(game))
    ref = lr.reference(net, x)[:2] if precision == "fp32" else None
    return spec, hip, x.cuda(), ref


def _lists(count, seed, slots=S, length=None):
    """A random subset of `count` slots in random order, then the unlisted slots (valid, stale entries), as a device tensor
    of `length` (default: `slots`) entries - past `slots` entries the unlisted slots repeat."""
    perm = torch.randperm(slots, generator=torch.Generator().manual_seed(seed))
    if length is not None and length > slots:
        stale = perm[count:] if count < slots else perm
        perm = torch.cat([perm, stale[torch.arange(length - slots) % stale.numel()]])
    return perm[:count], perm.to(torch.int32).cuda()


def _buffers(spec, slots=S):
    v = torch.full((slots, spec.num_players + 1), SENTINEL, device="cuda")
    pi = torch.full((slots, spec.num_moves), SENTINEL, device="cuda")
    return v, pi


def _untouched(v, pi, listed, what):
    keep = torch.ones(v.shape[0], dtype=torch.bool)
    keep[listed] = False
    keep = keep.cuda()
    assert bool((v[keep] == SENTINEL).all()) and bool((pi[keep] == SENTINEL).all()), f"{what}: an unlisted slot was written"


def _check_listed(hip, precision, x, ref, v, pi, listed, what):
    """assertion 1: bits of the dense call (every tier: the fp32 kernels compute a row from that row alone too); fp32 also
    within 1e-5 of the fp64 reference"""
    if listed.numel() == 0:
        return
    idx = listed.cuda()
    dv, dpi = hip.process(x[idx].contiguous())
    assert torch.equal(v[idx], dv) and torch.equal(pi[idx], dpi), f"{what}: a listed slot differs from the dense batch"
    if precision == "fp32":
        ev = (v[idx].double().cpu() - ref[0][listed]).abs().max().item()
        epi = (pi[idx].double().cpu() - ref[1][listed]).abs().max().item()
        assert ev <= lr.TOL_F32 and epi <= lr.TOL_F32, (what, ev, epi)


@pytest.mark.parametrize("game,precision", KERNELS)
def test_listed_rows_right_everything_else_untouched(game, precision):
    """assertions 1, 2 and 7 at every list length around the tile width, the 16-board FC group, a few hundred, and all"""
    spec, hip, x, ref = _setup(game, precision)
    for count in _counts(NETS[game][1]):
        listed, rows = _lists(count, seed=count)
        cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
        v, pi = _buffers(spec)
        hip.forward_rows(x, v, pi, rows, cnt)
        torch.cuda.synchronize()
        what = f"{game} {precision} count {count}"
        _untouched(v, pi, listed, what)
        _check_listed(hip, precision, x, ref, v, pi, listed, what)
        if count == 0:
            assert bool((v == SENTINEL).all()) and bool((pi == SENTINEL).all())


@pytest.mark.parametrize("game,precision", KERNELS)
def test_unlisted_inputs_are_never_read(game, precision):
    """assertion 3: NaN planes in every unlisted slot (padded tile slots, stale list entries, the fp32 gather's zero fill)
    change no bit of a listed slot and reach no output"""
    spec, hip, x, ref = _setup(game, precision)
    tbw = NETS[game][1]
    for count in (1, tbw + 1, 17, 211):
        listed, rows = _lists(count, seed=100 + count)
        cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
        v0, pi0 = _buffers(spec)
        hip.forward_rows(x, v0, pi0, rows, cnt)
        xn = torch.full_like(x, float("nan"))
        xn[listed.cuda()] = x[listed.cuda()]
        v, pi = _buffers(spec)
        hip.forward_rows(xn, v, pi, rows, cnt)
        torch.cuda.synchronize()
        what = f"{game} {precision} count {count}"
        assert torch.equal(v, v0) and torch.equal(pi, pi0), f"{what}: an unlisted slot's planes changed the outputs"
        _untouched(v, pi, listed, what)
        _check_listed(hip, precision, x, ref, v, pi, listed, what)


@pytest.mark.parametrize("precision,max_rows", [("bf16", 4096), ("bf16x3", 1024)])
def test_tile_choice_from_max_rows_does_not_change_bits(precision, max_rows):
    """assertion 4: the tile comes from max_rows (Connect4: 6 boards from 3072 rows on, bf16x3 above 768), so a 4096-slot
    engine with 40 live rows runs the big tile - and must give the bits of the small dense call (T3 replays, the cache)"""
    spec, hip, x, _ = _setup("connect4", precision)
    listed, rows = _lists(40, seed=5, length=max_rows)
    cnt = torch.tensor([40], dtype=torch.int32, device="cuda")
    v, pi = _buffers(spec)
    hip.forward_rows(x, v, pi, rows, cnt, max_rows=max_rows)
    vs, ps = _buffers(spec)
    hip.forward_rows(x, vs, ps, rows, cnt, max_rows=S)          # the small tile through the same list
    torch.cuda.synchronize()
    _untouched(v, pi, listed, precision)
    _check_listed(hip, precision, x, None, v, pi, listed, f"{precision} max_rows {max_rows}")
    assert torch.equal(v, vs) and torch.equal(pi, ps)


@pytest.mark.parametrize("game,precision", [("connect4", "bf16"), ("tawlbwrdd", "bf16"), ("brandubh", "bf16"), ("stargambit", "fp32")])
def test_count_is_read_on_the_device_at_kernel_time(game, precision):
    """assertion 5: the count is written by a device op on the same stream right before the call, nothing waits in between;
    the same buffers then serve a second call with another count and list"""
    spec, hip, x, ref = _setup(game, precision)
    counts = torch.tensor([23, 0, 9], dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), S, dtype=torch.int32, device="cuda")       # stale: a host-side read would take all S
    rows = torch.empty(S, dtype=torch.int32, device="cuda")
    la, ra = _lists(23, seed=1)
    lb, rb = _lists(9, seed=2)
    v, pi = _buffers(spec)
    torch.cuda.synchronize()
    rows.copy_(ra); cnt.copy_(counts[0:1])
    hip.forward_rows(x, v, pi, rows, cnt)
    va, pa = v.clone(), pi.clone()
    v.fill_(SENTINEL); pi.fill_(SENTINEL)
    rows.copy_(rb); cnt.copy_(counts[2:3])
    hip.forward_rows(x, v, pi, rows, cnt)
    torch.cuda.synchronize()
    _untouched(va, pa, la, "first call")
    _check_listed(hip, precision, x, ref, va, pa, la, f"{game} first call")
    _untouched(v, pi, lb, "second call")
    _check_listed(hip, precision, x, ref, v, pi, lb, f"{game} second call")


@pytest.mark.parametrize("game,precision", [("tawlbwrdd", "bf16"), ("brandubh", "bf16"), ("stargambit", "bf16"), ("tawlbwrdd", "bf16x3")])
def test_spatial_net_shared_by_two_streams(game, precision):
    """assertion 6: two streams share one spatial net, different lists and different max_rows, enqueued back to back; each
    gets the answers of its own serial run.  The pooled features between the tile and the FC kernels are per stream
    (StreamScratch); the second round's max_rows is above the first reservation of its stream (reserve_pool regrows)."""
    spec, hip, x, _ = _setup(game, precision)
    big = 4096 + 48
    la, ra = _lists(37, seed=11, length=big)
    lb, rb = _lists(203, seed=12)
    ca = torch.tensor([37], dtype=torch.int32, device="cuda")
    cb = torch.tensor([203], dtype=torch.int32, device="cuda")
    # serial runs
    va0, pa0 = _buffers(spec); vb0, pb0 = _buffers(spec)
    hip.forward_rows(x, va0, pa0, ra, ca, max_rows=S)
    torch.cuda.synchronize()
    hip.forward_rows(x, vb0, pb0, rb, cb)
    torch.cuda.synchronize()
    _check_listed(hip, precision, x, None, va0, pa0, la, "serial a")
    _check_listed(hip, precision, x, None, vb0, pb0, lb, "serial b")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    va, pa = _buffers(spec); vb, pb = _buffers(spec)
    va2, pa2 = _buffers(spec); vb2, pb2 = _buffers(spec)
    torch.cuda.synchronize()
    for _ in range(2):          # twice: first use of each stream (reservation), then the steady state
        with torch.cuda.stream(sa):
            hip.forward_rows(x, va, pa, ra, ca, max_rows=S)
        with torch.cuda.stream(sb):
            hip.forward_rows(x, vb, pb, rb, cb)
    # stream a again with a max_rows above its reservation while b's work may still be in flight, then b once more
    with torch.cuda.stream(sa):
        hip.forward_rows(x, va2, pa2, ra, ca, max_rows=big)
    with torch.cuda.stream(sb):
        hip.forward_rows(x, vb2, pb2, rb, cb)
    torch.cuda.synchronize()
    for got, want, who in ((va, va0, "a v"), (pa, pa0, "a pi"), (vb, vb0, "b v"), (pb, pb0, "b pi"),
                           (va2, va0, "a v regrown"), (pa2, pa0, "a pi regrown"), (vb2, vb0, "b v after regrow"), (pb2, pb0, "b pi after regrow")):
        assert torch.equal(got, want), who


@pytest.mark.parametrize("game,precision", KERNELS)
def test_count_zero_is_a_no_op(game, precision):
    """assertion 7: count 0 with max_rows > 0 returns OK and changes nothing; so does max_rows 0"""
    spec, hip, x, _ = _setup(game, precision)
    _, rows = _lists(0, seed=3)
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    v, pi = _buffers(spec)
    hip.forward_rows(x, v, pi, rows, cnt)
    hip.forward_rows(x, v, pi, rows, torch.full((1,), 5, dtype=torch.int32, device="cuda"), max_rows=0)
    torch.cuda.synchronize()
    assert bool((v == SENTINEL).all()) and bool((pi == SENTINEL).all())
