"""-m gpu: the sample path between self-play and training on the device - the per-row surprise loss (azmi_sample_loss), the
resample plan (azmi_resample_plan), the row gather (azmi_resample_gather) and the functions of alphazero.samples built on them,
up to selfplay.process_samples on Connect4 samples.  The yardstick is a few lines of numpy float64 written here (the
expressions of game_runner.py:1183-1193 and neural_net.py:875-886), with MCTSBatch._mix64 for the draw u_i."""
import math
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = 0x9E3779B97F4A7C15
FLT_MIN = float(np.finfo(np.float32).tiny)      # 1.17549435e-38


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


def _block():
    """kPlanBlock, from the kernel header"""
    header = open(os.path.join(ROOT, "alphazero-pybind11_amd", "csrc", "samples_kernels.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+kPlanBlock\s*=\s*(\d+)\s*;", header).group(1))


BLOCK = _block()


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _loss_ref(t, p, scale=1.0):
    t64, p64 = t.astype(np.float64), p.astype(np.float64)
    terms = np.where(t64 > 0, t64 * np.log(np.maximum(p64, FLT_MIN)), 0.0)
    return -scale * np.sum(terms, axis=1)


def _uniforms(az, seed, n):
    """u_i = (mix64(seed + GOLDEN * (i + 1)) >> 11) * 2^-53, arithmetic mod 2^64 (uint64 arrays wrap)"""
    i = np.arange(1, n + 1, dtype=np.uint64)
    x = az.MCTSBatch._mix64(np.uint64(seed) + np.uint64(GOLDEN) * i)
    u = (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    for j in (0, n // 2, n - 1):      # the array form is the scalar function
        assert u[j] == (az.MCTSBatch._mix64((seed + GOLDEN * (j + 1)) & (2 ** 64 - 1)) >> 11) * 2.0 ** -53
    return u


def _plan_ref(az, loss, seed, total):
    """game_runner.py:1186-1193 with our draw -> (copies, frac, u)"""
    n = len(loss)
    u = _uniforms(az, seed, n)
    if total <= 0:
        return np.ones(n, np.int64), np.zeros(n), u
    w = 0.5 + (loss / total) * 0.5 * n
    k = np.floor(w)
    frac = w - k
    return k.astype(np.int64) + (u < frac).astype(np.int64), frac, u


def _assert_plan(az, loss, seed, got, excluded_allowed=0):
    copies, offsets, rows_out, total = got
    n = len(loss)
    assert copies.dtype == np.uint32 and offsets.dtype == np.uint64 and copies.shape == offsets.shape == (n,)
    exact = math.fsum(loss)
    print(f"n = {n}: total_loss {total!r}, fsum {exact!r}, relative difference {abs(total - exact) / exact if exact else 0.0:.3e}")
    assert abs(total - exact) <= n * 2.0 ** -53 * abs(exact)      # the worst case of any summation order over terms of one sign
    c64 = copies.astype(np.int64)
    assert np.array_equal(offsets.astype(np.int64), np.cumsum(c64) - c64)
    assert rows_out == int(c64.sum())
    want, frac, u = _plan_ref(az, loss, seed, total)      # (with the device's own total)
    decided = np.abs(frac - u) > 1e-9
    print(f"n = {n}: {int((~decided).sum())} rows within 1e-9 of their draw, rows_out {rows_out}")
    assert int((~decided).sum()) <= excluded_allowed
    assert np.array_equal(c64[decided], want[decided])


# ---- loss ------------------------------------------------------------------------------------------------------------------------
LOSS_M = (1, 3, 7, 8, 9, 63, 64, 65, 1000)
LOSS_N = (1, 2, 257)


def _loss_case(M, n):
    """random targets and probabilities with the edge rows in: row 0 has a positive target on p = 0 (entry 0) and, for M > 1, a zero
    target on p = 0 (entry 1); row 1 has all-zero targets; from n = 257 on more of each, and rows with a single one-hot target"""
    rng = np.random.default_rng(1000 * M + n)
    t = rng.random((n, M)).astype(np.float32)
    t[rng.random((n, M)) < 0.3] = 0.0
    t[:, 0] = np.maximum(t[:, 0], np.float32(0.01))
    t /= t.sum(axis=1, keepdims=True)
    p = rng.random((n, M)).astype(np.float32) + np.float32(1e-6)
    p /= p.sum(axis=1, keepdims=True)
    for r in range(0, n, 16):
        p[r, 0] = 0.0
        if M > 1:
            t[r, 1] = 0.0
            p[r, 1] = 0.0
    for r in range(1, n, 16):
        t[r] = 0.0
        p[r, M - 1] = 0.0
    for r in range(2, n, 16):
        t[r] = 0.0
        t[r, (r * 7) % M] = 1.0
    return t, p


def _assert_loss(M, got, t, p, scale=1.0):
    want = _loss_ref(t, p, scale)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    bound = (M + 2) * 2.0 ** -52 * np.abs(want)      # one ulp for log, one for the product, M for the sum; every term has one sign
    print(f"M = {M}, n = {len(got)}: largest error {float((err / np.maximum(np.abs(want), 1e-300)).max()):.3e} relative, "
          f"bound {(M + 2) * 2.0 ** -52:.3e}")
    assert (err <= bound).all()
    zero_rows = ~(t > 0).any(axis=1)
    assert (got[zero_rows] == 0.0).all()      # exactly
    return want


@pytest.mark.parametrize("n", LOSS_N)
@pytest.mark.parametrize("M", LOSS_M)
def test_sample_loss_is_the_float64_cross_entropy(az, M, n):
    t, p = _loss_case(M, n)
    got = az.sample_loss(t, p)
    _assert_loss(M, got, t, p)
    # a positive target on p = 0 is finite: -t * log(FLT_MIN) is one of the row's terms
    assert got[0] >= -float(t[0, 0]) * math.log(FLT_MIN) * (1 - 2.0 ** -50)
    if n > 1:
        assert got[1] == 0.0 and not np.signbit(got[1])
    if n == 257:
        # the same rows inside a smaller n: the same bits (a row does not depend on n or on the launch geometry)
        for k in (1, 2, 5):
            assert np.array_equal(az.sample_loss(t[:k].copy(), p[:k].copy()), got[:k])
        assert np.array_equal(az.sample_loss(t[250:].copy(), p[250:].copy()), got[250:])


def test_sample_loss_scale_and_single_terms(az):
    t = np.zeros((4, 3), np.float32)
    p = np.full((4, 3), 1 / 3, np.float32)
    t[0, 1] = 0.75; p[0, 1] = 0.0                      # a positive target on an underflowed probability
    t[1, 2] = 1.0; p[1, 2] = 0.25                      # one term
    p[2] = 0.0                                         # zero targets on p = 0: no NaN, exactly 0
    t[3] = (0.5, 0.25, 0.25); p[3] = (1e-45, 0.5, 0.5)      # a denormal probability is floored too
    for cv in (1.0, 1.5):
        got = az.sample_loss(t, p, scale=cv)
        assert abs(got[0] - (-cv * 0.75 * math.log(FLT_MIN))) <= 5 * 2.0 ** -52 * abs(got[0])
        assert abs(got[1] - (-cv * math.log(0.25))) <= 5 * 2.0 ** -52 * abs(got[1])
        assert got[2] == 0.0
        _assert_loss(3, got, t, p, cv)


def test_sample_loss_on_cuda_tensors_is_the_staged_result(az):
    import torch
    t, p = _loss_case(7, 257)
    dev = torch.device("cuda", 0)
    got = az.sample_loss(torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev), scale=2.0)
    assert got.is_cuda and got.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), az.sample_loss(t, p, scale=2.0))


# ---- plan ------------------------------------------------------------------------------------------------------------------------
PLAN_N = (1, 2, BLOCK, BLOCK + 1, BLOCK * BLOCK + 1, 2 ** 20 + 3)      # BLOCK^2 + 1: the first n whose scan has a third level


def _plan_case(n):
    return np.random.default_rng(20261020 + n).random(n), 0xC0FFEE00 + n


@pytest.mark.parametrize("n", PLAN_N)
def test_resample_plan_is_the_reference_rule_with_our_draw(az, n):
    assert BLOCK == 1024, "PLAN_N was chosen for tiles of 1024: BLOCK^2 + 1 and 2^20 + 3 must both need the third level"
    loss, seed = _plan_case(n)
    _assert_plan(az, loss, seed, az.resample_plan(loss, seed))


def test_resample_plan_all_zero_loss_gives_ones(az):
    for n in (1, 5, BLOCK + 7):
        copies, offsets, rows_out, total = az.resample_plan(np.zeros(n), 11)
        assert total == 0.0 and rows_out == n and (copies == 1).all() and np.array_equal(offsets, np.arange(n, dtype=np.uint64))


def test_resample_plan_bits_do_not_depend_on_the_run_or_the_stream(az):
    import torch
    loss, seed = _plan_case(BLOCK * 3 + 5)
    first = az.resample_plan(loss, seed)
    again = az.resample_plan(loss, seed)
    dev = torch.device("cuda", 0)
    lt = torch.from_numpy(loss).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    c, o, rows_out, total = az.resample_plan(lt, seed, stream=side.cuda_stream)
    assert c.dtype == torch.int32 and o.dtype == torch.int64 and c.is_cuda and o.is_cuda
    other = (c.cpu().numpy().view(np.uint32), o.cpu().numpy().view(np.uint64), rows_out, total)
    for got in (again, other):
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]) and got[2] == first[2]
        assert np.float64(got[3]).tobytes() == np.float64(first[3]).tobytes()
    assert not np.array_equal(az.resample_plan(loss, seed + 1)[0], first[0])      # (the seed is the draw)


def test_resample_plan_names_the_first_non_finite_row(az):
    loss = np.random.default_rng(3).random(3000)
    loss[5] = np.nan
    with pytest.raises(RuntimeError, match=r"resample_plan: 1 of 3000 losses are not finite, the first at row 5 \(first_nonfinite\)"):
        az.resample_plan(loss, 1)
    loss[2999] = np.inf
    loss[1500] = -np.inf
    with pytest.raises(RuntimeError, match=r"3 of 3000 losses are not finite, the first at row 5 "):
        az.resample_plan(loss, 1)


def _skewed(n=1000, heavy=123):
    """one row carries 99 % of the loss: w = 0.5 + 0.99 * 0.5 * n"""
    loss = np.full(n, 0.01 / (n - 1))
    loss[heavy] = 0.99
    return loss


def test_resample_plan_skewed_row_stays_exact(az):
    loss = _skewed()
    got = az.resample_plan(loss, 77)
    _assert_plan(az, loss, 77, got)
    assert got[0][123] in (495, 496) and got[2] >= 495


# ---- gather ----------------------------------------------------------------------------------------------------------------------
def _plans(az):
    with_zeros = np.random.default_rng(8).random(1000)
    with_zeros[np.random.default_rng(9).random(1000) < 0.4] = 0.0      # w = 0.5: a coin decides between 0 and 1 copies
    plans = {"skewed": az.resample_plan(_skewed(), 77), "with zeros": az.resample_plan(with_zeros, 78)}
    assert (plans["with zeros"][0] == 0).sum() > 100 and plans["skewed"][0].max() >= 495
    return plans


def test_resample_rows_is_numpy_repeat(az):
    import torch
    rng = np.random.default_rng(12)
    n = 1000
    v = rng.random((n, 3)).astype(np.float32)             # 12 B rows: dwords
    canon = rng.random((n, 4, 6, 7)).astype(np.float32)   # 672 B rows: 16-byte accesses
    pi = rng.random((n, 7)).astype(np.float32)            # 28 B rows: dwords
    dev = torch.device("cuda", 0)
    for name, (copies, offsets, rows_out, _) in _plans(az).items():
        idx = np.repeat(np.arange(n), copies.astype(np.int64))
        got = az.resample_rows(copies, offsets, canon, v, pi)                # numpy, rows_out from the copies
        for g, x in zip(got, (canon, v, pi)):
            assert g.dtype == np.float32 and g.shape == (rows_out,) + x.shape[1:] and np.array_equal(g, x[idx]), name
        # CUDA tensors, with a 672 B array whose base sits 4 bytes past a 16-byte boundary: the vector path must decline it
        big = torch.zeros(n * 168 + 1, dtype=torch.float32, device=dev)
        view = big[1:].view(n, 4, 6, 7)
        view.copy_(torch.from_numpy(canon))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        ct = torch.from_numpy(copies.view(np.int32)).to(dev)
        ot = torch.from_numpy(offsets.view(np.int64)).to(dev)
        tens = az.resample_rows(ct, ot, view, torch.from_numpy(v).to(dev), torch.from_numpy(canon).to(dev), torch.from_numpy(pi).to(dev),
                                rows_out=rows_out)
        for g, x in zip(tens, (canon, v, canon, pi)):
            assert g.is_cuda and np.array_equal(g.cpu().numpy(), x[idx]), name
        one = az.resample_rows(ct, ot, torch.from_numpy(pi).to(dev))          # one array, rows_out read back
        assert np.array_equal(one[0].cpu().numpy(), pi[idx])


def test_azmi_resample_gather_with_several_arrays_in_one_call(az):
    """the exported entry point with n_arrays > 1 (resample_rows launches per array): the grid covers the array with the widest lane
    groups wherever it stands in the list, the arrays with narrower groups leave their surplus workgroups"""
    import ctypes as C
    import torch
    rng = np.random.default_rng(13)
    n = 1000
    dev = torch.device("cuda", 0)
    host = {"v": rng.random((n, 3)).astype(np.float32), "canon": rng.random((n, 4, 6, 7)).astype(np.float32),
            "pi": rng.random((n, 7)).astype(np.float32), "wide": rng.random((n, 300)).astype(np.float32)}      # 1200 B: 75 units, two passes
    tens = {k: torch.from_numpy(x).to(dev) for k, x in host.items()}
    big = torch.zeros(n * 168 + 1, dtype=torch.float32, device=dev)
    tens["view"] = big[1:].view(n, 4, 6, 7)      # 672 B rows 4 bytes past a 16-byte boundary: dwords
    tens["view"].copy_(tens["canon"])
    host["view"] = host["canon"]
    assert tens["view"].data_ptr() % 16 == 4
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for name, (copies, offsets, rows_out, _) in _plans(az).items():
        idx = np.repeat(np.arange(n), copies.astype(np.int64))
        ct = torch.from_numpy(copies.view(np.int32)).to(dev)
        ot = torch.from_numpy(offsets.view(np.int64)).to(dev)
        for order in (("canon", "v", "pi"), ("v", "pi", "canon", "view"), ("v", "pi"), ("pi", "view", "wide", "v", "canon", "v", "pi", "wide")):
            k = len(order)
            outs = [torch.zeros((rows_out,) + tuple(tens[a].shape[1:]), dtype=torch.float32, device=dev) for a in order]
            ins = (C.c_void_p * k)(*[tens[a].data_ptr() for a in order])
            dst = (C.c_void_p * k)(*[o.data_ptr() for o in outs])
            rb = (C.c_uint32 * k)(*[tens[a][0].numel() * 4 for a in order])
            rc = az.lib.azmi_resample_gather(ct.data_ptr(), ot.data_ptr(), n, k, ins, dst, rb, 0, stream)
            assert rc == 0, az.lib.azmi_samples_last_error().decode()
            for a, o in zip(order, outs):
                assert np.array_equal(o.cpu().numpy(), host[a][idx]), (name, order, a)


def test_resample_rows_with_nothing_to_write(az):
    copies = np.zeros(10, np.uint32)
    got = az.resample_rows(copies, np.zeros(10, np.uint64), np.ones((10, 7), np.float32))
    assert got[0].shape == (0, 7)


# ---- end to end on Connect4 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c4_net(az):
    import torch
    from alphazero import torch_net
    fx = np.load(os.path.join(HERE, "golden", "nn_connect4_6b64c.npz"))
    net = torch_net.LeafNet(torch_net.connect4_spec())
    net.load_state_dict({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")})
    return az.HipLeafNet(net.eval())


def _c4_params(az):
    params = az.PlayParams()
    params.games_to_play, params.concurrent_games, params.max_batch_size = 8, 8, 8
    params.mcts_visits = [16, 16]; params.model_groups = [0, 0]; params.history_enabled = True
    return params


def test_process_samples_on_connect4(az, c4_net, tmp_path):
    import torch
    from alphazero import selfplay, history_io
    result, samples = selfplay.self_play(az.Connect4GS, _c4_params(az), c4_net, engines=2)
    assert result.games == 8 and samples[0].shape[0] > 8 * 7
    folder = str(tmp_path / "history")
    (canonical, v, pi), loss = selfplay.process_samples(az.Connect4GS, samples, c4_net, seed=20261020, data_folder=folder, iteration=3)
    sc, sv, sp = (x.reshape((-1,) + tuple(x.shape[2:])) for x in az.symmetries_batch(az.Connect4GS, *samples))
    n = sc.shape[0]
    assert n == 2 * samples[0].shape[0] and loss.shape == (n,) and loss.dtype == torch.float64 and loss.is_cuda
    # the loss is the kernel on the net's own answers, bit for bit
    raw_v, raw_pi = c4_net.process(sc)
    assert torch.equal(loss, az.sample_loss(sp, raw_pi))
    # the rows are the numpy repeat of the symmetry-expanded samples under the plan of that loss
    copies, offsets, rows_out, total = az.resample_plan(loss.cpu().numpy(), 20261020)
    _assert_plan(az, loss.cpu().numpy(), 20261020, (copies, offsets, rows_out, total))
    idx = np.repeat(np.arange(n), copies.astype(np.int64))
    assert canonical.shape[0] == v.shape[0] == pi.shape[0] == rows_out
    for got, x in ((canonical, sc), (v, sv), (pi, sp)):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), x.cpu().numpy()[idx])
    # the .ptz triple holds them (stored as float16, like every sample file)
    triples = history_io.glob_file_triples(folder)
    assert len(triples) == 1 and triples[0][3] == rows_out and os.path.basename(triples[0][0]).startswith("0003-0000-canonical-")
    for path, x in zip(triples[0][:3], (canonical, v, pi)):
        assert torch.equal(history_io.load_compressed(path).float(), x.cpu().half().float())
    # iteration_losses: the two float64 means of the restatement
    v_loss, pi_loss = az.iteration_losses((sc, sv, sp), c4_net, cv=1.5)
    want_v = float(np.mean(_loss_ref(sv.cpu().numpy(), raw_v.cpu().numpy(), 1.5)))
    want_pi = float(np.mean(_loss_ref(sp.cpu().numpy(), raw_pi.cpu().numpy())))
    print(f"iteration_losses: v {v_loss!r} against {want_v!r}, pi {pi_loss!r} against {want_pi!r}, {n} rows")
    # a row is within (M + 2) * 2^-52 of the restatement (M = 3 and 7), a mean of n terms of one sign adds at most n * 2^-53
    assert abs(v_loss - want_v) <= ((3 + 2) * 2.0 ** -52 + n * 2.0 ** -53) * abs(want_v)
    assert abs(pi_loss - want_pi) <= ((7 + 2) * 2.0 ** -52 + n * 2.0 ** -53) * abs(want_pi)
    # a small batch_rows walks the same samples in chunks
    (c2, v2, p2), loss2 = az.resample_by_surprise((sc, sv, sp), c4_net, 20261020, batch_rows=64)
    assert torch.equal(c2, canonical) and torch.equal(v2, v) and torch.equal(p2, pi) and torch.equal(loss2, loss)


def test_readme_resample_example_runs_as_written(az, c4_net, tmp_path, monkeypatch):
    """the indented lines under the README's resample paragraph, with the `params` and `net` of the README's earlier snippets"""
    readme = open(os.path.join(ROOT, "README.md")).read()
    block = re.search(r"The two stages between self-play and training(?s:.*?)\n\n((?:    \S.*\n)+)", readme).group(1)
    lines = [ln[4:] for ln in block.splitlines()]
    assert len(lines) == 5 and "process_samples" in block and "iteration_losses" in block
    monkeypatch.chdir(tmp_path)
    from alphazero import selfplay
    scope = {"alphazero": az, "selfplay": selfplay, "params": _c4_params(az), "net": c4_net}
    exec("\n".join(lines), scope)
    assert scope["rows_out"] == len(scope["canonical"]) > 0 and scope["pi_loss"] > 0 and scope["v_loss"] > 0
    assert os.listdir(tmp_path / "history")
