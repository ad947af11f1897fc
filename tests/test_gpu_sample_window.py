"""-m gpu: the history window and the reservoir on the device - azmi_samples_reservoir_keys, azmi_samples_select_top,
azmi_samples_window_gather and what alphazero.samples builds on them (reservoir_keys, select_top, window_batches, SampleWindow,
selfplay.training_batches).  The yardstick is tests/sample_window_ref.py: numpy float64 and uint64, a stable argsort, the Feistel
permutation."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import sample_window_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# The largest distance between a device key and the numpy float64 key, measured over 10^6 rows with ages 0..200 at every decay of
# DECAYS: 4 ULP (1 at decay 1.0, 4 at 0.98, 2 at 0.5).  The bound is twice that, and never above 16.
KEY_ULP_MEASURED = 4
KEY_ULP_BOUND = min(16, 2 * KEY_ULP_MEASURED)
DECAYS = (1.0, 0.98, 0.5)


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


def _ulp_distance(a, b):
    """the number of float64 values between a and b, for finite values of one sign"""
    assert np.isfinite(a).all() and np.isfinite(b).all() and (np.signbit(a) == np.signbit(b)).all()
    return np.abs(a.view(np.int64) - b.view(np.int64))


# ---- select_top -------------------------------------------------------------------------------------------------------------------
def _key_sets(n, rng):
    bits = lambda b: np.asarray(b, dtype=np.uint64).view(np.float64)
    with_inf = rng.standard_normal(n)
    with_inf[rng.random(n) < 0.3] = -np.inf
    return {
        "distinct": rng.standard_normal(n),
        "all equal": np.full(n, -1.25),
        "three values": rng.choice(np.array([-2.0, 0.5, 3.0]), n),
        "low 8 bits": bits(np.uint64(0x3FF8000000000000) | rng.integers(0, 256, n, dtype=np.uint64)),
        # (the low 56 bits keep the exponent's low nibble 0: no pattern is an infinity or a NaN)
        "high 8 bits": bits((rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x0002345678ABCDEF)),
        "with -inf": with_inf,
        "signs and zeros": rng.choice(np.array([-3.5, -1.0, -0.0, 0.0, 1.0, 2.0]), n),
    }


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097, 70001])
def test_select_top_is_the_stable_argsort_bit_for_bit(az, n):
    rng = np.random.default_rng(20261021 + n)
    for name, keys in _key_sets(n, rng).items():
        assert not np.isnan(keys).any()
        for k in sorted({0, 1, n - 1, n, n // 2}):
            index, record = az.select_top(keys, k)
            want = ref.select_top(keys, k)
            assert index.dtype == np.int64 and np.array_equal(index, want), f"{name}, n = {n}, k = {k}"
            assert record["selected"] == k and record["first_bad_row"] is None
            if k:
                assert record["threshold_key"] == np.sort(keys)[n - k], f"{name}, n = {n}, k = {k}: the threshold"


def test_select_top_on_cuda_tensors_and_run_to_run(az):
    import torch
    rng = np.random.default_rng(5)
    keys = rng.choice(rng.standard_normal(500), 70001)      # many ties
    t = torch.from_numpy(keys).cuda()
    first, record = az.select_top(t, 30000)
    assert first.is_cuda and first.dtype == torch.int64 and np.array_equal(first.cpu().numpy(), ref.select_top(keys, 30000))
    for _ in range(3):
        assert torch.equal(az.select_top(t, 30000)[0], first)
    empty, record = az.select_top(t, 0)
    assert empty.is_cuda and empty.shape == (0,) and record["selected"] == 0


def test_select_top_names_the_first_nan_row(az):
    keys = np.random.default_rng(6).standard_normal(4097)
    keys[[3000, 37, 513]] = np.nan
    with pytest.raises(RuntimeError, match=r"select_top: 3 of 4097 keys are NaN, the first at row 37 \(first_bad_row\)"):
        az.select_top(keys, 100)
    keys[[3000, 37, 513]] = -np.inf      # legal: they lose to every finite key
    assert np.array_equal(az.select_top(keys, 4094)[0], ref.select_top(keys, 4094))


# ---- reservoir_keys -----------------------------------------------------------------------------------------------------------------
def test_reservoir_keys_against_numpy_float64(az):
    """u_i bit-exact as an integer; the key within KEY_ULP_BOUND of numpy's (log and pow are not correctly rounded on either side)"""
    n, seed, iteration = 1_000_000, 0xC0FFEE1234567, 200
    iters = (iteration - (np.arange(n) % 201)).astype(np.int32)      # ages 0 .. 200
    ids = np.random.default_rng(8).integers(0, 1 << 64, n, dtype=np.uint64)
    for decay in DECAYS:
        for row_ids in (None, ids):
            keys, m = az.reservoir_keys(iters, iteration, decay, seed, row_ids=row_ids, with_bits=True)
            assert keys.dtype == np.float64 and m.dtype == np.uint64
            assert np.array_equal(m, ref.uniform_bits(seed, np.arange(n) if row_ids is None else row_ids))
            want = ref.reservoir_keys(iters, iteration, decay, seed, row_ids=row_ids)
            d = _ulp_distance(keys, want)
            print(f"decay {decay}, row ids {'given' if row_ids is not None else 'implicit'}: largest distance {int(d.max())} ULP, "
                  f"{int((d > 0).sum())} of {n} keys differ")
            assert (keys < 0).all() and int(d.max()) <= KEY_ULP_BOUND


def test_reservoir_keys_at_decay_one_and_at_underflow(az):
    """decay = 1: w_i is exactly 1 at every age, so the key is log(u_i) as the formula rounds it - the same bits as at age 0, and
    numpy's log(u_i) within the bound of the log alone; an age whose weight underflows gives -inf"""
    n, seed = 4097, 99
    aged = az.reservoir_keys(np.arange(n, dtype=np.int32) % 300, 250, 1.0, seed)
    fresh = az.reservoir_keys(np.full(n, 250, np.int32), 250, 1.0, seed)
    assert np.array_equal(aged.view(np.int64), fresh.view(np.int64))
    u = ref.uniform_bits(seed, np.arange(n)).astype(np.float64) * 2.0 ** -53
    assert int(_ulp_distance(aged, np.log(u)).max()) <= KEY_ULP_BOUND
    future = az.reservoir_keys(np.full(n, 900, np.int32), 250, 0.5, seed)      # a row from a later iteration has age 0
    assert np.array_equal(future.view(np.int64), fresh.view(np.int64))
    iters = np.zeros(n, np.int32)
    assert np.array_equal(az.reservoir_keys(iters, 5000, 0.5, seed), np.full(n, -np.inf))      # 0.5 ** 5000 == 0
    keys = az.reservoir_keys(np.array([0, 4000, 0, 5000], np.int32), 5000, 0.5, seed)
    assert np.isneginf(keys[[0, 2]]).all() and np.isfinite(keys[[1, 3]]).all()
    assert np.array_equal(az.select_top(keys, 2)[0], [1, 3])      # -inf loses to every finite key


# ---- window_gather ----------------------------------------------------------------------------------------------------------------
def _segments(rows_list, row, rng):
    """row r of the window carries r in canonical[0] and v[0]; the rest is random"""
    out, at = [], 0
    for n in rows_list:
        c = rng.standard_normal((n, 1, 1, row)).astype(np.float32)
        v, pi = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 4 if row % 2 == 0 else 7)).astype(np.float32)
        c[:, 0, 0, 0] = v[:, 0] = np.arange(at, at + n)
        out.append((c, v, pi))
        at += n
    return out


SEGMENT_LISTS = {
    "one": [1000],
    "two": [1, 702],
    "sixty-four": [(0, 1, 37, 0, 5, 300, 1, 64)[s % 8] for s in range(64)],
    "empty ends": [0, 0, 611, 0],
}


@pytest.mark.parametrize("row", [1, 3, 7, 168, 169])
@pytest.mark.parametrize("name", list(SEGMENT_LISTS))
def test_window_batches_are_the_permuted_concatenation(az, name, row):
    rng = np.random.default_rng(row * 1000 + len(name))
    segments = _segments(SEGMENT_LISTS[name], row, rng)
    whole = [np.concatenate([seg[a] for seg in segments]) for a in range(3)]
    total = whole[0].shape[0]
    assert total & (total - 1), "the total is no power of two"
    seed = 20261021
    perms = [ref.permutation(total, seed, p) for p in (0, 1)]
    assert not np.array_equal(perms[0], perms[1])
    for p, perm in enumerate(perms):      # a whole pass in batches of 256 + 37 rows: every row once, the last batch short
        got = list(az.window_batches(segments, 293, seed, pass_index=p))
        assert len(got) == -(-total // 293) and got[-1][0].shape[0] == total - 293 * (len(got) - 1)
        for a in range(3):
            assert np.array_equal(np.concatenate([b[a] for b in got]), whole[a][perm]), f"array {a}, pass {p}"
        assert np.array_equal(np.sort(np.concatenate([b[1][:, 0] for b in got])), np.arange(total))
    # a cut that starts and ends inside a segment
    first = total // 3 + 1
    got = list(az.window_batches(segments, 37, seed, pass_index=1, first=first, batches=3))
    assert len(got) == 3
    for a in range(3):
        assert np.array_equal(np.concatenate([b[a] for b in got]), whole[a][perms[1][first:first + 111]])


def test_window_batches_on_cuda_tensors_and_views(az):
    """CUDA segments in place: 16-byte rows on the vector path, a view that starts off a 16-byte boundary on the dword path"""
    import torch
    rng = np.random.default_rng(77)
    segments = _segments([300, 1, 0, 511], 168, rng)
    flat = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), segments[3][2].ravel()])).cuda()
    on_dev = [tuple(torch.from_numpy(x).cuda() for x in seg) for seg in segments]
    on_dev[3] = (on_dev[3][0], on_dev[3][1], flat[1:].view(511, 4))      # pi of the last segment: 4 bytes past a 16-byte boundary
    assert on_dev[3][2].data_ptr() % 16 == 4 and on_dev[3][2].is_contiguous()
    whole = [np.concatenate([seg[a] for seg in segments]) for a in range(3)]
    perm = ref.permutation(812, 3, 2)
    got = list(az.window_batches(on_dev, 500, 3, pass_index=2))
    assert [b[0].shape[0] for b in got] == [500, 312] and all(x.is_cuda for b in got for x in b)
    for a in range(3):
        assert np.array_equal(torch.cat([b[a] for b in got]).cpu().numpy(), whole[a][perm])


# ---- SampleWindow -----------------------------------------------------------------------------------------------------------------
def _iteration(t, n):
    """row i of iteration t carries (t, i) in its planes"""
    c = np.zeros((n, 2, 1, 3), np.float32)
    c[:, 0], c[:, 1] = t, np.arange(n)[:, None, None]
    v = np.stack([np.full(n, t), np.arange(n), np.zeros(n)], axis=1).astype(np.float32)
    pi = np.repeat((t * 1000.0 + np.arange(n))[:, None], 7, axis=1).astype(np.float32)
    return c, v, pi


def test_sample_window_end_to_end(az):
    import torch
    from alphazero import selfplay, _rng
    R, decay, seed = 60, 0.7, 424242
    w = az.SampleWindow(hist_size=2, reservoir_rows=R, decay=decay, seed=seed)
    data = {t: _iteration(t, 50 + 7 * t) for t in range(5)}
    res, selecting = None, 0      # the model: (canonical, v, pi, iterations, row ids) of the reservoir
    for t in range(5):
        tensors = tuple(torch.from_numpy(x).cuda() for x in data[t])
        w.append(t, tensors)
        newest = w.segments()[len(w.stats()["window_iterations"]) - 1]
        assert [x.data_ptr() for x in newest] == [x.data_ptr() for x in tensors]      # no copy of a CUDA tensor
        staged = [t - 2] if t >= 2 else []
        assert w.stats()["staged_rows"] == sum(len(data[s][0]) for s in staged)
        kept = w.update_reservoir(t)
        stats = w.stats()
        assert stats["window_iterations"] == [s for s in (t - 1, t) if s >= 0]      # exactly the last two
        assert stats["window_rows"] == sum(len(data[s][0]) for s in stats["window_iterations"])
        assert stats["staged_rows"] == 0 and stats["evicted_iterations"] == max(0, t - 1)
        for s in staged:
            n = len(data[s][0])
            new = data[s] + (np.full(n, s, np.int32), np.arange(n, dtype=np.int64) + (s << 32))
            pool = new if res is None else tuple(np.concatenate([a, b]) for a, b in zip(res, new))
            if len(pool[0]) > R:
                selecting += 1
                last = w.last_update
                assert last["iteration"] == t and last["pool_rows"] == len(pool[0])
                assert np.array_equal(last["pool_iterations"].cpu().numpy(), pool[3]) and np.array_equal(last["pool_row_ids"].cpu().numpy(), pool[4])
                keys = last["keys"].cpu().numpy()      # the device's own keys: the selection below is exact
                useed = _rng.mix64((seed + 0x9E3779B97F4A7C15 * (t + 1)) & _rng.MASK64)
                assert int(_ulp_distance(keys, ref.reservoir_keys(pool[3], t, decay, useed, row_ids=pool[4])).max()) <= KEY_ULP_BOUND
                index = ref.select_top(keys, R)
                assert np.array_equal(last["index"].cpu().numpy(), index)
                res = tuple(x[index] for x in pool)
            else:
                res = pool
        assert kept == stats["reservoir_rows"] == (0 if res is None else len(res[0]))
        if res is not None:
            for got, want in zip(w.segments()[-1], res[:3]):
                assert np.array_equal(got.cpu().numpy(), want)
        assert stats["host_syncs"] == selecting      # one per update_reservoir that selects
    assert selecting == 2 and len(res[0]) == R and len(set(res[3])) > 1      # iterations 1 and 2 pushed rows out

    # batches(): train()'s step budget, from window + reservoir, no synchronisation
    syncs = w.stats()["host_syncs"]
    rows_in = {(int(a), int(b)) for x in (data[3][1], data[4][1], res[1]) for a, b in x[:, :2]}
    total, average = len(rows_in), (len(data[3][0]) + len(data[4][0])) / 2
    assert total == len(data[3][0]) + len(data[4][0]) + R
    for batch_rows, rate in ((16, 1.0), (16, 0.3), (64, 1.0)):
        got = list(selfplay.training_batches(w, batch_rows, sample_rate=rate, pass_seed=11))
        assert len(got) == math.ceil(average / batch_rows * rate) and len(got) * batch_rows <= total
        assert all(c.is_cuda and c.shape[0] == v.shape[0] == pi.shape[0] == batch_rows for c, v, pi in got)
        seen = [(int(a), int(b)) for _, v, _ in got for a, b in v.cpu().numpy()[:, :2]]
        assert len(set(seen)) == len(seen) and set(seen) <= rows_in      # one pass visits a row at most once
        for c, v, pi in got:      # a row's three arrays travel together
            c, v, pi = c.cpu().numpy(), v.cpu().numpy(), pi.cpu().numpy()
            assert np.array_equal(c[:, 0, 0, 0], v[:, 0]) and np.array_equal(c[:, 1, 0, 0], v[:, 1])
            assert np.array_equal(pi[:, 0], v[:, 0] * 1000 + v[:, 1])
    # a budget beyond one pass: the pass ends with a short batch and the next one begins
    got = list(w.batches(100, sample_rate=6.0, pass_seed=11))
    assert len(got) == math.ceil(average / 100 * 6.0) == 5
    assert [b[0].shape[0] for b in got] == [100, 100, total - 200, 100, 100]
    first_pass = [(int(a), int(b)) for _, v, _ in got[:3] for a, b in v.cpu().numpy()[:, :2]]
    assert sorted(first_pass) == sorted(rows_in)
    assert w.stats()["host_syncs"] == syncs      # zero per batches()


# ---- the distribution ---------------------------------------------------------------------------------------------------------------
def test_the_selection_draws_successive_weighted_samples(az):
    """The k largest exponential keys are successive sampling: P(i1, i2, i3) = w1 / S * w2 / (S - w1) * w3 / (S - w1 - w2).  The
    inclusion frequency of every row over 20 000 seeds against the exact probability, within 5 standard errors of a binomial with
    20 000 trials (a bound derived here, two-sided tail below 1e-6 per row)."""
    import torch
    n, k, decay, trials = 8, 3, 0.7, 20_000
    w = decay ** np.arange(n, dtype=np.float64)      # ages 0 .. 7
    p = np.zeros(n)
    for triple in itertools.permutations(range(n), k):
        prob, left = 1.0, w.sum()
        for i in triple:
            prob *= w[i] / left
            left -= w[i]
        p[list(triple)] += prob
    assert abs(p.sum() - k) < 1e-12
    tol = 5 * np.sqrt(p * (1 - p) / trials)
    iteration = 7
    iters = (iteration - np.arange(n)).astype(np.int32)
    seeds = np.arange(trials, dtype=np.uint64) * np.uint64(7919) + np.uint64(20261021)
    # on the CPU first: the restatement over these seeds stays inside the bound
    u = ref.uniform_bits(seeds[:, None], np.arange(n)[None, :]).astype(np.float64) * 2.0 ** -53
    keys = np.log(u) / w[None, :]
    freq = np.bincount(np.argsort(-keys, axis=1, kind="stable")[:, :k].ravel(), minlength=n) / trials
    print("exact", np.round(p, 4), "numpy", np.round(freq, 4), "tolerance", np.round(tol, 4))
    assert (np.abs(freq - p) <= tol).all()
    # then the device: keys and selection, one call each per seed
    iters_t = torch.from_numpy(iters).cuda()
    counts = torch.zeros(n, dtype=torch.int64, device="cuda")
    ones = torch.ones(k, dtype=torch.int64, device="cuda")
    for seed in seeds.tolist():
        index, _ = az.select_top(az.reservoir_keys(iters_t, iteration, decay, seed), k)
        counts.index_add_(0, index, ones)
    freq = counts.cpu().numpy() / trials
    print("device", np.round(freq, 4))
    assert (np.abs(freq - p) <= tol).all()


# ---- the README -------------------------------------------------------------------------------------------------------------------
def test_readme_window_example_runs_as_written(az):
    """the indented lines under the README's history-window paragraph, with the `samples` and `net` of the README's earlier snippets"""
    import torch
    from alphazero import selfplay, torch_net
    readme = open(os.path.join(ROOT, "README.md")).read()
    block = re.search(r"The history window and the recency-weighted reservoir(?s:.*?)\n\n((?:    .*\n)+)", readme).group(1)
    lines = [ln[4:] for ln in block.splitlines()]
    assert len(lines) == 5 and "SampleWindow" in block and "training_batches" in block and "update_reservoir" in block
    fx = np.load(os.path.join(HERE, "golden", "nn_connect4_6b64c.npz"))
    net = torch_net.LeafNet(torch_net.connect4_spec())
    net.load_state_dict({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")})
    net = az.HipLeafNet(net.eval())
    params = az.PlayParams()
    params.games_to_play, params.concurrent_games, params.max_batch_size = 8, 8, 8
    params.mcts_visits = [16, 16]; params.model_groups = [0, 0]; params.history_enabled = True
    result, samples = selfplay.self_play(az.Connect4GS, params, net, engines=2)
    scope = {"alphazero": az, "selfplay": selfplay, "samples": samples, "net": net, "iteration": 0, "steps": 0}
    exec("\n".join(lines), scope)
    rows = scope["window"].stats()["window_rows"]
    assert rows > samples[0].shape[0] > 0 and scope["steps"] == math.ceil(rows / 1024)
    assert scope["canonical"].shape[0] == scope["v"].shape[0] == scope["pi"].shape[0] == rows - 1024 * (scope["steps"] - 1)
