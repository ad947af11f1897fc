"""-m gpu: the device-pointer surface of the position cache (find_rows, insert_many on CUDA tensors, cached_forward,
MCTSBatch.leaf_keys) against the oracle's restatement of s3fifo_cache.h, driven as tests/test_gpu_cache.py drives it, and against
a twin cache driven through the numpy entry points.  Nothing here is compared with the device path itself."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = -7.25          # no probability, no value
GOLDEN = 0x9E3779B97F4A7C15
K_APPLY_MAX = 8192        # csrc/dev_cache.h


@pytest.fixture(scope="module")
def az():
    import alphazero
    return alphazero


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _pv(keys, np_=7, nv=3):
    p = np.zeros((len(keys), np_), np.float32); v = np.zeros((len(keys), nv), np.float32)
    for i, k in enumerate(keys):
        r = np.random.default_rng([int(k) & 0xFFFFFFFF, int(k) >> 32])
        p[i] = r.random(np_, dtype=np.float32); v[i] = r.random(nv, dtype=np.float32)
    return p, v


def _dev_keys(torch, keys):
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda()


def _stats(torch, c):
    torch.cuda.synchronize()
    return dict(hits=c.hits(), misses=c.misses(), evictions=c.evictions(), reinserts=c.reinserts(), size=c.size(), max_size=c.max_size())


def _find(torch, dev, orc, keys, what, np_=7, nv=3):
    """find_rows on the device against the oracle's finds, one key at a time in row order"""
    n = len(keys)
    p = torch.full((n, np_), SENTINEL, device="cuda"); v = torch.full((n, nv), SENTINEL, device="cuda")
    hit, p2, v2, rows, count = dev.find_rows(_dev_keys(torch, keys), p_out=p, v_out=v)
    assert p2 is p and v2 is v
    hit, p, v, rows, count = hit.cpu().numpy(), p.cpu().numpy(), v.cpu().numpy(), rows.cpu().numpy(), int(count.cpu()[0])
    want_hit = np.zeros(n, bool)
    for i, k in enumerate(keys):
        want = orc.find(int(k))
        want_hit[i] = want is not None
        if want is None:
            assert (p[i] == SENTINEL).all() and (v[i] == SENTINEL).all(), (what, i, "a miss's rows were written")
        else:
            assert np.array_equal(p[i], want[0]) and np.array_equal(v[i], want[1]), (what, i)
    assert np.array_equal(hit, want_hit), what
    assert count == int((~want_hit).sum()) and np.array_equal(rows[:count], np.flatnonzero(~want_hit)), what


def _insert(torch, dev, orc, keys, what, rows=None, row_count=None):
    p, v = _pv(keys)
    kw = {}
    order = range(len(keys))
    if rows is not None:
        kw["rows"] = torch.tensor(list(rows), dtype=torch.int32, device="cuda")
        order = list(rows)
    if row_count is not None:
        kw["row_count"] = torch.tensor([row_count], dtype=torch.int32, device="cuda")
        order = list(order)[:row_count]
    dev.insert_many(_dev_keys(torch, keys), torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda(), **kw)
    for j in order:
        orc.insert(int(keys[j]), p[j], v[j])


@pytest.mark.parametrize("max_size,shards,ghost", [(256, 4, 230), (96, 3, 30)])      # 64-entry wave shards; the generic tables
def test_find_rows_and_insert_rows_match_the_oracle_op_by_op(az, torch, oracle, max_size, shards, ghost):
    dev = az.ShardedS3FIFOCache(max_size, shards, ghost, 7, 3)
    orc = oracle.Cache(max_size, shards, ghost, 7, 3)
    rng = np.random.default_rng(max_size + shards)
    universe = rng.choice(np.arange(1, 1 << 20, dtype=np.uint64) * np.uint64(0x9E3779B1), size=4 * max_size, replace=False)
    step = [0]

    def same(what):
        step[0] += 1
        got, want = _stats(torch, dev), orc.stats()
        assert got == want, (step[0], what, got, want)

    for size in (1, 5, 64):
        keys = universe[:size]
        _find(torch, dev, orc, keys, f"find {size} (cold)"); same("find")
        _insert(torch, dev, orc, keys, f"insert {size}"); same("insert")
        _find(torch, dev, orc, keys, f"find {size} (warm)"); same("find")
    # a key three times in one batch: the finds (all hit or all miss, the counters add up), then the insert (first in, rest present)
    rep = np.array([universe[70], universe[3], universe[70], universe[71], universe[70]], np.uint64)
    _find(torch, dev, orc, rep, "find with a key three times"); same("find x3")
    _insert(torch, dev, orc, rep, "insert with a key three times"); same("insert x3")
    _find(torch, dev, orc, rep, "find with a key three times, present"); same("find x3")
    # hash 0 is a key, and so is the value it is stored as (different shards in both layouts: 0 and 1)
    zero = np.array([0, universe[72], GOLDEN], np.uint64)
    _find(torch, dev, orc, zero, "find 0 and the golden key (absent)"); same("find 0")
    _insert(torch, dev, orc, zero, "insert 0 and the golden key"); same("insert 0")
    _find(torch, dev, orc, zero, "find 0 and the golden key"); same("find 0")
    # a row list in non-ascending order, a list cut short on the device, an empty one
    keys = universe[80:100]
    _insert(torch, dev, orc, keys, "rows descending", rows=[17, 11, 5, 4, 19, 0]); same("rows descending")
    _insert(torch, dev, orc, keys, "rows cut by row_count", rows=[1, 2, 3, 6, 7, 8], row_count=4); same("row_count 4")
    _insert(torch, dev, orc, keys, "row_count 0", rows=[9, 10, 12], row_count=0); same("row_count 0")
    _insert(torch, dev, orc, keys, "row_count 0 without rows", row_count=0); same("row_count 0")
    _find(torch, dev, orc, keys, "find behind the row lists"); same("find")
    # evictions, promotions and ghost re-admissions: every key of a universe of 4 x capacity goes in, finds in between raise
    # frequencies, and the early keys come back while their ghosts are still there
    for lo in range(0, len(universe), 40):
        batch = universe[lo: lo + 40]
        _insert(torch, dev, orc, batch, f"fill {lo}"); same("fill")
        probe = rng.choice(universe[: lo + 40], size=min(24, lo + 40), replace=False)
        _find(torch, dev, orc, probe, f"probe {lo}"); same("probe")
    again = rng.choice(universe, size=3 * max_size // 2, replace=False)
    for lo in range(0, len(again), 33):
        rows = rng.permutation(len(again[lo: lo + 33]))
        _insert(torch, dev, orc, again[lo: lo + 33], f"again {lo}", rows=rows); same("again")
        _find(torch, dev, orc, again[lo: lo + 33], f"find again {lo}"); same("find again")
    st = orc.stats()
    assert st["evictions"] > max_size and st["reinserts"] > 0 and st["hits"] > 0


def test_insert_rows_across_the_chunk_boundary(az, torch, oracle):
    """kApplyMax + 1 rows in one call: two launches, the second with one element, and shards that recur on both sides"""
    max_size, shards = 16384, 256
    ghost = max_size * 9 // 10
    dev = az.ShardedS3FIFOCache(max_size, shards, ghost, 7, 3)
    orc = oracle.Cache(max_size, shards, ghost, 7, 3)
    n = K_APPLY_MAX + 1
    keys = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(shards) + np.uint64(5)) % np.uint64(1 << 40)      # most of them in shard 5 ...
    keys[::3] = np.arange(1, n + 1, dtype=np.uint64)[::3] * np.uint64(7919)                                     # ... the rest spread
    keys[-1] = keys[-2] + np.uint64(shards)       # the element behind the boundary falls into the shard of the one in front of it
    keys[-3] = keys[7]                            # and a key of the first chunk comes again just before it
    assert int(keys[-1]) % shards == int(keys[-2]) % shards
    p, v = _pv(keys)
    dev.insert_many(_dev_keys(torch, keys), torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda())
    for j in range(n):
        orc.insert(int(keys[j]), p[j], v[j])
    assert _stats(torch, dev) == orc.stats()
    uniq = np.unique(keys)
    hit, gp, gv = dev.find_many(uniq)             # the numpy entry point, pinned to the oracle by tests/test_gpu_cache.py
    for i, k in enumerate(uniq):
        want = orc.find(int(k))
        assert bool(hit[i]) == (want is not None), int(k)
        if want is not None:
            assert np.array_equal(gp[i], want[0]) and np.array_equal(gv[i], want[1])
    assert _stats(torch, dev) == orc.stats()


def test_wide_rows_take_the_row_copy(az, torch, oracle):
    """num_policy = 130 > 64: no row fits one load per lane (wave_copy_row)"""
    dev = az.ShardedS3FIFOCache(128, 2, 100, 130, 4)
    orc = oracle.Cache(128, 2, 100, 130, 4)
    keys = np.arange(1, 11, dtype=np.uint64) * np.uint64(0x51ED27)
    p, v = _pv(keys, 130, 4)
    dev.insert_many(_dev_keys(torch, keys), torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda(),
                    rows=torch.tensor([9, 8, 7, 6, 5, 4, 3, 2, 1, 0], dtype=torch.int32, device="cuda"))
    for j in range(9, -1, -1):
        orc.insert(int(keys[j]), p[j], v[j])
    _find(torch, dev, orc, keys, "wide rows", 130, 4)
    assert _stats(torch, dev) == orc.stats()
    hit, gp, gv = dev.find_many(keys)
    assert hit.all() and np.array_equal(gp, p) and np.array_equal(gv, v)


@pytest.mark.parametrize("n", [4096, 4001])
def test_miss_rows_are_the_absent_rows_in_ascending_order(az, torch, n):
    dev = az.ShardedS3FIFOCache.for_engine(1 << 14, 7, 3)
    keys = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B1)
    present = np.arange(n) % 3 == 0
    p, v = _pv(keys[present])
    dev.insert_many(keys[present], p, v)          # the numpy entry point
    dk = _dev_keys(torch, keys)
    for run in range(2):
        hit, _, _, rows, count = dev.find_rows(dk)
        hit, rows, count = hit.cpu().numpy(), rows.cpu().numpy(), int(count.cpu()[0])
        assert np.array_equal(hit, present), run
        assert count == int((~present).sum()) and np.array_equal(rows[:count], np.flatnonzero(~present)), run


# ---- cached_forward ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c4(az, torch):
    """the Connect4 ResNet tile at depth 1, 192 sparse positions and net.forward's answers for them (the reference of every check)"""
    from alphazero import torch_net
    import leafnet_ref as lr
    spec = dataclasses.replace(torch_net.connect4_spec(depth=1), v_fc_hidden=16)
    net = az.HipLeafNet(torch_net.random_init(spec, seed=23), spec)
    x = lr.sparse_planes(spec, 192, seed=4).cuda().contiguous()
    v = torch.empty((192, 3), device="cuda"); pi = torch.empty((192, 7), device="cuda")
    net.forward(x, v, pi)
    torch.cuda.synchronize()
    keys = torch.from_numpy((np.arange(1, 193, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03)).view(np.int64)).cuda()
    return dict(net=net, x=x, v=v, pi=pi, keys=keys)


def _cached_forward_sequence(az, torch, c4, stream):
    net, x, v, pi, keys = c4["net"], c4["x"], c4["v"], c4["pi"], c4["keys"]
    cache = az.ShardedS3FIFOCache.for_engine(1 << 12, 7, 3)
    first = torch.arange(64, device="cuda")
    gv, gpi, hit = az.cached_forward(net, cache, x[:64], keys[:64], stream=stream)
    st = _stats(torch, cache)
    assert not bool(hit.any()) and torch.equal(gv, v[:64]) and torch.equal(gpi, pi[:64])
    assert (st["hits"], st["misses"], st["size"]) == (0, 64, 64)
    gv, gpi, hit = az.cached_forward(net, cache, x[:64], keys[:64], stream=stream)
    st = _stats(torch, cache)
    assert bool(hit.all()) and torch.equal(gv, v[:64]) and torch.equal(gpi, pi[:64])
    assert (st["hits"], st["misses"], st["size"]) == (64, 64, 64)
    # half old, half new, one of the new keys twice: rows 32 .. 62 are new, row 63 repeats row 40
    idx = torch.cat([first[:32], torch.arange(100, 131, device="cuda"), torch.tensor([108], device="cuda")])
    vo = torch.full((64, 3), SENTINEL, device="cuda"); po = torch.full((64, 7), SENTINEL, device="cuda")
    gv, gpi, hit = az.cached_forward(net, cache, x[idx].contiguous(), keys[idx].contiguous(), v_out=vo, pi_out=po, stream=stream)
    st = _stats(torch, cache)
    assert gv is vo and gpi is po
    assert hit.cpu().tolist() == [True] * 32 + [False] * 32
    assert torch.equal(gv, v[idx]) and torch.equal(gpi, pi[idx])
    assert (st["hits"], st["misses"], st["size"]) == (96, 96, 64 + 31)
    return cache


def test_cached_forward_returns_the_nets_bits(az, torch, c4):
    _cached_forward_sequence(az, torch, c4, None)


def test_cached_forward_on_another_stream(az, torch, c4):
    net, x, v, pi = c4["net"], c4["x"], c4["v"], c4["pi"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    before_v = torch.empty((192, 3), device="cuda"); before_pi = torch.empty((192, 7), device="cuda")
    after_v = torch.empty((192, 3), device="cuda"); after_pi = torch.empty((192, 7), device="cuda")
    with torch.cuda.stream(s):
        net.forward(x, before_v, before_pi, stream=s.cuda_stream)
        _cached_forward_sequence(az, torch, c4, s)
        net.forward(x, after_v, after_pi, stream=s.cuda_stream)
    s.synchronize()
    assert torch.equal(before_v, v) and torch.equal(before_pi, pi) and torch.equal(after_v, v) and torch.equal(after_pi, pi)


# ---- the step API with a cache ---------------------------------------------------------------------------------------------------------
def _c4_states(az, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        gs = az.Connect4GS()
        for _ in range(int(rng.integers(0, 7))):      # (six plies cannot end a game)
            gs.play_move(int(rng.choice(np.flatnonzero(np.asarray(gs.valid_moves())))))
        out.append(gs)
    return out


def test_step_api_with_cached_forward_is_the_search(az, torch, c4):
    net = c4["net"]
    n, visits = 16, 24
    states = _c4_states(az, n, seed=8)
    assert all(g.scores() is None for g in states)
    seeds = [700 + i for i in range(n)]
    twin = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=visits, seeds=seeds)
    twin.reset(states)
    twin.search(visits, net=net)
    want = twin.counts()
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=visits, seeds=seeds)
    mb.reset(states)
    with pytest.raises(RuntimeError, match="leaf_keys"):
        mb.leaf_keys()
    cache = az.ShardedS3FIFOCache.for_engine(1 << 12, 7, 3)
    alone = [az.MCTS(1.25, 2, 7, seed=seeds[t], max_simulations=visits) for t in range(n)]      # the host's view of the first steps
    for step in range(visits):
        canonical, tree = mb.find_leaves()
        keys = mb.leaf_keys()
        assert keys.shape[0] == canonical.shape[0]
        v, pi, hit = az.cached_forward(net, cache, canonical, keys)
        if step < 3:      # the leaves rebuilt on the host: stand-alone trees fed the rows the batch was answered with
            torch.cuda.synchronize()
            rows = {int(t): r for r, t in enumerate(tree.cpu().numpy())}
            hk, hv, hpi = keys.cpu().numpy().view(np.uint64), v.cpu().numpy(), pi.cpu().numpy()
            for t in range(n):
                leaf = alone[t].find_leaf(states[t])
                if leaf.scores() is None:
                    assert t in rows and int(hk[rows[t]]) == int(az.hash_game_state(leaf)), (step, t)
                    alone[t].process_result(states[t], hv[rows[t]], hpi[rows[t]])
                else:
                    assert t not in rows, (step, t)
                    alone[t].process_result(states[t], np.full(3, 1 / 3, np.float32), np.full(7, 1 / 7, np.float32))
        mb.process_results(v, pi)
    assert np.array_equal(mb.counts(), want)
    torch.cuda.synchronize()
    assert cache.hits() > 0 and cache.misses() > 0
    with pytest.raises(RuntimeError, match="leaf_keys"):
        mb.leaf_keys()


# ---- refusals, all before any launch ---------------------------------------------------------------------------------------------------
def test_refusals_name_their_argument_and_leave_the_cache_alone(az, torch, c4):
    net, x, keys = c4["net"], c4["x"], c4["keys"]
    cache = az.ShardedS3FIFOCache.for_engine(1 << 10, 7, 3)
    k8 = keys[:8].contiguous()
    p = torch.rand((8, 7), device="cuda"); v = torch.rand((8, 3), device="cuda")
    cache.insert_many(k8, p, v)
    before = _stats(torch, cache)
    with pytest.raises(RuntimeError, match="cache"):                      # a cache of another shape than the net's answers
        az.cached_forward(net, az.ShardedS3FIFOCache.for_engine(1 << 10, 9, 3), x[:8], k8)
    with pytest.raises(RuntimeError, match="policies"):                   # host keys with a device payload
        cache.insert_many(k8.cpu().numpy().view(np.uint64), p, v.cpu().numpy())
    with pytest.raises(RuntimeError, match="values"):                     # device keys with a host payload
        cache.insert_many(k8, p, v.cpu().numpy())
    with pytest.raises(RuntimeError, match="policies"):                   # float64 payload
        cache.insert_many(k8, p.double(), v)
    with pytest.raises(RuntimeError, match="keys"):                       # non-contiguous keys
        cache.find_rows(keys[:16:2])
    with pytest.raises(RuntimeError, match="hashes"):
        cache.find_many(keys[:16:2])
    with pytest.raises(RuntimeError, match="keys"):
        az.cached_forward(net, cache, x[:8], keys[:16:2])
    with pytest.raises(RuntimeError, match="canonical"):                  # rows that do not match the keys
        az.cached_forward(net, cache, x[:7], k8)
    with pytest.raises(RuntimeError, match="rows"):                       # a float row list
        cache.insert_many(k8, p, v, rows=torch.zeros(3, device="cuda"))
    with pytest.raises(RuntimeError, match="values"):                     # a payload of another width
        cache.insert_many(k8, p, p)
    mb = az.MCTSBatch(az.Connect4GS, 2, 1.25, max_simulations=4)
    mb.reset([az.Connect4GS(), az.Connect4GS()])
    with pytest.raises(RuntimeError, match="leaf_keys"):
        mb.leaf_keys()
    assert _stats(torch, cache) == before
