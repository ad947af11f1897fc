"""-m gpu: the device S3-FIFO cache where tests/test_gpu_cache.py does not reach - insert batches of 1 .. 2 * 8192 + 1 elements with
chosen shard patterns and duplicates (cache_apply_batch: owner election, 64-element chunks, host chunks of kApplyMax), rows of
1 .. 2662 floats (wave_copy_row, the 8-lane read-out), key words that share or lack a 32-bit half, hash 0, repeated keys in one
find batch, ghost rings longer than a shard, wave_shard_find<64> (azmi_debug_cache_find_group) and the pipeline's locked insert
on its own (azmi_debug_cache_insert_locked).  Everything is exact comparison with the oracle's restatement of s3fifo_cache.h, op
by op; the payload is a pure function of the key, so a hit can also be checked without the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_STAT_KEYS = ("hits", "misses", "evictions", "reinserts", "size", "max_size")


def _mix(x):
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _rows(keys, np_=7, nv=3):
    """(policy [n, np_], value [n, nv]) float32: entry j of a key's row is (24 bits of a 64-bit mix of key and j, + 1) / 2^24 - in
    (0, 1], never zero (a miss returns zero rows), never NaN, exact in float32."""
    k = np.ascontiguousarray(keys, np.uint64).reshape(-1, 1)
    cols = np.arange(np_ + nv, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):
        x = _mix(_mix(k) + (cols + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
    r = (((x >> np.uint64(40)).astype(np.float32) + np.float32(1.0)) / np.float32(1 << 24)).astype(np.float32)
    return np.ascontiguousarray(r[:, :np_]), np.ascontiguousarray(r[:, np_:])


def _dev_stats(dev):
    st = dev._stats()
    st["max_size"] = dev.max_size()
    return st


class _Pair:
    """the device cache and the oracle, driven together; every op ends with the comparison of all six counters"""

    def __init__(self, az, oracle, cfg, np_=7, nv=3, find=None, insert=None):
        self.dev = az.ShardedS3FIFOCache(cfg[0], cfg[1], cfg[2], np_, nv)
        self.orc = oracle.Cache(cfg[0], cfg[1], cfg[2], np_, nv)
        self.np_, self.nv, self.cfg, self.ops = np_, nv, cfg, 0
        self._find = find or self.dev.find_many
        self._insert = insert or self.dev.insert_many

    def check_stats(self, what):
        got, want = _dev_stats(self.dev), self.orc.stats()
        assert got == want, (self.cfg, self.ops, what, got, want)
        self.ops += 1

    def insert(self, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        pol, val = _rows(keys, self.np_, self.nv)
        self._insert(keys, pol, val)
        for k, p, v in zip(keys.tolist(), pol, val):
            self.orc.insert(k, p, v)
        self.check_stats(("insert", len(keys)))

    def find(self, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        hit, p, v = self._find(keys)
        pol, val = _rows(keys, self.np_, self.nv)
        want = np.zeros(len(keys), bool)
        for i, k in enumerate(keys.tolist()):
            w = self.orc.find(k)
            want[i] = w is not None
            if w is not None:
                assert np.array_equal(w[0], pol[i]) and np.array_equal(w[1], val[i])      # (the oracle holds what was put in)
        assert np.array_equal(hit, want), (self.cfg, self.ops, np.flatnonzero(hit != want)[:8], keys[hit != want][:8])
        pol[~want] = 0; val[~want] = 0                                                    # a miss leaves its rows zero
        assert np.array_equal(p, pol), (self.cfg, self.ops, "policy rows", np.argwhere(p != pol)[:8])
        assert np.array_equal(v, val), (self.cfg, self.ops, "value rows", np.argwhere(v != val)[:8])
        self.check_stats(("find", len(keys)))
        return want


def _interleave(pair, universe, rng, steps, max_insert=12, max_find=12):
    """test_gpu_cache.py's random interleaving: insert batches with repeats, find batches of distinct keys"""
    for _ in range(steps):
        if rng.random() < 0.5:
            pair.insert(rng.choice(universe, size=rng.integers(1, max_insert + 1)))
        else:
            pair.find(rng.choice(universe, size=min(len(universe), rng.integers(1, max_find + 1)), replace=False))


# ---- batch shapes ---------------------------------------------------------------------------------------------------------------
_Q = 192          # keys per shard in play: three times a 64-entry shard


def _keys(q, r, shards):
    return np.asarray(q, np.uint64) * np.uint64(shards) + np.asarray(r, np.uint64)


def _batch(kind, n, shards, rng):
    """n keys q * shards + r (shard r); q in [1, _Q]"""
    q = rng.integers(1, _Q + 1, size=n)
    if kind == "one_shard":          # the owner is wave 0 and applies the whole batch in order; the shard evicts throughout
        return _keys(q, np.full(n, rng.integers(0, shards)), shards)
    if kind == "random":
        return _keys(q, rng.integers(0, shards, size=n), shards)
    if kind == "sparse":             # more shards than elements: every element in a shard of its own
        return _keys(q, rng.choice(shards, size=n, replace=False), shards)
    if kind == "late_owner":         # shard b first appears at index 70 (outside the first 64-element chunk), shard c at index 300
        a, b, c = rng.choice(shards, size=3, replace=False)      # (outside the first block's four elements, beyond 256)
        r = np.full(n, a)
        r[70:300] = rng.choice([a, b], size=len(r[70:300])); r[70] = b
        rest = np.asarray([s for s in range(shards) if s not in (a, b)])
        r[300:] = rng.choice(np.concatenate([rest, [a, b]]), size=len(r[300:])); r[300] = c
        assert not np.any(r[:70] == b) and not np.any(np.isin(r[:300], rest))
        return _keys(q, r, shards)
    assert kind == "dups"            # the same key twice: adjacent, 70 and 64 apart, and on both sides of every 8192 boundary
    keys = _keys(q, rng.integers(0, shards, size=n), shards)
    if n >= 2:
        keys[1] = keys[0]
        keys[n - 1] = keys[n - 2]
    if n > 140:
        keys[70] = keys[0]; keys[134] = keys[70]; keys[n - 1] = keys[n - 71]
    for edge in range(8192, n, 8192):
        keys[edge] = keys[edge - 1]                       # adjacent across the host's chunk boundary
        if edge + 5 < n:
            keys[edge + 5] = keys[edge - 100]
    return keys


def _batch_plan(shards):
    plan = []
    for n in (1, 4, 5, 63, 64, 65, 255, 256, 257):
        kinds = ["one_shard", "random", "dups"]
        if n < shards:
            kinds.append("sparse")
        plan += [(n, k) for k in kinds]
    plan += [(8191, "one_shard"), (8191, "random"), (8192, "dups"), (8193, "dups"), (8193, "one_shard"),
             (2 * 8192 + 1, "dups"), (2 * 8192 + 1, "one_shard")]
    if shards >= 3:
        plan += [(n, "late_owner") for n in (301, 8192, 2 * 8192 + 1)]
    return plan


@pytest.mark.parametrize("cfg", [(64, 1, 57), (192, 3, 171), (4096, 64, 3648), (48, 3, 40)])      # the last: generic tables
def test_insert_batch_shapes_match_oracle_op_by_op(oracle, cfg):
    """cache_apply_batch from 1 to 2 * kApplyMax + 1 elements.  The 301-element late_owner batch has its owners in the second
    chunk / beyond the first 64 blocks; the large ones run 32 KB of shard ids and the host's chunking."""
    import alphazero as az
    shards = cfg[1]
    pair = _Pair(az, oracle, cfg)
    rng = np.random.default_rng(cfg[0] * 7 + shards)
    absent = _keys(np.arange(10 * _Q, 10 * _Q + 64), rng.integers(0, shards, size=64), shards)      # never inserted
    hits = misses = 0
    for n, kind in _batch_plan(shards):
        keys = _batch(kind, n, shards, rng)
        pair.insert(keys)
        uniq = np.unique(keys)
        sample = np.concatenate([rng.choice(uniq, size=min(len(uniq), 48), replace=False), rng.choice(absent, size=8, replace=False)])
        found = pair.find(rng.permutation(sample))
        hits += int(found.sum()); misses += int((~found).sum())
    st = pair.orc.stats()
    assert st["evictions"] > 0 and st["reinserts"] > 0 and hits > 0 and misses > 0, st      # a condition on the inputs


# ---- row widths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(128, 2, 114), (16, 1, 14)])
@pytest.mark.parametrize("np_,nv", [(1, 1), (63, 3), (64, 64), (65, 3), (7, 65), (2048, 3), (2049, 3), (2662, 3)])
def test_row_widths_match_oracle_op_by_op(oracle, cfg, np_, nv):
    """np, nv <= 64: a wavefront's own row travels in registers; wider rows go through wave_copy_row<32> - one trip up to 2048
    floats, two for 2049 and Tawlbwrdd's 2662 - and come back through the 8-lane read-out."""
    import alphazero as az
    pair = _Pair(az, oracle, cfg, np_, nv)
    rng = np.random.default_rng(np_ * 100 + nv + cfg[0])
    universe = rng.integers(1, 2 ** 63, size=3 * cfg[0], dtype=np.uint64)
    _interleave(pair, universe, rng, 40, max_insert=70, max_find=70)
    st = pair.orc.stats()
    assert st["evictions"] > 0 and st["hits"] > 0 and st["misses"] > 0, st


# ---- key words ------------------------------------------------------------------------------------------------------------------
def _key_word_universe(max_size, rng):
    """keys a wave shard's two 32-bit halves can confuse; without 0x9E3779B97F4A7C15 (hash 0's stand-in, dev_cache.h)"""
    keys = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
    keys += [int(h) << 32 for h in rng.integers(1, 2 ** 32, size=4)]                  # zero low word
    keys += [int(l) for l in rng.integers(2, 2 ** 32 - 1, size=4)]                    # zero high word
    for _ in range(8):
        lo, h1, h2 = (int(x) for x in rng.integers(1, 2 ** 31, size=3))
        assert len({lo, h1, h2}) == 3
        keys += [(h1 << 32) | lo, ((h2 | 0x80000000) << 32) | lo]                     # equal low words
        keys += [(h1 << 32) | h2, (h1 << 32) | lo | 0x80000000]                       # equal high words
    keys += [int(x) for x in rng.integers(1, 2 ** 63, size=max(0, 3 * max_size - len(keys)), dtype=np.uint64)]
    keys = np.unique(np.asarray(keys, np.uint64))
    assert 0x9E3779B97F4A7C15 not in keys.tolist() and len(keys) >= 3 * max_size - 2
    return keys


def _finder(az, pair_dev, lanes):
    return None if lanes is None else (lambda keys: az.cache_find_group(pair_dev, lanes, keys))


_KEY_WORD_CASES = [((64, 1, 57), None), ((64, 1, 57), 8), ((64, 1, 57), 64), ((16, 1, 14), None), ((192, 3, 171), None), ((192, 3, 171), 64)]


@pytest.mark.parametrize("cfg,lanes", _KEY_WORD_CASES)
def test_key_words_match_oracle_op_by_op(oracle, cfg, lanes):
    """A wave shard matches a key on both 32-bit halves: keys that agree in one half, keys with a zero half, bit 63, all ones,
    and hash 0.  lanes: the finds go through wave_shard_find<lanes> (None: the stand-alone find)."""
    import alphazero as az
    pair = _Pair(az, oracle, cfg)
    if lanes is not None:
        pair._find = _finder(az, pair.dev, lanes)
    rng = np.random.default_rng(cfg[0] + 17 * cfg[1])
    universe = _key_word_universe(cfg[0], rng)
    pair.insert(universe[rng.permutation(len(universe))[: cfg[0] // 2]])
    _interleave(pair, universe, rng, 200)
    # the whole universe in one find batch, then in one insert batch, then again: every special key has been on both sides
    pair.find(universe)
    pair.insert(rng.permutation(universe))
    pair.find(universe)
    st = pair.orc.stats()
    assert st["evictions"] > 0 and st["reinserts"] > 0, st


@pytest.mark.parametrize("cfg", [(64, 1, 57), (16, 1, 14), (192, 3, 171)])
def test_hash_zero_is_a_key_like_any_other(oracle, cfg):
    """hash 0 is inserted, found, evicted into the ghost ring, counted as a reinsert and re-admitted, as in the reference (the
    engines' batches use key 0 for "nothing to insert"; the stand-alone cache does not)."""
    import alphazero as az
    pair = _Pair(az, oracle, cfg)
    shards, cap = cfg[1], cfg[0] // cfg[1]
    zero = np.zeros(1, np.uint64)
    assert not pair.find(zero)[0]
    pair.insert(np.asarray([0, 0, shards, 0], np.uint64))
    assert pair.find(np.asarray([shards], np.uint64))[0] and pair.orc.stats()["size"] == 2
    # never found: a scan through shard 0 pushes it out of Small into the ghost ring; a miss there is a reinsert
    pair.insert(np.arange(2, 2 + cap, dtype=np.uint64) * np.uint64(shards))
    before = pair.orc.stats()["reinserts"]
    assert not pair.find(zero)[0], "the inputs must evict key 0"
    assert pair.orc.stats()["reinserts"] == before + 1, "the inputs must leave key 0 in the ghost ring"
    # the next insert admits it to Main, where a scan through Small does not reach it
    pair.insert(zero)
    assert pair.find(zero)[0]
    pair.insert(np.arange(1000, 1000 + 3 * cap, dtype=np.uint64) * np.uint64(shards))
    assert pair.find(np.asarray([0, shards, 2 * shards], np.uint64))[0], "the inputs must keep key 0 in Main"


# ---- repeated keys in one find batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(64, 1, 57), (16, 1, 14)])
def test_repeated_keys_in_one_find_batch(oracle, cfg):
    """Concurrent finds of one key: freq = min(freq + count, 3) and the serial hit / miss / reinsert counts, whatever the order.
    The insert batches that follow evict, so the frequencies decide who survives - which the next finds compare."""
    import alphazero as az
    pair = _Pair(az, oracle, cfg)
    rng = np.random.default_rng(cfg[0] + 5)
    universe = rng.integers(1, 2 ** 63, size=3 * cfg[0], dtype=np.uint64)
    for _ in range(30):
        pair.insert(rng.choice(universe, size=rng.integers(cfg[0] // 4, cfg[0] + 1)))
        distinct = rng.choice(universe, size=rng.integers(1, min(58, len(universe) + 1)), replace=False)
        keys = np.repeat(distinct, rng.integers(1, 7, size=len(distinct)))[:200]
        pair.find(rng.permutation(keys))
    st = pair.orc.stats()
    assert st["evictions"] > 0 and st["reinserts"] > 0 and st["hits"] > 0, st


# ---- ghost rings longer than a shard ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(64, 1, 65), (64, 1, 100), (128, 2, 400), (16, 1, 40)])
def test_ghost_larger_than_the_shard(oracle, cfg):
    """ghost_size / shards > 64 on 64-entry shards: a wave shard has one ghost-ring entry per lane, so such a cache runs on the
    generic kernels (and is no engine cache: test_engines_refuse_a_ghost_ring_longer_than_a_wave_shard)."""
    import alphazero as az
    pair = _Pair(az, oracle, cfg)
    rng = np.random.default_rng(cfg[0] + cfg[2])
    universe = rng.integers(1, 2 ** 63, size=3 * max(cfg[0], cfg[2]), dtype=np.uint64)
    _interleave(pair, universe, rng, 300, max_insert=40)
    st = pair.orc.stats()
    assert st["evictions"] >= 2 * cfg[2] and st["reinserts"] > 0, st      # the ghost ring wrapped


def _c4_params(az):
    pp = az.PlayParams()
    pp.games_to_play, pp.concurrent_games, pp.max_batch_size = 4, 4, 4
    pp.model_groups = [0, 1]
    pp.mcts_visits = [10, 10]
    pp.eval_type = [az.EvalType.RANDOM, az.EvalType.RANDOM]
    return pp


@pytest.fixture(scope="module")
def c4_net():
    """MCTSBatch looks at a cache only beside a net (the first net of a process also pays for importing torch)"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    return az.HipLeafNet(torch_net.random_init(spec, seed=3), spec)


def test_engines_refuse_a_ghost_ring_longer_than_a_wave_shard(c4_net):
    import alphazero as az
    # an unused cache is re-created in the engine's layout with the ghost ring clamped to the cache
    c = az.ShardedS3FIFOCache(64, 1, 100, 7, 3)
    c._ensure_engine_layout()
    assert c._args[:3] == (64, 1, 64) and c.max_size() == 64
    pm = az.PlayManager(az.Connect4GS(), _c4_params(az), caches=[az.ShardedS3FIFOCache(128, 2, 400, 7, 3), None], seed=3)
    pm.play()
    assert pm.games_completed() == 4
    # a used one cannot be converted
    used = az.ShardedS3FIFOCache(64, 1, 100, 7, 3)
    used.insert(5, np.zeros(7, np.float32), np.zeros(3, np.float32))
    with pytest.raises(RuntimeError, match="ghost_size / shards > 64"):
        az.PlayManager(az.Connect4GS(), _c4_params(az), caches=[used, None])
    # and the C ABI refuses it by itself
    used._ensure_engine_layout = lambda: None
    with pytest.raises(RuntimeError, match=r"caches\[0\]: ghost_size / shards = 100, but a 64-entry wave shard keeps at most 64 ghost keys"):
        az.PlayManager(az.Connect4GS(), _c4_params(az), caches=[used, None])
    mb = az.MCTSBatch(az.Connect4GS, 2, 1.25, max_simulations=8, seeds=[1, 2])
    mb.reset([az.Connect4GS(), az.Connect4GS()])
    with pytest.raises(RuntimeError, match="cache: ghost_size / shards = 100, but a 64-entry wave shard keeps at most 64 ghost keys"):
        mb.search(4, net=c4_net, cache=used)


# ---- the lane groups of the engines' probe ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(64, 1, 57), (256, 4, 228), (640, 10, 570)])
@pytest.mark.parametrize("lanes", [8, 64])
def test_find_group_matches_oracle_op_by_op(oracle, cfg, lanes):
    """test_gpu_cache.py's interleaving with the finds through wave_shard_find<lanes>: 8 = the DPP reduction the stand-alone find
    uses, 64 = the __shfl_xor reduction of the one-wavefront-per-slot games."""
    import alphazero as az
    pair = _Pair(az, oracle, cfg)
    pair._find = _finder(az, pair.dev, lanes)
    rng = np.random.default_rng(cfg[0] * 1000 + cfg[1])
    universe = rng.integers(1, 2 ** 63, size=3 * cfg[0] + 8, dtype=np.uint64)
    _interleave(pair, universe, rng, 200)
    pair.find(universe)                                      # one batch larger than a block of either group size
    st = pair.orc.stats()
    assert st["evictions"] > 0 and st["reinserts"] > 0 and st["hits"] > 0, st


def test_debug_entry_points_refuse_what_they_do_not_cover():
    import alphazero as az
    keys = np.arange(1, 5, dtype=np.uint64)
    pol, val = _rows(keys)
    generic = az.ShardedS3FIFOCache(48, 3, 40, 7, 3)
    long_ghost = az.ShardedS3FIFOCache(64, 1, 100, 7, 3)
    for c, caps in ((generic, "max_size / shards = 16, ghost_size / shards = 13"), (long_ghost, "max_size / shards = 64, ghost_size / shards = 100")):
        with pytest.raises(RuntimeError, match=f"azmi_debug_cache_find_group: not a cache of 64-entry wave shards \\({caps}\\)"):
            az.cache_find_group(c, 8, keys)
        with pytest.raises(RuntimeError, match=f"azmi_debug_cache_insert_locked: not a cache of 64-entry wave shards \\({caps}\\)"):
            az.cache_insert_locked(c, keys, pol, val, 4)
    wave = az.ShardedS3FIFOCache(128, 2, 114, 7, 3)
    for lanes in (0, 1, 16, 32, 128):
        with pytest.raises(RuntimeError, match=f"group_lanes {lanes} is not a lane group of the engines \\(8 or 64\\)"):
            az.cache_find_group(wave, lanes, keys)
    for waves in (0, 8193):
        with pytest.raises(RuntimeError, match="waves must be 1 .. 8192"):
            az.cache_insert_locked(wave, keys, pol, val, waves)
    for np_, nv in ((65, 3), (7, 65)):
        wide = az.ShardedS3FIFOCache(128, 2, 114, np_, nv)
        p, v = _rows(keys, np_, nv)
        with pytest.raises(RuntimeError, match=f"num_policy and num_value must be <= 64 \\({np_}, {nv}\\)"):
            az.cache_insert_locked(wide, keys, p, v, 4)
    assert az.cache_insert_locked(wave, keys[:0], pol[:0], val[:0], 4) == 0
    assert _dev_stats(wave) == dict(hits=0, misses=0, evictions=0, reinserts=0, size=0, max_size=128)


# ---- the pipeline's locked insert ---------------------------------------------------------------------------------------------------
def test_locked_insert_one_wavefront_matches_oracle_op_by_op(oracle):
    """waves = 1: the entries go in in batch order, so wave_shard_insert_locked must be S3FIFOCache::insert op by op - repeats
    inside a batch, batches that overflow both shards, finds in between."""
    import alphazero as az
    cfg = (128, 2, 114)
    pair = _Pair(az, oracle, cfg)
    failed = []
    pair._insert = lambda keys, pol, val: failed.append(az.cache_insert_locked(pair.dev, keys, pol, val, 1))
    rng = np.random.default_rng(11)
    universe = rng.integers(1, 2 ** 63, size=3 * cfg[0], dtype=np.uint64)
    _interleave(pair, universe, rng, 120, max_insert=24)
    big = rng.choice(universe, size=300)                     # more than both shards hold, with repeats
    big[1] = big[0]; big[200] = big[3]
    pair.insert(big)
    pair.find(universe)
    pair.insert(rng.permutation(universe))
    pair.find(universe)
    st = pair.orc.stats()
    assert st["evictions"] > 0 and st["reinserts"] > 0 and st["hits"] > 0, st
    assert failed and not any(failed)


@pytest.mark.parametrize("cfg,per_shard,repeats,waves", [((512, 8, 456), 48, 4, 256), ((64, 1, 57), 64, 8, 512)])
def test_locked_insert_contended_without_eviction(cfg, per_shard, repeats, waves):
    """Many wavefronts on few shards, every key several times, nothing evicted: whatever the order, the cache ends up holding
    every distinct key once, with its row."""
    import alphazero as az
    shards = cfg[1]
    rng = np.random.default_rng(cfg[0])
    q = rng.integers(1, 1 << 40, size=per_shard * shards)
    distinct = _keys(q, np.repeat(np.arange(shards), per_shard), shards)
    keys = rng.permutation(np.repeat(distinct, repeats))
    assert len(keys) == per_shard * shards * repeats and len(np.unique(distinct)) == len(distinct)
    dev = az.ShardedS3FIFOCache(cfg[0], shards, cfg[2], 7, 3)
    pol, val = _rows(keys)
    assert az.cache_insert_locked(dev, keys, pol, val, waves) == 0
    assert _dev_stats(dev) == dict(hits=0, misses=0, evictions=0, reinserts=0, size=len(distinct), max_size=cfg[0])
    hit, p, v = dev.find_many(distinct)
    pol, val = _rows(distinct)
    assert hit.all() and np.array_equal(p, pol) and np.array_equal(v, val)
    assert _dev_stats(dev) == dict(hits=len(distinct), misses=0, evictions=0, reinserts=0, size=len(distinct), max_size=cfg[0])


def test_locked_insert_contended_with_eviction_then_serial_use():
    """256 distinct keys per 64-entry shard, each once, 256 wavefronts: every key is inserted once and nothing is found during
    the kernel, so every eviction leaves Small at frequency 0 into the ghost ring - 192 per shard in whatever order the lock was
    had, the ring keeping the last 57.  Then the cache is used serially: its state must be a valid S3-FIFO state."""
    import alphazero as az
    shards, per_shard = 4, 256
    rng = np.random.default_rng(4)
    q = rng.integers(1, 1 << 40, size=per_shard * shards)
    keys = rng.permutation(_keys(q, np.repeat(np.arange(shards), per_shard), shards))
    assert len(np.unique(keys)) == len(keys)
    dev = az.ShardedS3FIFOCache(256, shards, 228, 7, 3)
    pol, val = _rows(keys)
    assert az.cache_insert_locked(dev, keys, pol, val, 256) == 0
    assert _dev_stats(dev) == dict(hits=0, misses=0, evictions=768, reinserts=0, size=256, max_size=256)
    hit, p, v = dev.find_many(keys)
    assert np.bincount((keys % np.uint64(shards)).astype(np.int64)[hit], minlength=shards).tolist() == [64] * shards
    pol[~hit] = 0; val[~hit] = 0
    assert np.array_equal(p, pol) and np.array_equal(v, val)
    assert _dev_stats(dev) == dict(hits=256, misses=768, evictions=768, reinserts=4 * 57, size=256, max_size=256)
    # 50 serial steps on the state the contended kernel left
    for _ in range(50):
        if rng.random() < 0.5:
            ks = rng.choice(keys, size=rng.integers(1, 40))
            pol, val = _rows(ks)
            dev.insert_many(ks, pol, val)
        else:
            ks = rng.choice(keys, size=rng.integers(1, 40), replace=False)
            hit, p, v = dev.find_many(ks)
            pol, val = _rows(ks)
            pol[~hit] = 0; val[~hit] = 0
            assert np.array_equal(p, pol) and np.array_equal(v, val)
        assert dev.size() <= 256
    hit, p, v = dev.find_many(keys)
    pol, val = _rows(keys)
    pol[~hit] = 0; val[~hit] = 0
    assert np.array_equal(p, pol) and np.array_equal(v, val)
    assert int(hit.sum()) == dev.size()
