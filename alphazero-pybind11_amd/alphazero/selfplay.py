"""Device counterpart of the reference's self-play harness (GameRunner.run + the read-out of self_play(),
game_runner.py:392-747, 2057-2160): K engine shards on one GPU driven by the native round loop, the leaf net on the
matrix cores, finished samples left in HBM.

The reference spreads one PlayManager over `mcts_workers` threads and batcher threads; here the games are split over
K engines (contiguous slot ranges, distinct seeds) because four independent streams keep the GPU busy.
The results are the reference's: the multiset of (canonical, v, pi) rows and the counters self_play() reports."""
import dataclasses

import numpy as np

from . import (PlayManager, EvalType, ShardedS3FIFOCache, run_rounds, run_rounds_groups, run_pipeline, pipeline_supported, run_pipeline_groups,
               pipeline_supported_groups)


@dataclasses.dataclass
class SelfPlayResult:          # the fields of game_runner.SelfPlayResult that come from the PlayManager
    win_rates: list
    hit_rate: float
    game_length: float
    resign_win_rates: list
    resign_rate: float
    avg_leaf_depth: float
    avg_search_entropy: float
    fast_avg_leaf_depth: float
    fast_avg_search_entropy: float
    avg_moves_per_turn: float
    avg_valid_moves: float
    cache_saturation: float
    cache_churn: float
    games: int
    simulations: int
    leaf_evaluations: int
    samples: int
    # games with variants (StarGambitUnifiedGS; game_runner.py:2136-2145, 153-176): {variant id: ...}, empty otherwise
    variant_game_counts: dict = dataclasses.field(default_factory=dict)
    variant_win_rates: dict = dataclasses.field(default_factory=dict)
    variant_metrics: dict = dataclasses.field(default_factory=dict)
    # which driver played the games (a stall must show up as a failure or as a counted event, not as a slow run - VERDICT r5 item 7):
    # driver_used "pipeline" | "rounds" | "none" (no net); pipeline_retries = pipeline calls repeated after a recovered pipeline error;
    # fallbacks = 1 when driver="auto" gave the pipeline up in mid-run and the lock-step driver carried on
    driver_used: str = "rounds"
    pipeline_retries: int = 0
    fallbacks: int = 0


def _shard_params(params, k, K):
    import copy
    p = copy.copy(params)
    S, N = int(params.concurrent_games), int(params.games_to_play)
    lo, hi = S * k // K, S * (k + 1) // K
    p.concurrent_games = hi - lo
    p.games_to_play = N * (k + 1) // K - N * k // K        # contiguous game-index ranges
    p.max_batch_size = max(1, min(int(params.max_batch_size), p.concurrent_games))
    p.max_cache_size = int(params.max_cache_size) // K
    return p


def shard_seed(seed, k):
    """seed of engine shard k (bench.py uses the same rule)"""
    return int(seed) + 104729 * k


def self_play(game, params, net=None, engines=None, seed=20240601, device=0, streams=None, rounds_per_poll=512, data_folder=None,
              iteration=0, data_save_size=30_000, driver="auto", epochs_per_poll=16, max_fallbacks=None):
    """Runs `params.games_to_play` self-play games of `game`; `net` is a HipLeafNet (or None when every seat evaluates with
    RANDOM / PLAYOUT).  Returns (SelfPlayResult, (canonical, v, pi)) with the samples as device tensors in shard order (numpy
    arrays without a net, since nothing else needs torch then).  With `data_folder` the samples are also written as the
    reference's `.ptz` triples, `data_save_size` rows per batch (GameRunner.hist_saver, game_runner.py:736-747).
    driver: "pipeline" = ONE engine with every game on the asynchronous tree / net pipeline (azmi_run_pipeline: Connect4, PUCT or
    Gumbel seats, at most 16384 concurrent games), "rounds" = `engines` shards (default 4) on the lock-step round
    driver, "auto" = the pipeline where it applies.  The finished samples are taken out of the engines' rings at every poll
    (the ring is bounded: a long stream would overflow it), like the reference's hist_saver drains its queue.
    max_fallbacks: None = "auto" may fall back to the lock-step driver (counted in SelfPlayResult.fallbacks, with a warning); 0 = a run
    that would fall back raises instead (what a throughput measurement wants: a stall is a failure, not a slow run)."""
    want_pipe = driver in ("auto", "pipeline") and net is not None and (engines in (None, 1) or driver == "pipeline")
    if want_pipe:
        probe = PlayManager(game() if isinstance(game, type) else game, _shard_params(params, 0, 1), seed=shard_seed(seed, 0), device=device)
        if pipeline_supported(probe, net):
            pms, K = [probe], 1
        else:
            if driver == "pipeline":
                raise RuntimeError("self_play: the pipeline does not drive this engine / net (alphazero.pipeline_supported)")
            del probe
            want_pipe = False
    if not want_pipe:
        K = max(1, min(int(engines or 4), int(params.concurrent_games)))
        pms = [PlayManager(game() if isinstance(game, type) else game, _shard_params(params, k, K), seed=shard_seed(seed, k), device=device)
               for k in range(K)]
    no_net = bool(params.eval_type) and all(int(e) != int(EvalType.NN) for e in params.eval_type)
    drained = [[] for _ in range(K)]          # per shard: the sample rows taken out of its ring so far
    if no_net:
        for pm in pms:
            pm.play()
    else:
        if net is None:
            raise RuntimeError("self_play: seats with EvalType.NN need a net")
        import torch
        if streams is None:
            streams = [torch.cuda.Stream(device=device) for _ in range(K)]
        sps = [s.cuda_stream for s in streams]
        live = list(range(K))
        tdev = torch.device("cuda", device)
        spe = 256 * int(params.concurrent_games)
        pipe_state = {"retries": 0, "fallbacks": 0, "driver": "pipeline" if want_pipe else "rounds"}
        while live:
            group = [pms[i] for i in live]
            if want_pipe:
                # the pipeline's run-time preconditions (a second hardware queue beside the caller's stream, room for its tree and
                # net workgroups side by side) are only known once it runs: "auto" falls back to the lock-step driver - with fresh
                # shards while no game has finished, on the same engine otherwise (a pipeline error leaves the engine whole)
                if not _pipeline_step(lambda: run_pipeline(pms[0], net, epochs_per_poll, spe, sps[0]), pipe_state, driver, "self_play"):
                    want_pipe = False
                    pipe_state["fallbacks"] += 1; pipe_state["driver"] = "rounds"
                    if max_fallbacks is not None and pipe_state["fallbacks"] > int(max_fallbacks):
                        raise RuntimeError("self_play: the asynchronous pipeline gave up on this run and max_fallbacks=%d forbids the lock-step fallback" % int(max_fallbacks))
                    if pms[0].games_completed() == 0 and not drained[0]:
                        K = max(1, min(int(engines or 4), int(params.concurrent_games)))
                        pms = [PlayManager(game() if isinstance(game, type) else game, _shard_params(params, k, K), seed=shard_seed(seed, k), device=device)
                               for k in range(K)]
                        drained = [[] for _ in range(K)]
                        streams = [torch.cuda.Stream(device=device) for _ in range(K)]
                        sps = [s_.cuda_stream for s_ in streams]
                        live = list(range(K))
                    continue
            else:
                run_rounds(group, net, rounds_per_poll, [sps[i] for i in live])
            for i in live:
                if params.history_enabled:
                    drained[i].append(pms[i].take_history_device(tdev)[:3])
            live = [i for i in live if pms[i].poll(sps[i])[1] > 0]
    # ---- the read-out of self_play(), game_runner.py:2073-2145, combined over the shards from the raw sums
    P1 = pms[0]._P + 1
    scores = np.sum([pm.scores() for pm in pms], 0)
    resign = np.sum([pm.resign_scores() for pm in pms], 0)
    sums = {}
    for pm in pms:
        for k, v in pm.stat_sums().items():
            sums[k] = sums.get(k, 0.0) + v
    cs = np.sum([pm._cache_stats() for pm in pms], 0)
    cn = [pm.counters() for pm in pms]
    sn, rn = float(scores.sum()), float(resign.sum())
    hits, misses, evictions, reinserts, csize, cmax = (int(x) for x in cs)
    div = lambda a, b: (a / b) if b else 0.0
    if no_net:
        hist = [pm.history() for pm in pms]
        samples = tuple(np.concatenate([h[i] for h in hist], 0) for i in range(3))
        n_samples = samples[0].shape[0]
    else:
        import torch
        tdev = torch.device("cuda", device)
        for k in range(K):
            if params.history_enabled:
                drained[k].append(pms[k].take_history_device(tdev)[:3])          # what finished after the last poll
        hist = [tuple(torch.cat([part[i] for part in drained[k]], 0) for i in range(3)) if drained[k] else pms[k].history_device_tensors(tdev)[:3]
                for k in range(K)]
        samples = tuple(torch.cat([h[i] for h in hist], 0) for i in range(3))
        n_samples = int(samples[0].shape[0])
    res = SelfPlayResult(
        win_rates=[div(float(x), sn) for x in scores], hit_rate=div(hits, hits + misses), game_length=div(sums["game_length"], sums["games"]),
        resign_win_rates=[div(float(x), rn) for x in resign], resign_rate=div(rn, sn),
        avg_leaf_depth=div(sums["leaf_depth"], sums["full_moves"]), avg_search_entropy=div(sums["entropy"], sums["full_moves"]),
        fast_avg_leaf_depth=div(sums["fast_leaf_depth"], sums["fast_moves"]), fast_avg_search_entropy=div(sums["fast_entropy"], sums["fast_moves"]),
        avg_moves_per_turn=div(sums["moves"], sums["game_length"]), avg_valid_moves=div(sums["valid_moves"], sums["moves"]),
        cache_saturation=div(csize, cmax), cache_churn=div(evictions, hits), games=int(sums["games"]),
        simulations=sum(c["sims"] for c in cn), leaf_evaluations=sum(c["evals"] for c in cn), samples=n_samples)
    # per-variant read-out: the shards' raw sums (azmi_pm_variant_sums) added up, then the reference's own divisions
    for vid in range(pms[0].num_tracked_variants()):
        vs = dict(zip(PlayManager._SUM_KEYS, np.sum([pm.variant_sums(vid) for pm in pms], 0)))
        vscores = np.sum([pm.variant_scores(vid) for pm in pms], 0)
        res.variant_game_counts[vid] = int(vs["games"])
        if vs["games"] > 0:
            vn = float(vscores.sum())
            res.variant_win_rates[vid] = [div(float(x), vn) for x in vscores]
            res.variant_metrics[vid] = dict(game_length=div(vs["game_length"], vs["games"]), avg_depth=div(vs["leaf_depth"], vs["full_moves"]),
                                            avg_entropy=div(vs["entropy"], vs["full_moves"]), avg_mpt=div(vs["moves"], vs["game_length"]),
                                            avg_vm=div(vs["valid_moves"], vs["moves"]), fast_avg_depth=div(vs["fast_leaf_depth"], vs["fast_moves"]),
                                            fast_avg_entropy=div(vs["fast_entropy"], vs["fast_moves"]))
    if no_net:
        res.driver_used = "none"
    else:
        res.driver_used, res.pipeline_retries, res.fallbacks = pipe_state["driver"], pipe_state["retries"], pipe_state["fallbacks"]
    res._pms = pms                      # keeps the engines (and the device memory behind `samples`) alive
    if data_folder is not None and n_samples:
        from . import history_io
        import torch
        c, v, p = (torch.as_tensor(x) for x in samples)
        for b, lo in enumerate(range(0, n_samples, int(data_save_size))):
            hi = min(n_samples, lo + int(data_save_size))
            history_io.write_history_batch(data_folder, iteration, b, c[lo:hi], v[lo:hi], p[lo:hi])
    return res, samples


def process_samples(game, samples, net, seed, **kwargs):
    """The two stages between self_play and training (game_runner.py:4234-4239): exploit_symmetries (symmetries_batch, when the
    game has more than one symmetry), then resample_by_surprise with `net` and `seed`; the keywords are resample_by_surprise's.
    -> ((canonical, v, pi) resampled, loss), loss holding one entry per symmetry-expanded sample."""
    from .games import symmetries_batch
    from . import _args
    from .samples import resample_by_surprise, _check_samples
    cls = game if isinstance(game, type) else type(game)
    _check_samples("process_samples", samples, kwargs.get("batch_rows", 65536))      # the named errors, before symmetries_batch's own
    _args.seed64(seed, "process_samples")
    if cls.NUM_SYMMETRIES() > 1 and int(samples[0].shape[0]) > 0:
        samples = symmetries_batch(cls, *samples)
    return resample_by_surprise(samples, net, seed, **kwargs)


def training_batches(window, batch_rows, sample_rate=1.0, pass_seed=0):
    """The batches train() takes from the history window and the reservoir (game_runner.py:1289-1345): SampleWindow.batches of
    `window`, ceil(average_generation / batch_rows * sample_rate) (canonical, v, pi) CUDA batches cut from shuffled passes."""
    from .samples import SampleWindow
    if not isinstance(window, SampleWindow):
        raise RuntimeError(f"training_batches: window must be a SampleWindow, got {type(window).__name__}")
    return window.batches(batch_rows, sample_rate=sample_rate, pass_seed=pass_seed)


def refresh_net(hip, model, caches=(), stream=None):
    """The hand-off from training back to self-play (game_runner.py:2043-2051 loads the iteration's checkpoint): hip.refresh(model) -
    the trained LeafNet's weights written into the live HipLeafNet on the device, no new handle - and then clear() on every cache
    given: a position cache filled under the old weights serves stale answers (the reference builds a fresh cache per self_play
    call, game_runner.py:2013-2060).  ShardedS3FIFOCache has no clear(): a caller that keeps one across iterations builds a new one
    instead of passing it here, and an engine (PlayManager with max_cache_size > 0, MCTSBatch given a cache) that outlives the
    refresh keeps its own cache with the old answers in it: build the engine anew, as self_play does per call.  A cache without
    clear() is a TypeError before anything is refreshed.  Returns hip."""
    for c in caches:
        if not callable(getattr(c, "clear", None)):
            raise TypeError(f"refresh_net: {type(c).__name__} has no clear(); build a new cache after the refresh instead")
    hip.refresh(model, stream=stream)
    for c in caches:
        c.clear()
    return hip


def window_effective_rank(window, net, rows=512, seed=0):
    """The effective-rank diagnostic game_runner tracks after every iteration (game_runner.py:4462-4491: _sample_recent_history_batch,
    then NNWrapper.effective_rank; `effective_rank_enabled` with 512 positions by default): effective_rank of `net` (an fp32
    HipLeafNet) over up to `rows` positions of the newest iteration in `window` (a SampleWindow) - all of them when it holds no more,
    otherwise the first `rows` entries of the window's per-row permutation of that iteration keyed by (seed, pass 0), the rows
    window_batches([newest], rows, seed, batches=1) yields.  -> a float; NaN for an empty window or an empty iteration."""
    from . import _args
    from .samples import SampleWindow, effective_rank, _window_gather
    what = "window_effective_rank"
    if not isinstance(window, SampleWindow):
        raise RuntimeError(f"{what}: window must be a SampleWindow, got {type(window).__name__}")
    rows = _args.integer(rows, f"{what}: rows must be an integer in [1, 2^30], got {rows!r}", 1, 1 << 30)
    seed = _args.seed64(seed, what)
    newest = window.newest()
    if newest is None:
        return effective_rank(None, net)
    canonical = newest[1][0]
    n = int(canonical.shape[0])
    if n > rows:
        canonical = _window_gather([canonical], [n], None, seed, 0, 0, rows, None)
    return effective_rank(canonical, net)


UNIFIED_VARIANT_NAMES =("skirmish", "showdown", "clash", "battle")      # game_runner.py:37


def variant_buckets(game, canonical, **kwargs):
    """The variant of every sample of a unified StarGambit game, read from its canonical planes: (ids, names) with ids =
    plane_argmax(canonical, 32, 4, 6, 6) (uint8 [n]: the one-hot planes 32..35 at the centre cell, star_gambit_gs.cc:2604-2610;
    game_runner.py:2535) and the four variant names; None for every other game.  The keywords are plane_argmax's."""
    from .games import StarGambitUnifiedGS
    from .samples import plane_argmax
    cls = game if isinstance(game, type) else type(game)
    if not issubclass(cls, StarGambitUnifiedGS):
        return None
    return plane_argmax(canonical, 32, 4, 6, 6, **kwargs), UNIFIED_VARIANT_NAMES


def analyze_iteration(game, samples, net, **kwargs):
    """game_runner._analyze_iteration_variants on the samples where self_play leaves them: analyze_samples, split by variant for a
    unified StarGambit game (variant_buckets) and one "overall" bucket for every other game; the keywords are analyze_samples'."""
    from .samples import analyze_samples, _check_samples
    _, n, canonical, _, _ = _check_samples("analyze_iteration", samples, kwargs.get("batch_rows", 65536))
    split = variant_buckets(game, canonical, **{k: kwargs[k] for k in ("device", "stream") if k in kwargs}) if n else None
    if split is None:
        return analyze_samples(samples, net, **kwargs)
    return analyze_samples(samples, net, buckets=split[0], names=split[1], **kwargs)


def _pipeline_step(call, state, driver, what):
    """One call of the asynchronous pipeline under the error contract of include/azmi.h: a "pipeline error mask" error (a spin that hit
    the stall cap: the host was held up between the launches, another tenant took CUs) leaves the engine whole and the call is simply
    made again - at most three times per run; a precondition failure (no second hardware queue beside the caller's stream, no room for
    the kernels side by side, an engine the pipeline does not drive) makes driver="auto" fall back to the lock-step driver, with a warning;
    everything else (out of memory, invalid arguments) is raised.  Returns True when the call ran, False to fall back."""
    import warnings
    while True:
        try:
            call()
            return True
        except RuntimeError as e:
            msg = str(e)
            if "pipeline error mask" in msg and state["retries"] < 3:
                state["retries"] += 1
                warnings.warn(f"{what}: pipeline error, call repeated ({state['retries']} of 3): {msg[:200]}")
                continue
            precondition = any(k in msg for k in ("hardware queue", "does not hold", "the pipeline drives", "pipeline error mask"))
            if driver != "auto" or not precondition:
                raise
            warnings.warn(f"{what}: the asynchronous pipeline does not run here, falling back to the lock-step driver: {msg[:200]}")
            return False


@dataclasses.dataclass
class MatchResult:             # what play_past() returns from the PlayManager (game_runner.py:2250-2332)
    nn_rate: float
    draw_rate: float
    hit_rate: float
    game_length: float
    n_games: int
    nn_wins: int
    past_wins: int
    n_draws: int
    perm_scores: list
    driver_used: str = "rounds"      # as SelfPlayResult's
    pipeline_retries: int = 0
    fallbacks: int = 0


def gating_match(game, params, net_new, net_past, engines=2, seed=20240601, device=0, rounds_per_poll=256, driver="rounds", epochs_per_poll=16):
    """play_past (game_runner.py:2184-2332) on the device: model group 0 = the new model, group 1 = the past one, every seating
    of the two (2 players: both; N players: the new model alone in each seat, then the past model alone in each seat), games
    split over `engines` shards.  `net_new` / `net_past` are HipLeafNets, or None for the reference's RandPlayer (RANDOM
    evaluator).  `params` supplies the search settings (visits, temperatures, cache ...); its groups, permutations and
    evaluator types are set here like play_past does.
    driver: "rounds" (the default) = `engines` shards on the lock-step driver: the same seed gives the same match, game for game - gating
    decides model promotion; "auto" = ONE engine on the asynchronous pipeline with one net per model group (azmi_run_pipeline_groups)
    where it applies (Connect4 with Connect4-family nets; 2-3 x the games per second), falling back to the lock-step driver on the same
    engine when the pipeline cannot run - the k-th game of a slot is still a function of the seed alone, but WHICH slots receive the last
    restarts of a finite match depends on the order in which games end inside an epoch, so two runs of one seed may differ in a few
    games (as the reference's workers race for games_started_, play_manager.cc:506-513); "pipeline" = the pipeline or an error."""
    import copy
    import torch
    g = game() if isinstance(game, type) else game
    P = type(g).NUM_PLAYERS()
    p = copy.copy(params)
    if P == 2:
        p.model_groups, p.seat_perms = [0, 1], [[0, 1], [1, 0]]
    else:
        p.model_groups = [0] + [1] * (P - 1)
        p.seat_perms = [[0 if j == i else 1 for j in range(P)] for i in range(P)] + [[1 if j == i else 0 for j in range(P)] for i in range(P)]
    visits = list(p.mcts_visits)
    nets = [net_new, net_past]
    p.eval_type = [EvalType.NN if nets[grp] is not None else EvalType.RANDOM for grp in p.model_groups]
    p.mcts_visits = visits
    n_perms = len(p.seat_perms)
    use_pipe = False
    if driver in ("auto", "pipeline") and any(n is not None for n in nets):
        probe = PlayManager(type(g)(), _shard_params(p, 0, 1), seed=shard_seed(seed, 0), device=device)
        if pipeline_supported_groups(probe, nets):
            pms, K, use_pipe = [probe], 1, True
        elif driver == "pipeline":
            raise RuntimeError("gating_match: the pipeline does not drive this engine / these nets (alphazero.pipeline_supported_groups)")
        else:
            del probe
    if not use_pipe:
        K = max(1, min(int(engines), int(p.concurrent_games)))
        pms = [PlayManager(type(g)(), _shard_params(p, k, K), seed=shard_seed(seed, k), device=device) for k in range(K)]
    streams = [torch.cuda.Stream(device=device) for _ in range(K)]
    sps = [s.cuda_stream for s in streams]
    live = list(range(K))
    pipe_state = {"retries": 0, "fallbacks": 0, "driver": "pipeline" if use_pipe else "rounds"}
    while live:
        if use_pipe:
            if not _pipeline_step(lambda: run_pipeline_groups(pms[0], nets, epochs_per_poll, 256 * int(p.concurrent_games), sps[0]), pipe_state, driver, "gating_match"):
                use_pipe = False          # (a pipeline error leaves the engine whole: the lock-step driver carries on with it)
                pipe_state["fallbacks"] += 1; pipe_state["driver"] = "rounds"
                continue
        else:
            run_rounds_groups([pms[i] for i in live], nets, rounds_per_poll, [sps[i] for i in live])
        live = [i for i in live if pms[i].poll(sps[i])[1] > 0]
    perm_scores = [np.sum([pm.perm_scores(q) for pm in pms], 0) for q in range(n_perms)]
    perm_games = [sum(pm.perm_games_completed(q) for pm in pms) for q in range(n_perms)]
    nn_rate = draw_rate = 0.0
    n_games = nn_wins = past_wins = n_draws = 0
    for q in range(n_perms):                              # game_runner.py:2268-2288
        if perm_games[q] == 0:
            continue
        n_games += perm_games[q]
        for seat in range(P):
            if p.seat_perms[q][seat] == 0:
                nn_rate += float(perm_scores[q][seat]) / perm_games[q]; nn_wins += int(perm_scores[q][seat])
            else:
                past_wins += int(perm_scores[q][seat])
        draw_rate += float(perm_scores[q][P]) / perm_games[q]; n_draws += int(perm_scores[q][P])
    cs = np.sum([pm._cache_stats() for pm in pms], 0)
    sums = {}
    for pm in pms:
        for k2, v in pm.stat_sums().items():
            sums[k2] = sums.get(k2, 0.0) + v
    return MatchResult(nn_rate=nn_rate / n_perms, draw_rate=draw_rate / n_perms, hit_rate=(float(cs[0]) / float(cs[0] + cs[1])) if cs[0] + cs[1] else 0.0,
                       game_length=(sums["game_length"] / sums["games"]) if sums["games"] else 0.0, n_games=n_games, nn_wins=nn_wins,
                       past_wins=past_wins, n_draws=n_draws, perm_scores=[x.tolist() for x in perm_scores],
                       driver_used=pipe_state["driver"], pipeline_retries=pipe_state["retries"], fallbacks=pipe_state["fallbacks"])
