"""-m gpu: the asynchronous tree / net pipeline (azmi_run_pipeline, csrc/pipeline*.hip) plays the games of the lock-step engine and
of the oracle.  A slot's game is a function of its seed alone: the answer to a position does not depend on when, where or in
which tile the net evaluates it, so persistent tree wavefronts + persistent net workgroups (request ring, tagged result granules,
moves and cache inserts between epochs) must reproduce, move for move / visit count for visit count / pcg32 position for pcg32
position, what azmi_run_rounds plays and what the ORACLE PlayManager plays when its evaluator sends each leaf through the same
HIP net (tier T3).  Reference: PlayManager::play (play_manager.cc:258-600), which has no global barrier either."""
import numpy as np
import pytest
import torch

from test_gpu_t3_nn_in_the_loop import _check_slots, _net_eval, _selfplay_params

pytestmark = pytest.mark.gpu


def _pipeline_games(az, pp, seed, hip, sims_per_epoch, max_epochs=4000, env=None):
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    assert az.pipeline_supported(pm, hip)
    st = torch.cuda.Stream()
    stats, epochs = None, 0
    while pm.remaining_games() > 0 and epochs < max_epochs:
        stats = az.run_pipeline(pm, hip, 4, sims_per_epoch, st.cuda_stream)
        epochs += 4
        if pm.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    return pm, pm.move_log(), stats


def _lockstep_games(az, pp, seed, hip):
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    st = torch.cuda.Stream()
    while pm.remaining_games() > 0:
        az.run_rounds([pm], hip, 64, [st.cuda_stream])
        if pm.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    return pm, pm.move_log()


def _sorted_log(rows, counts):
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))          # by slot, game in slot, turn
    return rows[order], counts[order]


def _history_multiset(pm):
    if getattr(pm, "_hist_rows", None) is None:       # (history() hands the rows out once)
        c, v, p = pm.history()
        rows = np.concatenate([c.reshape(len(c), -1), v, p], 1)
        pm._hist_rows = rows[np.lexsort(rows.T[::-1])]
    return pm._hist_rows


@pytest.mark.parametrize("cache", [0, 1 << 16])
def test_pipeline_plays_the_lockstep_engines_games(cache):
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=21), spec)
    S, seed = 128, 9001
    pp = _selfplay_params(az, S, 100, cache=cache)
    pa, (ra, ca), stats = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 40)
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pa.games_completed() == pb.games_completed() == S
    ra, ca = _sorted_log(ra, ca)
    rb, cb = _sorted_log(rb, cb)
    assert ra.shape == rb.shape and len(ra) > 8 * S
    assert np.array_equal(ra, rb), "moves / pcg32 positions differ between the pipeline and the lock-step engine"
    assert np.array_equal(ca, cb), "visit counts differ"
    assert np.array_equal(pa.scores(), pb.scores())
    assert np.array_equal(_history_multiset(pa), _history_multiset(pb)), "sample rows differ"
    xa, xb = pa.counters(), pb.counters()
    assert xa["sims"] == xb["sims"]
    assert stats["tiles"] > 0 and stats["tile_boards"] >= stats["tiles"]
    assert stats["tree_wgs_started"] == stats["tree_wgs"]
    if cache:
        assert xa["cache_hits"] > 0 and xa["evals"] < xa["sims"]
    else:
        assert xa["evals"] == xb["evals"]         # without a cache every non-terminal leaf goes to the net on both paths


def test_pipeline_equals_the_oracle_driven_by_the_same_net(oracle):
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=11), spec)
    S, seed = 96, 4242
    pp = _selfplay_params(az, S, 120, cache=1 << 16)
    pm, (rows, counts), _ = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 64)
    assert pm.games_completed() == S
    n = _check_slots(az, oracle, oracle.GAME_CONNECT4, pp, seed, rows, counts, (0, 1, 17, 40, 95), evaluator=_net_eval(hip))
    assert n > 40


def test_pipeline_with_playout_cap_resign_and_restarts(oracle):
    """playout-cap randomisation, resignation with play-through and a game stream longer than the slots (restarts between
    epochs): the first game of sampled slots equals the oracle's, the stream completes."""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=12), spec)
    S, seed = 48, 77
    pp = _selfplay_params(az, S, 80, cache=1 << 14)
    pp.games_to_play = 3 * S
    pp.playout_cap_randomization, pp.playout_cap_depth, pp.playout_cap_percent = True, 12, 0.5
    pp.resign_percent, pp.resign_playthrough_percent = 0.05, 0.2
    pm, (rows, counts), _ = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 32)
    assert pm.games_completed() == 3 * S
    _check_slots(az, oracle, oracle.GAME_CONNECT4, pp, seed, rows, counts, (0, 7, 47), evaluator=_net_eval(hip))


def test_pipeline_and_lockstep_rounds_interleave_on_one_engine():
    """epochs of the pipeline and rounds of the lock-step driver alternate on ONE engine: between epochs a slot is in the
    lock-step kernels' own form (pending answers in the (v, pi) rows), so the games are still the games of either driver."""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=5), spec)
    S, seed = 64, 31337
    pp = _selfplay_params(az, S, 64, cache=1 << 14)
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    st = torch.cuda.Stream()
    turn = 0
    while pm.remaining_games() > 0 and turn < 5000:
        if turn % 2 == 0:
            az.run_pipeline(pm, hip, 2, S * 16, st.cuda_stream)
        else:
            az.run_rounds([pm], hip, 5, [st.cuda_stream])
        turn += 1
        if pm.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    assert pm.games_completed() == S
    ra, ca = _sorted_log(*pm.move_log())
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    rb, cb = _sorted_log(rb, cb)
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)


def test_pipeline_rejects_what_it_does_not_drive():
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=1), spec)
    pp = _selfplay_params(az, 8, 16, cache=0)
    pp.eval_type = [az.EvalType.NN, az.EvalType.PLAYOUT]
    pp.model_groups = [0, 1]
    pm = az.PlayManager(az.Connect4GS(), pp, seed=1)
    assert not az.pipeline_supported(pm, hip)                     # a PLAYOUT seat: the rollout code is the lock-step engine's
    with pytest.raises(RuntimeError, match="pipeline"):
        az.run_pipeline(pm, hip, 1, 100)
    pp2 = _selfplay_params(az, 4, 8, cache=0)
    tw = az.PlayManager(az.TawlbwrddGS(), pp2, seed=1)
    assert not az.pipeline_supported(tw, hip)                     # the wide-game engine
    pp3 = _selfplay_params(az, 8, 16, cache=0)
    pp3.model_groups = [0, 1]
    two = az.PlayManager(az.Connect4GS(), pp3, seed=1)
    x3 = az.HipLeafNet(torch_net.random_init(spec, seed=2), spec, precision="bf16x3")
    assert az.pipeline_supported_groups(two, [hip, hip])
    assert not az.pipeline_supported_groups(two, [hip, None])     # NN seats without a net
    assert not az.pipeline_supported_groups(two, [hip, x3])       # two precision tiers in one call
    with pytest.raises(RuntimeError, match="pipeline"):
        az.run_pipeline_groups(two, [hip, None], 1, 100)


# ---- the generic tree kernel (round 4): Gumbel seats, two model groups ---------------------------------------------------------
def _groups_pipeline_games(az, pp, seed, nets, sims_per_epoch, max_calls=4000, recovered_errors=0):
    """recovered_errors: how many pipeline errors (a spin that hit the stall cap: reported once, the engine stays whole - the
    recoverable-error contract, test_a_pipeline_error_is_reported_once...) the run may meet and carry on from; the games are compared
    afterwards all the same"""
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    assert az.pipeline_supported_groups(pm, nets)
    st = torch.cuda.Stream()
    stats, n = None, 0
    while pm.remaining_games() > 0 and n < max_calls:
        try:
            stats = az.run_pipeline_groups(pm, nets, 4, sims_per_epoch, st.cuda_stream)
        except RuntimeError as e:
            if "pipeline error mask" not in str(e) or recovered_errors <= 0:
                raise
            recovered_errors -= 1
            print("recovered pipeline error:", str(e)[:400])
            continue
        n += 1
        if pm.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    return pm, pm.move_log(), stats


def _groups_lockstep_games(az, pp, seed, nets):
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    st = torch.cuda.Stream()
    while pm.remaining_games() > 0:
        az.run_rounds_groups([pm], list(nets), 64, [st.cuda_stream])
        if pm.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    return pm, pm.move_log()


def _same_games(pa, la, pb, lb, S):
    assert pa.games_completed() == pb.games_completed() == S
    ra, ca = _sorted_log(*la)
    rb, cb = _sorted_log(*lb)
    assert ra.shape == rb.shape and len(ra) > 6 * S
    assert np.array_equal(ra, rb), "moves / pcg32 positions differ between the pipeline and the lock-step engine"
    assert np.array_equal(ca, cb), "visit counts differ"
    assert np.array_equal(pa.scores(), pb.scores())
    assert np.array_equal(_history_multiset(pa), _history_multiset(pb)), "sample rows differ"
    assert pa.counters()["sims"] == pb.counters()["sims"]


_GUMBEL = {
    "global": dict(gumbel_enabled=True, gumbel_m=8),
    "full_improved": dict(gumbel_enabled=True, gumbel_m=16, gumbel_full=True, seat_gumbel_use_improved_policy=[[1, 1]], gumbel_c_scale=0.5),
    "one_seat": dict(seat_gumbel_enabled=[[1, 0]], seat_gumbel_m=[[4, 16]], seat_gumbel_c_visit=[[50.0, 20.0]]),
}


@pytest.mark.parametrize("name", sorted(_GUMBEL))
@pytest.mark.parametrize("cache", [0, 1 << 15])
def test_pipeline_drives_gumbel_seats(name, cache):
    """Sequential-halving Gumbel roots (mcts.cc:233-342) on the pipeline (the fast tree kernel's Gumbel build: the root's choice by the
    halving schedule, interior nodes by the improved policy when gumbel_full) - moves, visit counts, pcg32 positions and sample rows
    (the improved policy) are the lock-step engine's"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=31), spec)
    S, seed = 96, 515
    pp = _selfplay_params(az, S, 64, cache=cache)
    for k, v in _GUMBEL[name].items():
        setattr(pp, k, v)
    pa, la, stats = _groups_pipeline_games(az, pp, seed, [hip], S * 24)
    pb, lb = _groups_lockstep_games(az, pp, seed, [hip])
    _same_games(pa, la, pb, lb, S)
    assert stats["tiles"] > 0 and stats["tree_wgs_started"] == stats["tree_wgs"]
    if cache:
        assert pa.counters()["cache_hits"] > 0


@pytest.mark.parametrize("shape", ["gumbel", "two_nets"])
def test_generic_tree_kernel_plays_the_same_games(monkeypatch, shape):
    """AZMI_PIPE_GENERIC=1: the generic tree kernel (every step of a slot through the lock-step engine's own move-step function, one
    simulation per pass) as an independent cross-check of the fast kernel's Gumbel and two-group builds"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    nets = [az.HipLeafNet(torch_net.random_init(spec, seed=51), spec), az.HipLeafNet(torch_net.random_init(spec, seed=52), spec)]
    S, seed = 64, 949
    pp = _selfplay_params(az, S, 48, cache=1 << 14)
    if shape == "gumbel":
        pp.gumbel_enabled, pp.gumbel_m, pp.gumbel_full = True, 8, True
        nets = nets[:1]
    else:
        pp.model_groups, pp.seat_perms = [0, 1], [[0, 1], [1, 0]]
        pp.seat_gumbel_enabled = [[1, 0], [0, 0]]
    pa, la, _ = _groups_pipeline_games(az, pp, seed, nets, S * 16)
    monkeypatch.setenv("AZMI_PIPE_GENERIC", "1")
    # (round 4 met a stall-cap error here once in ~3000 calls and tolerated it; round 5 found it - every wavefront of both kernels stood
    # still for ~200 ms inside ONE poll: the GPU's scheduler, not the protocol - and credits such freezes against the caps
    # (pipe_freeze_credit, profiles/r5_repro_generic.txt): the test is strict again)
    pb, lb, stats = _groups_pipeline_games(az, pp, seed, nets, S * 16)
    monkeypatch.delenv("AZMI_PIPE_GENERIC")
    _same_games(pa, la, pb, lb, S)
    pc, lc = _groups_lockstep_games(az, pp, seed, nets)
    _same_games(pa, la, pc, lc, S)


def test_pipeline_gumbel_equals_the_oracle_driven_by_the_same_net(oracle):
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=32), spec)
    S, seed = 40, 616
    pp = _selfplay_params(az, S, 48, cache=1 << 14)
    pp.gumbel_enabled, pp.gumbel_m = True, 8
    pm, (rows, counts), _ = _groups_pipeline_games(az, pp, seed, [hip], S * 16)
    assert pm.games_completed() == S
    _check_slots(az, oracle, oracle.GAME_CONNECT4, pp, seed, rows, counts, (0, 13, 39), evaluator=_net_eval(hip))


@pytest.mark.parametrize("cache", [0, 1 << 15])
def test_pipeline_routes_two_model_groups_to_two_nets(oracle, cache):
    """play_past (game_runner.py:2184-2332): two DIFFERENT nets, seats swapped by the permutations, one request ring and one S3-FIFO per
    group - the games of the lock-step engine with the same two nets and of the oracle whose group evaluator sends a leaf to its
    group's net; swapping the nets changes the games"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    nets = [az.HipLeafNet(torch_net.random_init(spec, seed=41), spec), az.HipLeafNet(torch_net.random_init(spec, seed=42), spec)]
    evs = [_net_eval(n) for n in nets]
    S, seed = 64, 727
    pp = _selfplay_params(az, S, 60, cache=cache)
    pp.mcts_visits = [60, 44]
    pp.model_groups, pp.seat_perms = [0, 1], [[0, 1], [1, 0]]
    pa, la, stats = _groups_pipeline_games(az, pp, seed, nets, S * 24)
    pb, lb = _groups_lockstep_games(az, pp, seed, nets)
    _same_games(pa, la, pb, lb, S)
    for q in range(2):
        assert np.array_equal(pa.perm_scores(q), pb.perm_scores(q)) and pa.perm_games_completed(q) == pb.perm_games_completed(q)
    rows, counts = la
    _check_slots(az, oracle, oracle.GAME_CONNECT4, pp, seed, rows, counts, (0, 1, 62, 63), group_evaluator=lambda g, c: evs[g](c))
    pc, lc, _ = _groups_pipeline_games(az, pp, seed, nets[::-1], S * 24)
    assert not np.array_equal(_sorted_log(*lc)[0][:, 2:4], _sorted_log(*la)[0][:, 2:4]) or len(lc[0]) != len(la[0])
    if cache:
        assert pa.counters()["cache_hits"] > 0


def test_pipeline_groups_with_external_caches_of_two_sizes():
    """PlayManager(gs, params, caches=[...]) (play_manager.cc:644-649): the caller's ShardedS3FIFOCache per model group, of DIFFERENT sizes
    (the insert locks of group 1's shards start behind group 0's); a second engine on the same caches starts warm"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    nets = [az.HipLeafNet(torch_net.random_init(spec, seed=61), spec), az.HipLeafNet(torch_net.random_init(spec, seed=62), spec)]
    S, seed = 48, 1051
    pp = _selfplay_params(az, S, 50, cache=0)
    pp.model_groups, pp.seat_perms = [0, 1], [[0, 1], [1, 0]]

    def games(caches, pipeline):
        pm = az.PlayManager(az.Connect4GS(), pp, caches=caches, seed=seed, log_moves=True)
        st = torch.cuda.Stream()
        n = 0
        while pm.remaining_games() > 0 and n < 4000:
            if pipeline:
                az.run_pipeline_groups(pm, nets, 4, S * 20, st.cuda_stream)
            else:
                az.run_rounds_groups([pm], nets, 64, [st.cuda_stream])
            n += 1
            if pm.poll(st.cuda_stream)[1] == 0:
                break
        torch.cuda.synchronize()
        return pm
    ca = [az.ShardedS3FIFOCache.for_engine(8192, 7, 3), az.ShardedS3FIFOCache.for_engine(2048, 7, 3)]
    cb = [az.ShardedS3FIFOCache.for_engine(8192, 7, 3), az.ShardedS3FIFOCache.for_engine(2048, 7, 3)]
    pa, pb = games(ca, True), games(cb, False)
    _same_games(pa, pa.move_log(), pb, pb.move_log(), S)
    assert ca[0].size() > 0 and ca[1].size() > 0 and ca[0].hits() > 0
    evals_cold = pa.counters()["evals"]
    again = games(ca, True)                        # the same games on the warm caches: fewer leaves reach the nets
    assert again.counters()["evals"] < evals_cold
    ra, _ = _sorted_log(*pa.move_log())
    rb, _ = _sorted_log(*again.move_log())
    assert np.array_equal(ra[:, :5], rb[:, :5])


def test_pipeline_with_a_net_behind_one_group_and_random_seats_in_the_other():
    """the reference's baseline match (game_runner.py:2143-2182: the model against RandPlayer): group 1's seats use EvalType.RANDOM, so
    only group 0 has a ring and a net behind it; a per-seat Gumbel seat on top"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=43), spec)
    S, seed = 48, 838
    pp = _selfplay_params(az, S, 40, cache=1 << 14)
    pp.model_groups, pp.seat_perms = [0, 1], [[0, 1], [1, 0]]
    pp.eval_type = [az.EvalType.NN, az.EvalType.RANDOM]
    pp.seat_gumbel_enabled = [[1, 0], [0, 0]]
    pa, la, stats = _groups_pipeline_games(az, pp, seed, [hip, None], S * 16)
    pb, lb = _groups_lockstep_games(az, pp, seed, [hip, None])
    _same_games(pa, la, pb, lb, S)
    assert 0 < pa.counters()["evals"] < pa.counters()["sims"]


def test_ring_positions_wrap_past_2_to_the_32(monkeypatch):
    """the rings' positions are free-running 32-bit counters (a long run wraps them after about two minutes): started 40,000
    positions below 2^32 (AZMI_PIPE_POS0, read when an engine's pipeline is created), the request, READY and MOVE rings all wrap
    inside this run and the games are still the lock-step engine's."""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=33), spec)
    S, seed = 192, 555
    pp = _selfplay_params(az, S, 150, cache=1 << 15)
    monkeypatch.setenv("AZMI_PIPE_POS0", str((1 << 32) - 40000))
    pa, (ra, ca), stats = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 48)
    monkeypatch.delenv("AZMI_PIPE_POS0")
    assert pa.counters()["evals"] > 60000             # more requests than the distance to the wrap
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pa.games_completed() == pb.games_completed() == S
    ra, ca = _sorted_log(ra, ca)
    rb, cb = _sorted_log(rb, cb)
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)


@pytest.mark.parametrize("S,sims,cache,spe,epochs", [
    (100, 60, 1 << 12, 37, 3),            # fewer simulations per epoch than slots: epochs of a fraction of a pass
    (257, 33, 0, 257 * 5, 1),             # odd slot count, no cache, one epoch per call
    (1000, 25, 1 << 16, 1000 * 300, 2),   # the quota never ends an epoch: the waiting-slot rule and the movers do
    (24, 200, 1 << 10, 24 * 8, 7),        # fewer slots than one workgroup serves, a cache that evicts constantly
])
def test_pipeline_equals_lockstep_over_odd_shapes(S, sims, cache, spe, epochs):
    """slot counts that are not multiples of anything, epochs far shorter and far longer than a search, a cache smaller than one
    game's positions: the games are the lock-step engine's every time (moves, visit counts, pcg32 positions, sample rows)"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=S), spec)
    pp = _selfplay_params(az, S, sims, cache=cache)
    pp.games_to_play = S + S // 2                      # restarts and retirements inside the run
    seed = 1000 + S
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    st = torch.cuda.Stream()
    calls = 0
    while pm.remaining_games() > 0 and calls < 200000:
        az.run_pipeline(pm, hip, epochs, spe, st.cuda_stream)
        calls += 1
        if pm.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pm.games_completed() == pb.games_completed() == pp.games_to_play
    ra, ca = _sorted_log(*pm.move_log())
    rb, cb = _sorted_log(rb, cb)
    # WHICH slots receive the last restarts depends on the order in which games end (the reference's workers race for
    # games_started_ the same way, play_manager.cc:506-513) - the lock-step engine hands them out round by round, the pipeline epoch
    # by epoch -, but the k-th game of a slot is a function of the seed alone: every (slot, game) both drivers played is identical
    def by_game(rows, counts):
        out = {}
        for key in np.unique(rows[:, :2], axis=0):
            sel = (rows[:, 0] == key[0]) & (rows[:, 1] == key[1])
            out[(int(key[0]), int(key[1]))] = (rows[sel], counts[sel])
        return out
    ga, gb = by_game(ra, ca), by_game(rb, cb)
    common = sorted(set(ga) & set(gb))
    assert all((s_, 0) in ga and (s_, 0) in gb for s_ in range(S))            # every slot's first game ran on both
    assert len(common) >= S + S // 4
    for key in common:
        assert np.array_equal(ga[key][0], gb[key][0]) and np.array_equal(ga[key][1], gb[key][1]), key
    if set(ga) == set(gb):
        assert np.array_equal(pm.scores(), pb.scores())
        assert np.array_equal(_history_multiset(pm), _history_multiset(pb))


def test_pipeline_after_stop_returns_at_once_and_changes_nothing():
    """PlayManager.stop() (py_wrapper.cc:369-372): epochs asked for afterwards find the stop word, every persistent workgroup leaves
    at once, no pipeline error is raised and no simulation runs"""
    import time
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=2), spec)
    S = 512
    pp = _selfplay_params(az, S, 200, cache=1 << 14)
    pp.games_to_play = 1 << 20
    pm = az.PlayManager(az.Connect4GS(), pp, seed=5)
    az.run_pipeline(pm, hip, 4, S * 32)
    before = pm.counters()["sims"]
    assert before > 0
    pm.stop()
    assert pm.stopped()
    t0 = time.perf_counter()
    stats = az.run_pipeline(pm, hip, 8, S * 32)
    assert time.perf_counter() - t0 < 1.0
    assert stats["last_epoch_sims"] == 0 and pm.counters()["sims"] == before


def test_two_pipelines_and_two_nets_alternate_in_one_process():
    """two engines, each with its own pipeline state, take turns on one stream, each with its own net: nothing of a pipeline is
    process-wide, so both play the games their lock-step twins play"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    nets = [az.HipLeafNet(torch_net.random_init(spec, seed=s), spec) for s in (41, 42)]
    cfgs = [(128, 70, 1 << 14, 901), (96, 90, 0, 902)]
    pms = []
    for (S, sims, cache, seed) in cfgs:
        pms.append(az.PlayManager(az.Connect4GS(), _selfplay_params(az, S, sims, cache=cache), seed=seed, log_moves=True))
    st = torch.cuda.Stream()
    for _ in range(100000):
        live = 0
        for pm, net, (S, _, _, _) in zip(pms, nets, cfgs):
            if pm.remaining_games() > 0 and pm.poll(st.cuda_stream)[1] > 0:
                az.run_pipeline(pm, net, 2, S * 24, st.cuda_stream)
                live += 1
        if live == 0:
            break
    torch.cuda.synchronize()
    for pm, net, (S, sims, cache, seed) in zip(pms, nets, cfgs):
        pb, (rb, cb) = _lockstep_games(az, _selfplay_params(az, S, sims, cache=cache), seed, net)
        assert pm.games_completed() == pb.games_completed() == S
        ra, ca = _sorted_log(*pm.move_log())
        rb, cb = _sorted_log(rb, cb)
        assert np.array_equal(ra, rb) and np.array_equal(ca, cb)


def test_pipeline_reports_a_full_sample_ring_by_name():
    """a sample ring that is too small and never drained: the move step raises the engine's overflow bit inside an epoch, every
    persistent workgroup leaves, and the call fails with the engine's own message - no hang, no pipeline time-out"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=7), spec)
    pp = _selfplay_params(az, 64, 30, cache=0)
    pp.games_to_play = 640
    pm = az.PlayManager(az.Connect4GS(), pp, seed=5, history_capacity=128)
    with pytest.raises(RuntimeError, match="history"):
        for _ in range(400):
            az.run_pipeline(pm, hip, 2, 64 * 16)
            pm.poll()


def test_pipeline_holds_a_huge_epoch_quota_below_the_stall_cap():
    """sims_per_epoch far beyond what an epoch may last: the library holds the quota to 1024 simulations per slot, the epochs
    end by it and the run completes without touching the wall-clock cap"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=8), spec)
    S = 256
    pp = _selfplay_params(az, S, 300, cache=1 << 14)
    pm = az.PlayManager(az.Connect4GS(), pp, seed=12)
    for _ in range(4000):
        st = az.run_pipeline(pm, hip, 1, 1 << 40)
        assert st["last_epoch_sims"] <= 1024 * S + 64 * S
        if pm.poll()[1] == 0:
            break
    assert pm.games_completed() == S


def test_a_small_engine_launches_no_more_net_workgroups_than_its_slots_can_keep_busy(monkeypatch):
    """round 5: a slot has one request out at most and a tile takes three, so an epoch launches min(measured places, S / 3 + 8) net
    workgroups - hundreds of idle persistent workgroups beside a few tree workgroups are what the seconds-long stalls of the tree side
    needed; AZMI_PIPE_NET_ALL=1 launches them all (the games are the same either way)"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=31), spec)
    S, seed = 96, 4242
    pp = _selfplay_params(az, S, 60, cache=1 << 14)
    pa, (ra, ca), stats = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 40)
    assert stats["net_wgs"] == (S + 2) // 3 + 8 and stats["net_wgs_started"] == stats["net_wgs"]
    monkeypatch.setenv("AZMI_PIPE_NET_ALL", "1")
    pb, (rb, cb), stats_all = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 40)
    monkeypatch.delenv("AZMI_PIPE_NET_ALL")
    assert stats_all["net_wgs"] > 2 * stats["net_wgs"] and stats_all["net_wgs_started"] == stats_all["net_wgs"]
    sa, sb = _sorted_log(ra, ca), _sorted_log(rb, cb)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])


def test_pipeline_follows_the_callers_stream_from_call_to_call():
    """the caller's stream changes between calls (two torch streams and the engine's own): the net-side stream is re-checked against
    each new partner (a shared hardware queue would serialise the two persistent kernels) and the games stay the lock-step engine's"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=9), spec)
    S, seed = 128, 77
    pp = _selfplay_params(az, S, 80, cache=1 << 14)
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None, torch.cuda.Stream(), torch.cuda.Stream()]
    i = 0
    while pm.remaining_games() > 0 and i < 20000:
        s = streams[i % len(streams)]
        torch.cuda.synchronize()                     # (the engine's state is handed from stream to stream by the caller)
        az.run_pipeline(pm, hip, 2, S * 32, None if s is None else s.cuda_stream)
        i += 1
        if pm.poll(None if s is None else s.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pm.games_completed() == pb.games_completed() == S
    ra, ca = _sorted_log(*pm.move_log())
    rb, cb = _sorted_log(rb, cb)
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)


def test_two_threads_drive_two_pipelines():
    """two host threads, each driving its own engine through azmi_run_pipeline (ctypes releases the GIL): the calls take turns inside
    the library - an epoch's workgroup counts assume the chip to itself - and both engines finish with their lock-step twins' games"""
    import threading
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=10), spec)
    cfgs = [(160, 60, 1 << 13, 301), (96, 70, 0, 302)]
    pms = [az.PlayManager(az.Connect4GS(), _selfplay_params(az, S, sims, cache=cache), seed=seed, log_moves=True) for (S, sims, cache, seed) in cfgs]
    errors = []

    def drive(pm, S):
        try:
            st = torch.cuda.Stream()
            n = 0
            while pm.remaining_games() > 0 and n < 20000:
                az.run_pipeline(pm, hip, 2, S * 24, st.cuda_stream)
                n += 1
                if pm.poll(st.cuda_stream)[1] == 0:
                    break
        except Exception as e:          # noqa: BLE001 - reported by the main thread
            errors.append(e)
    threads = [threading.Thread(target=drive, args=(pm, cfg[0])) for pm, cfg in zip(pms, cfgs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    torch.cuda.synchronize()
    assert not errors, errors
    for pm, (S, sims, cache, seed) in zip(pms, cfgs):
        pb, (rb, cb) = _lockstep_games(az, _selfplay_params(az, S, sims, cache=cache), seed, hip)
        assert pm.games_completed() == pb.games_completed() == S
        ra, ca = _sorted_log(*pm.move_log())
        rb, cb = _sorted_log(rb, cb)
        assert np.array_equal(ra, rb) and np.array_equal(ca, cb)


def test_tree_side_alone_with_random_seats_plays_the_lockstep_games():
    """round 4: an engine whose seats all use EvalType.RANDOM runs on the pipeline's tree kernel alone (no request ever leaves, no net
    kernel is launched: what rocprofv3 --pmc looks at) - moves, visit counts and pcg32 positions are the lock-step engine's"""
    import alphazero as az
    S, seed = 200, 606
    pp = _selfplay_params(az, S, 90, cache=0)
    pp.eval_type = [az.EvalType.RANDOM, az.EvalType.RANDOM]
    pp.games_to_play = S + 40
    pa = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    assert az.pipeline_supported(pa, None)
    st = torch.cuda.Stream()
    n = 0
    while pa.remaining_games() > 0 and n < 20000:
        stats = az.run_pipeline(pa, None, 3, S * 50, st.cuda_stream)
        n += 1
        if pa.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    assert stats["tiles"] == 0 and stats["net_wgs_started"] == 0
    pb = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    pb.play()
    assert pa.games_completed() == pb.games_completed() == pp.games_to_play
    ra, ca = _sorted_log(*pa.move_log())
    rb, cb = _sorted_log(*pb.move_log())
    first = ra[:, 1] == 0                      # (the last restarts may land in other slots: see test_pipeline_equals_lockstep_over_odd_shapes)
    firstb = rb[:, 1] == 0
    assert np.array_equal(ra[first], rb[firstb]) and np.array_equal(ca[first], cb[firstb])


@pytest.mark.parametrize("tree_wgs,net_wgs", [(5, 700), (3, None), (7, 40)])
def test_workgroup_counts_are_measured_not_assumed(monkeypatch, tree_wgs, net_wgs):
    """round 4: nothing in the library encodes how the dispatcher deals workgroups to shader engines - the net side's workgroup count is
    MEASURED beside the tree workgroups before the first epoch (pipe_calibrate: both kernels launched with a hold, late starters
    counted).  Perturbed counts - an odd number of tree workgroups, far more net workgroups than the chip holds, far fewer - either
    run (with every launched workgroup resident: no late starter) or fail by name; the games are the lock-step engine's."""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=14), spec)
    S, seed = 160, 2024
    pp = _selfplay_params(az, S, 70, cache=1 << 14)
    monkeypatch.setenv("AZMI_PIPE_TREE_WGS", str(tree_wgs))
    if net_wgs is not None:
        monkeypatch.setenv("AZMI_PIPE_NET_WGS", str(net_wgs))
    pa, (ra, ca), stats = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 40)
    monkeypatch.delenv("AZMI_PIPE_TREE_WGS")
    if net_wgs is not None:
        monkeypatch.delenv("AZMI_PIPE_NET_WGS")
    assert stats["tree_wgs"] == tree_wgs and stats["tree_wgs_started"] == tree_wgs
    assert stats["net_wgs_started"] == stats["net_wgs"] and stats["calibration_rounds"] >= 1
    if net_wgs == 700:
        assert stats["net_wgs"] < 700 and stats["calibration_rounds"] >= 2       # the chip does not hold 700 + 5 workgroups of this size
    if net_wgs == 40:
        assert stats["net_wgs"] == 40
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pa.games_completed() == pb.games_completed() == S
    ra, ca = _sorted_log(ra, ca)
    rb, cb = _sorted_log(rb, cb)
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)


def test_a_pipeline_error_is_reported_once_and_the_engine_stays_usable(monkeypatch):
    """a spin that hits the epoch's time cap (here: a cap of 20 us) is reported by name - and then cleared.  Slots whose
    requests went unanswered are back in the move step's kSlotQueued form, so later calls of EITHER driver carry on: the finished
    games are still the lock-step engine's."""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=15), spec)
    S, seed = 192, 99
    pp = _selfplay_params(az, S, 60, cache=1 << 13)
    pm = az.PlayManager(az.Connect4GS(), pp, seed=seed, log_moves=True)
    st = torch.cuda.Stream()
    az.run_pipeline(pm, hip, 2, S * 16, st.cuda_stream)
    monkeypatch.setenv("AZMI_PIPE_CAP_MS", "0.02")
    monkeypatch.setenv("AZMI_PIPE_SOFT_MS", "1000")        # (an epoch normally ends at a quarter of the cap, before it can trip)
    failures = 0
    for _ in range(3):
        try:
            az.run_pipeline(pm, hip, 2, S * 400, st.cuda_stream)
        except RuntimeError as e:
            assert "pipeline error mask" in str(e)
            failures += 1
    monkeypatch.delenv("AZMI_PIPE_CAP_MS")
    monkeypatch.delenv("AZMI_PIPE_SOFT_MS")
    assert failures >= 1
    turn = 0
    while pm.remaining_games() > 0 and turn < 20000:
        if turn % 3 == 2:
            az.run_rounds([pm], hip, 4, [st.cuda_stream])
        else:
            az.run_pipeline(pm, hip, 2, S * 32, st.cuda_stream)
        turn += 1
        if pm.poll(st.cuda_stream)[1] == 0:
            break
    torch.cuda.synchronize()
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pm.games_completed() == pb.games_completed() == S
    ra, ca = _sorted_log(*pm.move_log())
    rb, cb = _sorted_log(rb, cb)
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)


def test_self_play_auto_falls_back_when_the_pipeline_cannot_run(monkeypatch):
    """self_play(driver="auto") must not raise where the lock-step default worked - the pipeline's run-time preconditions
    are only known once it runs (here it is made to fail: a 1 us time cap); "auto" then plays the games on lock-step shards, and only
    driver="pipeline" raises"""
    import alphazero as az
    from alphazero import torch_net, selfplay
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=16), spec)
    pp = _selfplay_params(az, 64, 40, cache=1 << 12)
    pp.games_to_play = 96
    monkeypatch.setenv("AZMI_PIPE_CAP_MS", "0.001")
    monkeypatch.setenv("AZMI_PIPE_SOFT_MS", "1000")
    res, _ = selfplay.self_play(az.Connect4GS, pp, hip, seed=5)
    assert res.games == 96
    # round 6: the change of driver is COUNTED in the result, and a caller that measures throughput can forbid it
    assert res.fallbacks == 1 and res.driver_used == "rounds" and res.pipeline_retries == 3
    with pytest.raises(RuntimeError, match="max_fallbacks"):
        selfplay.self_play(az.Connect4GS, pp, hip, seed=5, max_fallbacks=0)
    with pytest.raises(RuntimeError, match="pipeline"):
        selfplay.self_play(az.Connect4GS, pp, hip, seed=5, driver="pipeline")
    monkeypatch.delenv("AZMI_PIPE_CAP_MS"); monkeypatch.delenv("AZMI_PIPE_SOFT_MS")
    ok, _ = selfplay.self_play(az.Connect4GS, pp, hip, seed=5)
    assert ok.games == 96 and ok.fallbacks == 0 and ok.driver_used == "pipeline" and ok.pipeline_retries == 0


def test_pipeline_runs_the_bf16x3_tier(oracle):
    """round 4: the north star's 1e-5 tier (precision="bf16x3": bf16 high + low parts, three MFMAs per product) on the fast driver -
    k_pipe_net<.., X3>, one net workgroup per CU (16 activation planes) beside the tree workgroups, its workgroup count measured like
    the bf16 kernel's.  The games are the lock-step engine's with the same net, and the oracle's driven by that net."""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=23), spec, precision="bf16x3")
    S, seed = 144, 808
    pp = _selfplay_params(az, S, 90, cache=1 << 14)
    pm0 = az.PlayManager(az.Connect4GS(), pp, seed=seed)
    assert az.pipeline_supported(pm0, hip)
    del pm0
    pa, (ra, ca), stats = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 40)
    assert stats["tiles"] > 0 and stats["net_wgs_started"] == stats["net_wgs"] and stats["calibration_rounds"] >= 1
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pa.games_completed() == pb.games_completed() == S
    sa, sb = _sorted_log(ra, ca), _sorted_log(rb, cb)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    n = _check_slots(az, oracle, oracle.GAME_CONNECT4, pp, seed, ra, ca, (0, 5, 143), evaluator=_net_eval(hip))
    assert n > 20
    # one engine, two tiers: a bf16 net on the same engine re-sizes and re-measures the net side
    hip16 = az.HipLeafNet(torch_net.random_init(spec, seed=23), spec)
    pp2 = _selfplay_params(az, 64, 40, cache=0)
    pm2 = az.PlayManager(az.Connect4GS(), pp2, seed=3)
    st = torch.cuda.Stream()
    a = az.run_pipeline(pm2, hip, 1, 64 * 16, st.cuda_stream)
    b = az.run_pipeline(pm2, hip16, 1, 64 * 16, st.cuda_stream)
    assert a["net_wgs_started"] == a["net_wgs"] and b["net_wgs_started"] == b["net_wgs"] and b["net_wgs"] >= a["net_wgs"]


def test_in_epoch_answer_table_is_transparent_and_saves_evaluations(monkeypatch):
    """round 4: the reference inserts an answer into the position cache the moment it arrives (PlayManager::update_inferences,
    play_manager.cc:631-640); the pipeline's S3-FIFO inserts wait for the epoch boundary, so the net workgroups also drop every answer
    into a direct-mapped table of self-validating granules {tag32(key, k) | float} that the tree side probes beside the S3-FIFO shard.
    With long epochs it answers probes (fewer evaluations than without it), and the games do not change (the lock-step engine's)."""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=31), spec)
    S, seed = 256, 4711
    pp = _selfplay_params(az, S, 120, cache=1 << 16)
    pa, (ra, ca), stats = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 600)
    assert stats["answer_table_hits"] > 0
    monkeypatch.setenv("AZMI_PIPE_NO_L0", "1")
    pn, (rn, cn), stats_n = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 600)
    monkeypatch.delenv("AZMI_PIPE_NO_L0")
    assert stats_n["answer_table_hits"] == 0
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pa.games_completed() == pn.games_completed() == pb.games_completed() == S
    sa, sn, sb = _sorted_log(ra, ca), _sorted_log(rn, cn), _sorted_log(rb, cb)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert np.array_equal(sn[0], sb[0]) and np.array_equal(sn[1], sb[1])
    xa, xn = pa.counters(), pn.counters()
    assert xa["sims"] == xn["sims"] and xa["evals"] < xn["evals"]
    assert xa["cache_hits"] + xa["cache_misses"] == xn["cache_hits"] + xn["cache_misses"]      # same probes, more of them answered


def test_a_request_the_net_side_cannot_read_is_given_up_and_sent_again(monkeypatch, capfd):
    """round 4: once in ~1e10 requests a net workgroup was found waiting at a ring position two laps behind the tail (it had been
    switched out; its request was overwritten a lap later) - and it waited until the stall cap.  Now a position more than half a ring
    behind the tail is given up, the slot stays unanswered, k_pipe_settle puts it back into the move step's kSlotQueued form and the
    next epoch sends the request again: no stall, no error, same games.  The hook writes ONE request (ring position 3000) with a
    foreign lap tag - what an overwritten entry looks like."""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=17), spec)
    S, seed = 512, 321
    pp = _selfplay_params(az, S, 150, cache=0)            # no cache: every leaf is a request, the tail moves fast
    monkeypatch.setenv("AZMI_PIPE_TEST_DROP", "3000")
    pa, (ra, ca), stats = _pipeline_games(az, pp, seed, hip, sims_per_epoch=S * 256)
    monkeypatch.delenv("AZMI_PIPE_TEST_DROP")
    assert "given up by the net side and sent again" in capfd.readouterr().err
    pb, (rb, cb) = _lockstep_games(az, pp, seed, hip)
    assert pa.games_completed() == pb.games_completed() == S
    sa, sb = _sorted_log(ra, ca), _sorted_log(rb, cb)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])


def test_the_default_library_has_no_conveyor_and_says_so(monkeypatch):
    """the conveyor (round 5's weight-stationary net side, a measured loser) was removed; the library answers
    AZMI_PIPE_NET=conveyor with an error by name instead of silently running the tiles"""
    import alphazero as az
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    hip = az.HipLeafNet(torch_net.random_init(spec, seed=4), spec)
    pp = _selfplay_params(az, 64, 20, cache=1 << 10)
    pm = az.PlayManager(az.Connect4GS(), pp, seed=3)
    st = torch.cuda.Stream()
    monkeypatch.setenv("AZMI_PIPE_NET", "conveyor")
    with pytest.raises(RuntimeError, match="no conveyor"):
        az.run_pipeline(pm, hip, 1, 64 * 8, st.cuda_stream)
    monkeypatch.delenv("AZMI_PIPE_NET")
    az.run_pipeline(pm, hip, 1, 64 * 8, st.cuda_stream)          # the engine is whole: the tile kernel carries on
