"""Playout cap randomization on the device: per-game budgets, noise and record switches (tg_sp_begin_move_games), the marked
plies in the games' records, the compacting harvest -- against the oracle search driven by the same schedule.

The oracle side is computed once per (cap seed) and shared; so is the engine's run.  The budgets are small (48 / 16 simulations),
so the evaluator has to be peaked enough that a fast search still visits some root child twice: the reference's
counts == 1 -> 0 step makes np.random.choice raise otherwise (engine.py documents its own deviation for that case).
test_oracle_plays_every_game_without_raising holds that condition on the CPU."""
import functools

import numpy as np
import pytest

from oracle import evaluators

G, R, FULL, FAST, MAX_STEP, P_FULL, CAP_SEED, OTHER_CAP_SEED = 12, 4, 48, 16, 14, 0.5, 0, 1
EV = evaluators.sharp              # `spike` and `flat` leave some fast search without a twice-visited root child at these seeds; `sharp` none
SEEDS = np.arange(300, 300 + G).astype(np.uint32)
A = 82


# ---- the oracle side -------------------------------------------------------------------------------------------------------------
def _oracle_game(seed, cap_seed):
    """One game of OracleSearch under the schedule of (seed, cap_seed): per move the kind, n0, the raw root counts, the action, the
    root's observation and side to move; the final state and the final MT19937 stream."""
    from oracle.go_oracle import OracleGoEnv
    from oracle.wp_mcts import OracleSearch, temperature
    from transgo_amd import playout_cap
    env = OracleGoEnv(max_step=MAX_STEP)
    rng = np.random.RandomState(int(seed))
    o = OracleSearch(env, EV, rng, num_simulation=FULL, parallel_readouts=R)
    moves, done, ply = [], False, 0
    while not done:
        full = bool(playout_cap.schedule(int(seed), ply, P_FULL, cap_seed))
        o.num_simulation = FULL if full else FAST
        if full:
            o.root.add_root_noise(rng)
        n0 = o.root.n
        while o.root.n < n0 + o.num_simulation:
            o.wave()
        raw = np.array([o.root.kids[a].n if a in o.root.kids else 0 for a in range(A)])
        counts = np.where(raw == 1, 0, raw)
        if counts.sum() == 0:
            raise ValueError(f"seed {seed} ply {ply}: no root child has two visits (np.random.choice would raise)")
        pi = counts / np.sum(counts)
        powed = np.power(counts, 1.0 / temperature(env.getStep(o.root.state)))       # the self-play temperature on both kinds
        action = rng.choice(np.arange(A), p=np.array(powed) / np.sum(powed))
        moves.append(dict(full=full, n0=n0, root_n=o.root.n, raw=raw, pi=pi, action=int(action), obs=env.encode(o.root.state),
                          player=int(env.getPlayer(o.root.state))))
        done = o.advance(action)
        ply += 1
    st = rng.get_state()
    return dict(moves=moves, final=o.root.state, env=env, key=np.asarray(st[1], np.uint32), pos=int(st[2]))


@functools.lru_cache(maxsize=None)
def _oracle(cap_seed):
    return [_oracle_game(s, cap_seed) for s in SEEDS]


def test_oracle_plays_every_game_without_raising():
    """The condition on the inputs (CPU, oracle only): with this evaluator and these budgets the reference's own move selection
    never meets an all-zero count vector, under the schedule of the test and under the negative control's; and the schedule
    really mixes the kinds, with a full move behind a fast one somewhere (test 5)."""
    for cap in (CAP_SEED, OTHER_CAP_SEED):
        games = _oracle(cap)
        assert len(games) == G and all(1 <= len(g["moves"]) <= MAX_STEP for g in games)
    kinds = [[m["full"] for m in g["moves"]] for g in _oracle(CAP_SEED)]
    flat = [k for ks in kinds for k in ks]
    assert 0 < sum(flat) < len(flat)
    assert any(not a and b for ks in kinds for a, b in zip(ks, ks[1:]))
    assert kinds != [[m["full"] for m in g["moves"]] for g in _oracle(OTHER_CAP_SEED)]


# ---- the engine's side -----------------------------------------------------------------------------------------------------------
def _engine(**kw):
    from transgo_amd.engine import SelfPlayEngine
    return SelfPlayEngine(G, num_simulation=FULL, parallel_readouts=R, max_step=MAX_STEP, evaluator=EV, **kw)


def _capped_move(eng, record=True):
    """One searched move of every game under the schedule; returns what the move looked like."""
    from transgo_amd import playout_cap
    live = ~eng.finished
    full = playout_cap.schedule(SEEDS, eng.root_plies(), P_FULL, CAP_SEED)
    _, n0, _, _, _ = eng.root_info(obs=False)
    eng.search(True, np.where(full, FULL, FAST), noise=full, record=full if record else None)
    vis, rn, pl, st, ob = eng.root_info()
    acts, pis = eng.choose_moves(vis, st)
    return dict(live=live, full=full, n0=n0, root_n=rn, vis=vis, acts=acts, pis=pis, obs=ob, player=pl)


@functools.lru_cache(maxsize=None)
def _engine_run():
    """All twelve games to their end under the schedule of CAP_SEED: the moves, each game's stream when it finished, the harvests."""
    eng = _engine()
    eng.reset(SEEDS)
    moves, streams, harvests = [], {}, []
    for _ in range(MAX_STEP + 1):
        if eng.finished.all():
            break
        mv = _capped_move(eng)
        moves.append(mv)
        done = eng.play(mv["acts"])
        for g in np.flatnonzero(done & mv["live"]):
            streams[int(g)] = eng.rng_state(int(g))
        if (done & mv["live"]).any():
            harvests.append(eng.harvest(device=False, seeds=SEEDS))
    errors = eng.stats()["errors"]
    eng.close()
    return dict(moves=moves, streams=streams, harvests=harvests, errors=errors)


def _mismatches(run, games):
    """Comparison 1: every way the engine's run differs from the oracle's games (empty = equal)."""
    from oracle.wp_mcts import targets_for_game
    bad = []
    played = [0] * G
    for m, mv in enumerate(run["moves"]):
        for g in np.flatnonzero(mv["live"]):
            if m >= len(games[g]["moves"]):
                bad.append((g, m, "the oracle's game is over")); continue
            om = games[g]["moves"][m]
            played[g] += 1
            if bool(mv["full"][g]) != om["full"]:
                bad.append((g, m, "kind"))
            if not np.array_equal(mv["vis"][g], om["raw"]):
                bad.append((g, m, "root visit counts"))
            if int(mv["acts"][g]) != om["action"]:
                bad.append((g, m, "action"))
            if not np.array_equal(mv["obs"][g], om["obs"]) or int(mv["player"][g]) != om["player"]:
                bad.append((g, m, "root position"))
    for g in range(G):
        if played[g] != len(games[g]["moves"]) or g not in run["streams"]:
            bad.append((g, -1, "game length")); continue
        key, pos = run["streams"][g]
        if pos != games[g]["pos"] or not np.array_equal(key, games[g]["key"]):
            bad.append((g, -1, "final MT19937 stream"))
    seen = set()
    for h in run["harvests"]:
        tup, cnt, pl, nm = h.targets(), h.view("counts"), h.view("player"), h.view("n_moves")
        if (pl & 0x80).any():
            bad.append((-1, -1, "a player byte carries the mark"))
        o = 0
        for i, g in enumerate(h.view("slot")):
            g = int(g); seen.add(g)
            fm = [m for m in games[g]["moves"] if m["full"]]
            if int(nm[i]) != len(fm):
                bad.append((g, -1, "n_moves")); break
            want = targets_for_game(games[g]["env"], games[g]["final"], [m["obs"] for m in fm], [m["pi"] for m in fm],
                                    [m["player"] for m in fm])
            got = tup[8 * o:8 * (o + len(fm))]
            if len(got) != len(want) or not all(all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(got, want)):
                bad.append((g, -1, "harvested targets (obs, pi, z, own)"))
            if not np.array_equal(cnt[o:o + len(fm)], np.array([m["raw"] for m in fm], np.int32).reshape(-1, A)):
                bad.append((g, -1, "harvested raw counts"))
            if [int(x) for x in pl[o:o + len(fm)]] != [m["player"] for m in fm]:
                bad.append((g, -1, "harvested players"))
            o += len(fm)
        if o != h.n_positions:
            bad.append((-1, -1, "n_positions"))
    if seen != set(range(G)):
        bad.append((-1, -1, "not every game was harvested"))
    return bad


@pytest.mark.gpu
def test_mixed_budgets_against_the_oracle():
    """1. p_full = 0.5: per game and move the root visit counts, the chosen action and the root position; per game the final MT19937
    stream; the harvest holds exactly the full plies, in order -- obs bits, pi, z, own (the oracle's targets_for_game of the full
    plies), raw counts, players without the mark, n_moves = the number of full plies."""
    run = _engine_run()
    assert run["errors"] == 0
    assert _mismatches(run, _oracle(CAP_SEED)) == []


@pytest.mark.gpu
def test_negative_control_another_cap_seed_fails_the_comparison():
    """6. The oracle driven by the schedule of another cap seed plays other games: comparison 1 must notice."""
    bad = _mismatches(_engine_run(), _oracle(OTHER_CAP_SEED))
    assert bad and any(what == "kind" for _, _, what in bad)


@pytest.mark.gpu
def test_tree_reuse_across_kinds():
    """5. A full move behind a fast one starts from root.n of the sub-tree the fast move kept, and its target is that + N: the root
    count before the search equals the oracle's n0, the one after it the oracle's (first wave that reaches n0 + N)."""
    run, games = _engine_run(), _oracle(CAP_SEED)
    checked = 0
    for m, mv in enumerate(run["moves"]):
        for g in np.flatnonzero(mv["live"]):
            om = games[g]["moves"][m]
            assert int(mv["n0"][g]) == om["n0"] and int(mv["root_n"][g]) == om["root_n"], (g, m)
            budget = FULL if om["full"] else FAST
            assert om["n0"] + budget <= int(mv["root_n"][g]) < om["n0"] + budget + 2 * R, (g, m)
            if m > 0 and om["full"] and not games[g]["moves"][m - 1]["full"] and om["n0"] > 0:
                checked += 1
    assert checked > 0


@pytest.mark.gpu
def test_cap_off_is_the_parent():
    """2. search() with all-ones masks and a constant budget is tg_sp_begin_move: byte-identical harvests over a whole generation;
    and a BatchedSelfPlay with the default Config never calls the new entry point."""
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay

    def generation(per_game):
        eng = _engine()
        eng.reset(SEEDS)
        out = []
        for _ in range(MAX_STEP + 1):
            if eng.finished.all():
                break
            if per_game:
                eng.search(True, np.full(G, FULL), noise=np.ones(G, bool), record=np.ones(G, bool))
            else:
                eng.search(True, FULL)
            vis, st = eng.root_visits()
            acts, _ = eng.choose_moves(vis, st)
            out.append(vis.tobytes())
            if eng.play(acts).any():
                out.append(eng.harvest(device=False, seeds=SEEDS).buf.tobytes())
        out.append(eng.rng_streams().tobytes())
        eng.close()
        return out
    a, b = generation(False), generation(True)
    assert len(a) == len(b) > MAX_STEP // 2 and a == b
    sp = BatchedSelfPlay(Config(num_simulation=16, max_step=5), 6, evaluator=EV)
    names, call = [], sp.engine.ctx.call
    sp.engine.ctx.call = lambda name, *args: (names.append(name), call(name, *args))[1]
    got = [sp.advance() for _ in range(6)]
    assert any(h is not None for h in got)
    assert "tg_sp_begin_move" in names and "tg_sp_begin_move_games" not in names
    sp.engine.close()


@pytest.mark.gpu
def test_all_fast_games_finish_restart_and_feed_an_empty_harvest():
    """3. p_full close to 0: games finish and restart, a game without a full ply is listed with n_moves = 0, a harvest without any
    position goes through the device replay store, and nothing errs."""
    from transgo_amd import playout_cap
    from transgo_amd.configure import Config
    from transgo_amd.replay_buffer import DeviceReplayMemory
    from transgo_amd.self_play import BatchedSelfPlay
    store = DeviceReplayMemory(Config(buffer_size=8 * 1024), capacity_positions=1024)
    zero_games = empty_harvests = 0
    for p in (0.04, 1e-6):
        cfg = Config(num_simulation=FULL, max_step=8, playout_cap_p_full=p, playout_cap_fast=FAST, playout_cap_seed=3, buffer_size=8 * 1024)
        sp = BatchedSelfPlay(cfg, G, evaluator=EV)
        names, call = [], sp.engine.ctx.call
        sp.engine.ctx.call = lambda name, *args: (names.append(name), call(name, *args))[1]
        sp.start()
        full_plies = np.zeros(G, np.int64)                            # what the schedule says each slot's running game has recorded
        positions = 0
        for _ in range(17):                                           # two generations and a move
            full = playout_cap.schedule(sp.seeds, sp.engine.root_plies(), p, 3)
            full_plies += full
            h = sp.advance(device=True)
            if h is None:
                continue
            assert h.on_device
            host = h.to_host()
            slots, nm = host.view("slot"), host.view("n_moves")
            assert np.array_equal(nm, full_plies[slots]) and h.n_positions == int(nm.sum())
            assert not (host.view("player") & 0x80).any() and len(host.records()) == h.n_games
            zero_games += int((nm == 0).sum())
            empty_harvests += int(h.n_positions == 0)
            before = store.info()["entries"]
            store.append_harvest(h)
            assert store.info()["entries"] == before + 8 * h.n_positions
            positions += h.n_positions
            full_plies[slots] = 0
        assert sp.games_finished >= 2 * G and (sp.games_started >= 3).all() and sp.games_dropped == 0     # finished and restarted
        assert positions == sp.full_moves - int(full_plies.sum())     # what was recorded and harvested = the full moves of finished games
        assert "tg_sp_begin_move_games" in names and "tg_sp_begin_move" not in names
        assert sp.engine.stats()["errors"] == 0
        sp.engine.close()
    assert zero_games > 0 and empty_harvests > 0
    store.close()


@pytest.mark.gpu
def test_snapshot_mid_game_carries_the_marks():
    """4. A snapshot taken after some marked plies: the restored worker continues bit for bit and harvests the same filtered
    positions; the snapshot is as large as that of a run with the same trees and no mark."""
    from transgo_amd import snapshot
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    cfg = Config(num_simulation=FULL, max_step=MAX_STEP, playout_cap_p_full=P_FULL, playout_cap_fast=FAST, playout_cap_seed=CAP_SEED)
    seed_fn = lambda g, k: int(SEEDS[g]) + 1000 * k

    def play(sp, n):
        out = []
        for _ in range(n):
            h = sp.advance()
            out.append((sp.engine.root_visits()[0].tobytes(), sp.engine.rng_streams().tobytes(),
                        None if h is None else h.to_host().buf.tobytes()))
        return out
    a = BatchedSelfPlay(cfg, G, evaluator=EV, seed_fn=seed_fn)
    play(a, 6)
    snap, state = a.engine.snapshot(), a.checkpoint_state()
    hdr = snapshot.parse_header(snap)
    marks = snapshot.section(snap, hdr, "hist_pl")
    assert (marks & 0x80).any() and not (marks & 0x80).all() and set(np.unique(marks & 0x7f)) <= {1, 2}
    b = BatchedSelfPlay(cfg, G, evaluator=EV, seed_fn=seed_fn)
    b._restore_part(state, snap)
    after = MAX_STEP + 2                                              # past the end of the generation: the marked plies are harvested
    la, lb = play(a, after), play(b, after)
    assert la == lb and any(h is not None for _, _, h in la)
    assert a.full_moves > 0 and a.games_finished == b.games_finished >= G
    # the same searches with every ply recorded: the same trees, a snapshot of the same size, other bytes in hist_pl only
    eng = _engine()
    eng.reset(SEEDS)
    for _ in range(6):
        eng.play(_capped_move(eng, record=False)["acts"])
    plain = eng.snapshot()
    assert len(plain) == len(snap)
    ph = snapshot.parse_header(plain)
    assert ph["sections"] == hdr["sections"] and not (snapshot.section(plain, ph, "hist_pl") & 0x80).any()
    assert np.array_equal(snapshot.section(plain, ph, "hist_pl"), marks & 0x7f)
    for k in ("hist_obs", "hist_cnt", "rng", "moves"):
        assert np.array_equal(snapshot.section(plain, ph, k), snapshot.section(snap, hdr, k)), k
    for e in (a.engine, b.engine, eng):
        e.close()
