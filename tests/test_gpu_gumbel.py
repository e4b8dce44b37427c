"""Gumbel root search on the device (tg_sp_gumbel, k_collect_gumbel, k_gumbel_move, k_play_gumbel) against the oracle search with
the same rule (tests/gumbel_ref.py, written with the definition in transgo_amd/gumbel.py), on the same seeds: everything compared
is bit-identical.

The oracle games and the engine runs are computed once and shared.  tests/test_gumbel_host.py holds the condition on the inputs
(m = 16 really changes the search for `sharp`, seed 500) on the CPU."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import evaluators

R = 4
CASES = {                                   # name -> (evaluator, board, games, simulations, m, moves, max_step, first seed)
    "sharp9": ("sharp", 9, 8, 64, 16, 6, 6, 500),         # max_step = 6: the games end with their sixth move and are harvested
    "flat9": ("flat", 9, 8, 64, 16, 6, 6, 500),
    "sharp19": ("sharp", 19, 2, 32, 8, 2, 450, 700),      # 362 children: the multi-pass child loops
    "wide9": ("sharp", 9, 2, 24, 128, 3, 120, 510),       # m larger than any child count: every child is considered
    "tiny9": ("flat", 9, 2, 8, 16, 3, 120, 520),          # n < m_eff: the budget ends inside the first phase
}


def _seeds(case):
    G, s0 = CASES[case][2], CASES[case][7]
    return np.arange(s0, s0 + G).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(case, m=None, noised=None, sims=None):
    from tests.gumbel_ref import play_moves
    name, S, G, n, m0, moves, max_step, _ = CASES[case]
    games, sel, fb = [], 0, 0
    for g, s in enumerate(_seeds(case)):
        mv, o = play_moves(evaluators.BY_NAME[name], int(s), m0 if m is None else m, moves, n if sims is None else sims[g], board_size=S,
                           max_step=max_step, readouts=R, selfplay=True if noised is None else bool(noised[g]))
        games.append(mv); sel += o.root_selections; fb += o.fallback_selections
    return dict(games=games, stats=dict(root_selections=sel, fallback_selections=fb))


def _engine(case, **kw):
    from transgo_amd.engine import SelfPlayEngine
    name, S, G, sims, _, _, max_step, _ = CASES[case]
    return SelfPlayEngine(G, board_size=S, num_simulation=sims, parallel_readouts=R, max_step=max_step, evaluator=evaluators.BY_NAME[name], **kw)


def _move(eng, search):
    """One searched move of every game; `search` issues the search.  Returns what the move looked like, the move played."""
    live = ~eng.finished
    search()
    raw, _, _, st, _ = eng.root_info(obs=False)
    gl = eng.gumbel_table() if eng.gumbel_m > 0 else None
    acts, pis, gg = eng.choose_gumbel_moves(raw, st) if eng.gumbel_m > 0 else (*eng.choose_moves(raw, st), np.zeros(eng.G, bool))
    done = eng.play(acts)
    assert not eng.gumbel_moves()[1].any()                 # the flag ended with the move
    ch = eng.root_children()
    return dict(live=live, raw=raw, gl=gl, gg=gg, acts=acts, pis=pis, done=done, new_root_n=ch["root_n"],
                pos=np.array([eng.rng_state(g)[1] for g in range(eng.G)]), streams=eng.rng_streams())


def _hist(eng):
    from transgo_amd import snapshot
    snap = eng.snapshot()
    return snapshot.section(snap, snapshot.parse_header(snap), "hist_cnt", np.int32).reshape(-1, eng.A).copy()


@functools.lru_cache(maxsize=None)
def _run(case):
    _, S, G, _, m, moves, _, _ = CASES[case]
    eng = _engine(case, gumbel_m=m)
    assert eng.get_gumbel() == (m, 50.0, 1.0)
    eng.reset(_seeds(case))
    out, harvests = [], []
    for _ in range(moves):
        if eng.finished.all():
            break
        mv = _move(eng, lambda: eng.search(True))
        out.append(mv)
        if (mv["done"] & mv["live"]).any():
            harvests.append(eng.harvest(device=False, seeds=_seeds(case)))
    hist = _hist(eng)
    stats, errors = eng.gumbel_stats(), eng.stats()["errors"]
    eng.close()
    return dict(moves=out, harvests=harvests, hist=hist, stats=stats, errors=errors)


def _compare(run, games, noised=None):
    """Every way the engine's moves differ from the oracle's games (empty = equal)."""
    bad = []
    for m, mv in enumerate(run["moves"]):
        for g in np.flatnonzero(mv["live"]):
            if m >= len(games[g]):
                bad.append((g, m, "the oracle's game is over")); continue
            om = games[g][m]
            gum = noised is None or bool(noised[g])
            if not np.array_equal(mv["raw"][g], om["raw"]):
                bad.append((g, m, "raw root visits"))
            if gum and not np.array_equal(mv["gl"][g], om["gl"]):
                bad.append((g, m, "gl table"))
            if int(mv["acts"][g]) != om["action"]:
                bad.append((g, m, "action"))
            if not np.array_equal(mv["pis"][g], om["pi"]):
                bad.append((g, m, "pi"))
            if int(mv["pos"][g]) != om["pos"]:
                bad.append((g, m, "MT19937 stream position"))
            if bool(mv["gg"][g]) != gum:
                bad.append((g, m, "gumbel_game flag"))
    return bad


def _check_case(case, n_moves):
    run, orc = _run(case), _oracle(case)
    assert run["errors"] == 0 and len(run["moves"]) == n_moves
    assert _compare(run, orc["games"]) == []
    assert run["stats"] == orc["stats"] and orc["stats"]["root_selections"] > 0
    return run, orc


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sharp9", "flat9"])
def test_gumbel_search_against_the_oracle_9x9(case):
    """8 games, 64 simulations, m = 16, 6 moves: raw visits, the gl table, moves, pi', stream positions and both counters are the
    oracle twin's; the harvested counts are the fixed-point targets."""
    run, orc = _check_case(case, 6)
    games, seen = orc["games"], set()
    for h in run["harvests"]:
        cnt, nm = h.view("counts").reshape(-1, 82), h.view("n_moves")
        o = 0
        for i, g in enumerate(h.view("slot")):
            want = np.array([m["record"] for m in games[int(g)]], np.int32)
            assert int(nm[i]) == len(want) and np.array_equal(cnt[o:o + len(want)], want), int(g)
            o += len(want); seen.add(int(g))
    assert seen == set(range(8))
    for mv in run["moves"]:                                 # only considered children gained visits
        assert ((mv["gl"] > -np.inf).sum(1)[mv["live"]] == 16).all()


@pytest.mark.gpu
def test_gumbel_search_against_the_oracle_19x19():
    """19x19 (6 passes over the children), 2 games, 32 simulations, m = 8, 2 moves; the counts k_play_gumbel recorded (read from a
    snapshot: the games are still running) are the fixed-point targets."""
    run, orc = _check_case("sharp19", 2)
    want = np.array([m["record"] for g in orc["games"] for m in g], np.int32)
    assert np.array_equal(run["hist"], want)


@pytest.mark.gpu
def test_m_larger_than_the_child_count():
    run, orc = _check_case("wide9", 3)
    for m, mv in enumerate(run["moves"]):
        for g in range(2):
            assert (mv["gl"][g] > -np.inf).sum() == orc["games"][g][m]["nchild"] < 128


@pytest.mark.gpu
def test_budget_smaller_than_the_considered_set():
    """n = 8 < m_eff = 16: v(t) = 0 at every step, a wave's overshoot included, so in the first move (a fresh tree) every
    simulation goes to another considered child."""
    run, orc = _check_case("tiny9", 3)
    first = run["moves"][0]["raw"]
    assert (first <= 1).all() and ((first.sum(1) >= 8) & (first.sum(1) < 8 + R)).all()


@pytest.mark.gpu
def test_mixed_batch_of_gumbel_and_plain_games():
    """tg_sp_begin_move_games with half the games noised: the games without noise are bit-identical to the same games in an engine
    with m = 0, the noised ones match the oracle twin."""
    case = "sharp9"
    _, S, G, sims, M, _, _, _ = CASES[case]
    nz = np.array([g % 2 == 0 for g in range(G)])
    budget = np.where(nz, sims, 24)

    def run(m, moves=3):
        eng = _engine(case, gumbel_m=m)
        eng.reset(_seeds(case))
        out = [_move(eng, lambda: eng.search(True, budget, noise=nz, record=nz)) for _ in range(moves)]
        hist = _hist(eng)
        eng.close()
        return out, hist
    (gum, hg), (plain, hp) = run(M), run(0)
    fast = ~nz
    for a, b in zip(gum, plain):
        assert not b["gg"].any() and np.array_equal(a["gg"], nz & a["live"])
        for key in ("raw", "acts", "pis", "pos", "new_root_n"):
            assert np.array_equal(a[key][fast], b[key][fast]), key
        assert np.array_equal(a["streams"][fast], b["streams"][fast])
    A = S * S + 1
    assert np.array_equal(hg.reshape(G, -1, A)[fast, :3], hp.reshape(G, -1, A)[fast, :3])
    assert any(not np.array_equal(a["raw"][nz], b["raw"][nz]) for a, b in zip(gum, plain))
    twins = _oracle(case)["games"]
    for m, mv in enumerate(gum):
        for g in np.flatnonzero(nz):
            om = twins[g][m]
            assert np.array_equal(mv["raw"][g], om["raw"]) and np.array_equal(mv["gl"][g], om["gl"]), (g, m)
            assert int(mv["acts"][g]) == om["action"] and int(mv["pos"][g]) == om["pos"] and np.array_equal(mv["pis"][g], om["pi"]), (g, m)


@pytest.mark.gpu
def test_off_is_off():
    """m never set, set to 0, and set then cleared: identical visits, moves, streams and records over 4 moves."""
    case = "sharp9"

    def run(prepare):
        eng = _engine(case)
        prepare(eng)
        eng.reset(_seeds(case))
        out = []
        for _ in range(4):
            eng.search(True)
            vis, st = eng.root_visits()
            assert not eng.gumbel_moves()[1].any() and (eng.gumbel_moves()[0] == -1).all()
            acts, pis = eng.choose_moves(vis, st)
            eng.play(acts)
            out.append((vis.tobytes(), acts.tobytes(), pis.tobytes(), eng.rng_streams().tobytes()))
        out.append(_hist(eng).tobytes())
        out.append(eng.gumbel_stats())
        eng.close()
        return out
    a = run(lambda e: e.set_gumbel(0))
    b = run(lambda e: None)
    c = run(lambda e: (e.set_gumbel(16), e.set_gumbel(0)))
    assert a == b == c and a[-1] == dict(root_selections=0, fallback_selections=0)
    # ... and they are the plain oracle's games
    orc = _oracle(case, m=0)["games"]
    vis0 = np.frombuffer(b[0][0], np.int32).reshape(8, 82)
    assert all(np.array_equal(vis0[g], orc[g][0]["raw"]) for g in range(8))


@pytest.mark.gpu
def test_argument_and_state_refusals():
    from transgo_amd import _lib
    eng = _engine("sharp9")
    for bad in ((-1, 50.0, 1.0), (4, float("nan"), 1.0), (4, 50.0, float("inf"))):
        with pytest.raises(_lib.TransgoError, match="tg_sp_gumbel"):
            eng.ctx.call("tg_sp_gumbel", bad[0], ctypes.c_double(bad[1]), ctypes.c_double(bad[2]))
    with pytest.raises(ValueError, match="gumbel_m"):
        eng.set_gumbel(-3)
    buf = np.zeros((eng.G, eng.A), np.int32)
    with pytest.raises(_lib.TransgoError, match="tg_sp_reset"):
        eng.ctx.call("tg_sp_gumbel_move", buf.ctypes.data_as(ctypes.c_void_p), None)
    eng.reset(_seeds("sharp9"))
    with pytest.raises(_lib.TransgoError, match="is off"):
        eng.stage_gumbel_targets(buf, np.ones(eng.G, bool))
    # forced playouts and Gumbel refuse each other, whichever comes second
    eng.set_forced_playouts(2.0)
    with pytest.raises(_lib.TransgoError, match="forced playouts are on"):
        eng.set_gumbel(8)
    assert eng.get_gumbel()[0] == 0
    eng.set_gumbel(0)                                       # switching off is always allowed
    eng.set_forced_playouts(0.0)
    eng.set_gumbel(8, 40.0, 0.5)
    assert eng.get_gumbel() == (8, 40.0, 0.5)
    with pytest.raises(_lib.TransgoError, match="Gumbel root search is on"):
        eng.set_forced_playouts(2.0)
    assert eng.get_forced_playouts() == 0.0
    eng.set_forced_playouts(0.0)
    eng.ctx.call("tg_sp_begin_move", 1, 0)
    act, rows = ctypes.c_int32(), ctypes.c_int32()
    eng.ctx.call("tg_sp_collect", ctypes.byref(act), ctypes.byref(rows))
    assert rows.value > 0
    with pytest.raises(_lib.TransgoError, match="batch is pending"):
        eng.ctx.call("tg_sp_gumbel", 4, ctypes.c_double(50.0), ctypes.c_double(1.0))
    assert eng.get_gumbel() == (8, 40.0, 0.5)
    eng._evaluate(rows.value)
    eng.ctx.call("tg_sp_absorb")
    eng.close()


@pytest.mark.gpu
def test_masked_reset_ends_the_gumbel_move_of_the_restarted_slots_only():
    case = "sharp9"
    eng = _engine(case, gumbel_m=16)
    eng.reset(_seeds(case))
    eng.search(True)
    before, gg = eng.gumbel_moves()
    assert gg.all() and (before >= 0).all()
    mask = np.zeros(eng.G, bool); mask[[0, 3]] = True
    eng.reset(_seeds(case), mask)
    after, gg = eng.gumbel_moves()
    assert np.array_equal(gg, ~mask) and np.array_equal(after[~mask], before[~mask]) and (after[mask] == -1).all()
    eng.close()


@pytest.mark.gpu
def test_the_new_root_keeps_the_chosen_childs_visits():
    run, games = _run("sharp9"), _oracle("sharp9")["games"]
    checked = 0
    for m, mv in enumerate(run["moves"]):
        for g in np.flatnonzero(mv["live"] & ~mv["done"]):
            a = int(mv["acts"][g])
            assert int(mv["new_root_n"][g]) == int(mv["raw"][g, a]) == games[g][m]["child_n"] == games[g][m]["new_root_n"], (g, m)
            checked += 1
    assert checked == 8 * 5


@pytest.mark.gpu
def test_batched_self_play_applies_the_rule_on_full_plies_only():
    from transgo_amd import playout_cap
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    cfg = Config(num_simulation=48, max_step=8, playout_cap_p_full=0.5, playout_cap_fast=16, playout_cap_seed=0, gumbel_m=8)
    sp = BatchedSelfPlay(cfg, 8, evaluator=evaluators.sharp)
    sp.start()
    eng, seen = sp.engine, []
    choose = eng.choose_gumbel_moves

    def spy(vis, steps, selfplay=True):
        before = eng.rng_streams()
        out = choose(vis, steps, selfplay)
        seen.append((out[2], out[0].copy(), eng.gumbel_moves()[0], before, eng.rng_streams()))
        return out
    eng.choose_gumbel_moves = spy
    assert eng.get_gumbel()[0] == 8
    harvested = 0
    for _ in range(10):
        live = ~eng.finished
        full = playout_cap.schedule(sp.seeds, eng.root_plies(), 0.5, 0) & live
        h = sp.advance()
        gg, acts, gact, s0, s1 = seen[-1]
        assert np.array_equal(gg, full) and np.array_equal(acts[gg], gact[gg])
        assert np.array_equal(s0[gg], s1[gg])                           # a Gumbel game's stream is not touched at move time
        assert all(not np.array_equal(s0[g], s1[g]) for g in np.flatnonzero(live & ~gg))
        harvested += 0 if h is None else h.n_positions
    assert harvested > 0 and 0 < sp.full_moves < sp.moves_played and eng.stats()["errors"] == 0
    state, snap = sp.checkpoint_state(), eng.snapshot()
    eng.set_gumbel(0)
    sp._restore_part(state, snap)
    assert eng.get_gumbel()[0] == 8
    eng.close()


@pytest.mark.gpu
def test_wp_mcts_returns_the_twins_action_and_improved_policy():
    from transgo_amd.configure import Config
    from transgo_amd.self_play import WP_MCTS
    name, S, G, sims, M, moves, max_step, s0 = CASES["sharp9"]
    game = _oracle("sharp9")["games"][0]
    mcts = WP_MCTS(Config(num_simulation=sims, max_step=max_step, gumbel_m=M), seed=s0, evaluator=evaluators.BY_NAME[name])
    done = False
    for m, om in enumerate(game):
        a, pi, _ = mcts.get_action_probs()
        assert a == om["action"] and np.array_equal(pi, om["pi"]), m
        done = mcts.update_with_action(a)
    assert done
    h = mcts.engine.harvest(device=False)
    assert np.array_equal(h.view("counts").reshape(-1, 82), np.array([om["record"] for om in game], np.int32))
    mcts.close()
