"""Search ownership on the device (tg_sp_search_ownership, k_absorb_own, k_root_ownership) against the restatement of
tests/search_ownership_ref.py on the same seeds: mean, n and score lead are compared bit for bit after every move.

The restatement games and the engine runs are computed once and shared.  tests/test_search_ownership_host.py holds, on the CPU, what
the cases must contain (dropped duplicate leaves, terminal simulations, roots of both colours, reused sub-trees, a search that
completes only terminal simulations)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import evaluators
from tests import search_ownership_ref as so

pytestmark = pytest.mark.gpu
F32 = np.float32
RULE_KW = {"plain": ({}, {}), "forced": (dict(forced_k=2.0), dict(forced_playouts_k=2.0)), "gumbel": (dict(gumbel_m=8), dict(gumbel_m=8))}


@functools.lru_cache(maxsize=None)
def _oracle(case, own="tenths", rule="plain", invert=False):
    return [mv for mv, _, _ in so.play_case(case, own=own, rule=rule, invert_sign=invert, **RULE_KW[rule][0])]


def _engine(case, own="tenths", rule="plain", on=True, **kw):
    from transgo_amd.engine import SelfPlayEngine
    name, S, G, sims, _, max_step, _ = so.CASES[case]
    ev = so.with_own(name, so.OWN_BY_NAME[own]) if on else evaluators.BY_NAME[name]
    return SelfPlayEngine(G, board_size=S, num_simulation=sims, parallel_readouts=so.R, max_step=max_step, evaluator=ev,
                          search_ownership=on, **RULE_KW[rule][1], **kw)


def _choose(eng, rule):
    raw, _, _, st, _ = eng.root_info(obs=False)
    if rule == "forced":
        vis, st = eng.root_visits(pruned=True)
        return raw, eng.choose_moves(vis, st)[0]
    if rule == "gumbel":
        return raw, eng.choose_gumbel_moves(raw, st)[0]
    return raw, eng.choose_moves(raw, st)[0]


def _moves(eng, n, rule="plain"):
    """n searched moves of every game: per move the live mask, raw visits, the ownership read-out (None with the mode off), the
    moves played and every stream's position after the move."""
    out = []
    for _ in range(n):
        if eng.finished.all():
            break
        live = ~eng.finished
        eng.search(True)
        ro = eng.root_ownership() if eng.search_ownership else None
        raw, acts = _choose(eng, rule)
        eng.play(acts)
        out.append(dict(live=live, raw=raw, own=ro, acts=acts, pos=np.array([eng.rng_state(g)[1] for g in range(eng.G)])))
    return out


@functools.lru_cache(maxsize=None)
def _run(case, own="tenths", rule="plain", on=True):
    eng = _engine(case, own, rule, on)
    assert eng.get_search_ownership() == on
    eng.reset(so.case_seeds(case))
    out = _moves(eng, so.CASES[case][4], rule)
    errors = eng.stats()["errors"]
    eng.close()
    assert errors == 0
    return out


def _compare(run, games, S):
    """Every way the engine's moves differ from the restatement's games (empty = equal)."""
    bad = []
    for m, mv in enumerate(run):
        for g in np.flatnonzero(mv["live"]):
            if m >= len(games[g]):
                bad.append((g, m, "the restatement's game is over")); continue
            om = games[g][m]
            if not np.array_equal(mv["raw"][g], om["raw"]):
                bad.append((g, m, "raw root visits"))
            if int(mv["acts"][g]) != om["action"]:
                bad.append((g, m, "action"))
            if int(mv["pos"][g]) != om["pos"]:
                bad.append((g, m, "MT19937 stream position"))
            ro = mv["own"]
            if int(ro["n"][g]) != om["n"]:
                bad.append((g, m, f"n {int(ro['n'][g])} != {om['n']}"))
            if not np.array_equal(ro["mean"][g].reshape(-1).view(np.uint32), om["mean"].view(np.uint32)):
                bad.append((g, m, "mean"))
            if F32(ro["score_lead"][g]).view(np.uint32) != F32(om["score_lead"]).view(np.uint32):
                bad.append((g, m, "score_lead"))
    assert sum(len(g) for g in games) == sum(int(mv["live"].sum()) for mv in run), "the engine played fewer searched moves than the restatement"
    return bad


@pytest.mark.parametrize("own", ["tenths", "exact"])
def test_9x9_bit_identical_to_the_restatement(own):
    run, games = _run("flat9", own), _oracle("flat9", own)
    assert len(run) == 5 and run[0]["live"].all()
    assert _compare(run, games, 9) == []
    assert run[0]["own"]["mean"].dtype == np.float32 and run[0]["own"]["mean"].shape == (6, 9, 9)


def test_a_search_of_terminal_simulations_only_reads_zero():
    """flat9's fifth move: every simulation ends the game inside the collect stage, so nothing is absorbed."""
    run, games = _run("flat9"), _oracle("flat9")
    hit = 0
    for g in range(6):
        if games[g][4]["n"] == 0:
            ro = run[4]["own"]
            assert ro["n"][g] == 0 and not ro["mean"][g].any() and ro["score_lead"][g] == F32(-7.5)
            assert run[4]["raw"][g].sum() > 0                       # the search itself did run
            hit += 1
    assert hit >= 1


def test_the_mode_does_not_steer_the_search():
    on, off = _run("flat9"), _run("flat9", on=False)
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert b["own"] is None
        assert np.array_equal(a["raw"], b["raw"]) and np.array_equal(a["acts"], b["acts"]) and np.array_equal(a["pos"], b["pos"])


def test_19x19_bit_identical_to_the_restatement():
    """361 points: six strides of 64 lanes, the last a tail of 41."""
    run, games = _run("flat19"), _oracle("flat19")
    assert len(run) == 2
    assert _compare(run, games, 19) == []
    assert all(mv["own"]["n"].min() > 0 and mv["own"]["mean"][:, 18, 10:].any() for mv in run)      # the tail points are written


@pytest.mark.parametrize("rule", ["forced", "gumbel"])
def test_forced_and_gumbel_searches_share_the_absorb_stage(rule):
    run, games = _run("rule9", "tenths", rule), _oracle("rule9", "tenths", rule)
    assert _compare(run, games, 9) == []
    assert sum(int(mv["own"]["n"].sum()) for mv in run) > 0


def test_negative_control_inverted_sign_differs():
    """The restatement with contributions taken from the leaf mover's own side: the same searches, other means -- the comparator
    can fail on perspective."""
    run, wrong = _run("flat9"), _oracle("flat9", invert=True)
    bad = _compare(run, wrong, 9)
    assert bad and all(what in ("mean", "score_lead") for _, _, what in bad)
    assert sum(what == "mean" for _, _, what in bad) >= 6


# ---- real network ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["none", "position"])
def test_real_network_means_equal_the_restatement(mode):
    """Route taken: the bit-for-bit one.  It rests on the premise that the forward of a board does not depend on what else is in the
    batch (tests/test_gpu_half_attention.py and its siblings assert it; tests/test_gpu_symmetry.py's search-parity test relies on it
    the same way): the engine evaluates its 8 games' leaves in one batch with tg_sp_eval, the restatement evaluates each game's
    leaves alone through HipNetwork.main_prediction of the same weights in a second context (under "position" through the host
    wrapper symmetry.evaluate_with_symmetry).  Visit counts must be equal; then the ownership means must be equal bit for bit."""
    from oracle.go_oracle import OracleGoEnv
    from transgo_amd import model, symmetry
    from transgo_amd.engine import SelfPlayEngine
    G, sims, moves, seed = 8, 32, 2, 11
    sd = model.random_weights(9, 10, 32, 2, seed=23)
    eng = SelfPlayEngine(G, num_simulation=sims, parallel_readouts=so.R, net_blocks=2, net_filters=32, eval_symmetry=mode, symmetry_seed=seed,
                         search_ownership=True)
    model.load_into(eng.ctx, sd, 9, 10, 32, 2)
    hn = model.HipNetwork(9, 10, 32, 2, rows_cap=G * so.R)
    hn.set_weights(sd)

    def evaluate(obs):
        p, v, o = symmetry.evaluate_with_symmetry(hn.main_prediction, obs, mode, seed)
        return p, np.asarray(v, np.float32).reshape(-1, 1), o
    seeds = np.arange(G) + 100
    eng.reset(seeds)
    run = _moves(eng, moves)
    eng.close()
    games = []
    for s in seeds:
        mv, _ = so.play_moves(evaluate, int(s), moves, sims, readouts=so.R)
        games.append(mv)
    hn.ctx.close()
    for m, mv in enumerate(run):
        for g in range(G):
            assert np.array_equal(mv["raw"][g], games[g][m]["raw"]), f"visit counts differ, game {g} move {m}"
    assert _compare(run, games, 9) == []
    for mv in run:
        ro = mv["own"]
        assert (ro["n"] > 0).all()
        assert np.abs(ro["mean"]).max() <= 1.0 and all(ro["mean"][g].any() for g in range(G))


# ---- refusals and edges ---------------------------------------------------------------------------------------------------------

def _small(on, **kw):
    from transgo_amd.engine import SelfPlayEngine
    ev = so.with_own("flat", so.own_tenths) if on else evaluators.flat
    return SelfPlayEngine(2, num_simulation=16, parallel_readouts=so.R, evaluator=ev, search_ownership=on, **kw)


def test_refusals():
    from transgo_amd._lib import TransgoError
    eng = _small(True)
    with pytest.raises(TransgoError, match="tg_sp_root_ownership.*tg_sp_reset"):
        eng.root_ownership()                                        # before the first reset
    eng.reset([1, 2])
    assert not eng.root_ownership()["n"].any()                      # legal at once; nothing searched yet
    # a leaf batch pending: the switch is refused, and so is plain tg_sp_set_eval
    eng.ctx.call("tg_sp_begin_move", 1, 0)
    act, rows = ctypes.c_int32(), ctypes.c_int32()
    eng.ctx.call("tg_sp_collect", ctypes.byref(act), ctypes.byref(rows))
    assert rows.value > 0
    with pytest.raises(TransgoError, match="tg_sp_search_ownership: an evaluation batch is pending"):
        eng.set_search_ownership(False)
    assert eng.get_search_ownership()
    pol, val = np.zeros((rows.value, 82), F32), np.zeros(rows.value, F32)
    with pytest.raises(TransgoError, match="tg_sp_set_eval_own"):
        eng.ctx.call("tg_sp_set_eval", pol.ctypes.data_as(ctypes.c_void_p), val.ctypes.data_as(ctypes.c_void_p), rows.value)
    eng._evaluate(rows.value)
    eng.ctx.call("tg_sp_absorb")
    assert eng.root_ownership()["n"].sum() > 0
    # the evaluation cache and the mode refuse each other, in both orders
    with pytest.raises(TransgoError, match="tg_sp_eval_cache.*tg_sp_search_ownership"):
        eng.set_eval_cache(64)
    eng.set_search_ownership(False)
    with pytest.raises(TransgoError, match="search ownership is off"):
        eng.root_ownership()                                        # the mode is off
    eng.set_eval_cache(64)
    with pytest.raises(TransgoError, match="tg_sp_search_ownership.*tg_sp_eval_cache"):
        eng.set_search_ownership(True)
    assert not eng.get_search_ownership()
    eng.set_eval_cache(0)
    eng.set_search_ownership(True)
    assert eng.get_search_ownership()
    eng.close()
    # a host evaluator that returns a two-tuple
    from transgo_amd.engine import SelfPlayEngine
    two = SelfPlayEngine(2, num_simulation=16, evaluator=evaluators.flat, search_ownership=True)
    with pytest.raises(ValueError, match="two-tuple"):
        two.reset([1, 2])
    two.close()


def test_restore_clears_and_the_next_search_fills_as_on_a_fresh_engine():
    a = _small(True)
    a.reset([5, 6])
    _moves(a, 1)
    assert (a.root_ownership()["n"] > 0).all()                      # the last search's sums stay until the next move begins
    snap = a.snapshot()
    a.restore(snap)
    ro = a.root_ownership()
    assert not ro["n"].any() and not ro["mean"].any() and (ro["score_lead"] == F32(-7.5)).all()
    b = _small(True)
    b.reset([0, 0])
    b.restore(snap)
    for eng in (a, b):
        eng.search(True)
    ra, rb = a.root_ownership(), b.root_ownership()
    assert (ra["n"] > 0).all()
    assert all(np.array_equal(ra[k], rb[k]) for k in ("mean", "n", "score_lead"))
    # reset clears too, for the games it restarts
    a.reset([7, 8])
    assert not a.root_ownership()["n"].any()
    a.close(); b.close()


def test_grouped_engine_switch_reaches_every_group_and_reads_out_in_game_order():
    """Four games as two groups of two against the same four games on one engine (same seeds by slot, and a network row does not
    depend on its batch): the concatenated read-out equals the single engine's, game by game."""
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay, GroupedSelfPlay
    cfg = Config(num_simulation=16, num_features=32, num_blocks=2, search_ownership=True)
    sd = model.random_weights(9, 10, 32, 2, seed=7)
    one, two = BatchedSelfPlay(cfg, 4), GroupedSelfPlay(cfg, 4, groups=2)
    for w in (one, two):
        w.set_weights(sd)
        w.start()
        w.advance()
    assert two.get_search_ownership() and all(p.engine.get_search_ownership() for p in two.parts)
    a, b = one.engine.root_ownership(), two.root_ownership()
    assert b["mean"].shape == (4, 9, 9) and b["n"].shape == (4,) and (a["n"] > 0).all()
    assert len({a["mean"][g].tobytes() for g in range(4)}) == 4            # four different maps: an order mix-up would show
    assert all(np.array_equal(a[k], b[k]) for k in ("mean", "n", "score_lead"))
    two.set_search_ownership(False)
    assert not any(p.engine.get_search_ownership() for p in two.parts)
    one.engine.close(); two.close()
    for p in two.parts:
        p.engine.close()


# ---- analysis -------------------------------------------------------------------------------------------------------------------

def test_analyse_with_ownership():
    from transgo_amd import analysis, model
    from transgo_amd.engine import SelfPlayEngine
    from transgo_amd.environment import GoEnv
    env = GoEnv(board_size=9)
    states = []
    for line in ((), (40, 20), (30, 50, 31, 51), (40,), (40, 20, 60), (10, 11, 12, 13, 14)):       # three with Black to move, three with White
        st, _ = env.reset()
        for a in line:
            st, done = env.step(st, a)
            assert not done
        states.append(np.frombuffer(st, np.uint8).copy())
    states = np.stack(states)
    eng = SelfPlayEngine(6, num_simulation=32, parallel_readouts=so.R, net_blocks=2, net_filters=32)
    model.load_into(eng.ctx, model.random_weights(9, 10, 32, 2, seed=3), 9, 10, 32, 2)
    eng.reset(np.arange(6))
    recs = analysis.analyse(eng, states, ownership=True)
    assert not eng.get_search_ownership()                           # the engine's own switch is put back
    players = eng.root_info(obs=False)[2]
    assert sorted(players.tolist()) == [1, 1, 1, 2, 2, 2]
    for r in recs:
        own = r["ownership"]
        assert own.shape == (9, 9) and own.dtype == np.float32 and r["ownership_evals"] > 0 and np.abs(own).max() <= 1.0 and own.any()
        s = own.reshape(-1)[0]
        for p in range(1, 81):
            s = F32(s + own.reshape(-1)[p])
        assert r["score_lead"] == float(F32(s - F32(7.5)))
        txt = analysis.format_analysis(r, 9)
        assert f"search ownership over {r['ownership_evals']} evaluations" in txt and len(txt.split("\n")) >= 2 + 1 + 11
    plain = analysis.analyse(eng, states[:1])
    assert "ownership" not in plain[0]
    with pytest.raises(ValueError, match="evaluation cache"):
        analysis.analyse(eng, states, ownership=True, eval_cache_entries=1024)
    eng.close()
