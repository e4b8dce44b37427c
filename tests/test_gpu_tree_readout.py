"""Tree read-out (tg_sp_root_children, tg_sp_pv, transgo_amd.analysis) against the CPU oracle's Vertex objects, driven exactly as
tests/test_gpu_search.py::test_many_games_vs_oracle drives engine and oracle.  Every comparison is exact: visit and pending counters
as integers, w / var as float32 bit patterns, priors as float64 bit patterns (the oracle's Python-float 0. of an unvisited node is
0.0f).  Evaluators are the stand-ins of oracle/evaluators.py unless a test says otherwise."""
import ctypes

import numpy as np
import pytest

from oracle import evaluators

pytestmark = pytest.mark.gpu


def uniform(obs):
    """Equal priors everywhere and a constant value: every PUCT comparison among unvisited siblings is a tie."""
    k, _, S, _ = np.asarray(obs).shape
    A = S * S + 1
    return np.full((k, A), np.float32(1) / np.float32(A), np.float32), np.zeros((k, 1), np.float32)


def _engine(fn, G, sims, **kw):
    from transgo_amd.engine import SelfPlayEngine
    return SelfPlayEngine(G, num_simulation=sims, evaluator=fn, **kw)


def _oracles(fn, seeds, S, sims, max_step):
    from oracle.go_oracle import OracleGoEnv
    from oracle.wp_mcts import OracleSearch
    out = []
    for s in seeds:
        rng = np.random.RandomState(int(s))
        out.append((OracleSearch(OracleGoEnv(board_size=S, max_step=max_step), fn, rng, num_simulation=sims, board_size=S), rng))
    return out


def _f32(x):
    return np.float32(x).view(np.uint32)


def _f64(x):
    return np.float64(x).view(np.uint64)


def oracle_tables(root, A):
    """root.kids as the dense arrays root_children() returns, floats as bit patterns."""
    t = dict(n=np.zeros(A, np.int32), pending=np.zeros(A, np.int32), w=np.zeros(A, np.uint32), var=np.zeros(A, np.uint32),
             prior=np.zeros(A, np.uint64), present=np.zeros(A, bool), open=np.zeros(A, bool), prior32=np.zeros(A, bool))
    for a, k in root.kids.items():
        t["n"][a], t["pending"][a], t["w"][a], t["var"][a], t["prior"][a] = k.n, k.pending, _f32(k.w), _f32(k.var), _f64(k.prior)
        t["present"][a], t["open"][a], t["prior32"][a] = True, k.open, isinstance(k.prior, np.float32)
    return t


def assert_game_equals_oracle(eng, rc, g, root, where):
    t = oracle_tables(root, eng.A)
    assert rc["status"][g] == eng.ROOT_OK, (where, g, rc["status"][g])
    assert (rc["n"][g] == t["n"]).all() and (rc["pending"][g] == t["pending"]).all(), (where, g, "n / pending")
    assert (rc["w"][g].view(np.uint32) == t["w"]).all(), (where, g, "w")
    assert (rc["var"][g].view(np.uint32) == t["var"]).all(), (where, g, "var")
    assert (rc["prior"][g].view(np.uint64) == t["prior"]).all(), (where, g, "prior")
    f = rc["flags"][g]
    assert (((f & eng.CHILD_PRESENT) != 0) == t["present"]).all(), (where, g, "present")
    assert (((f & eng.CHILD_OPEN) != 0) == t["open"]).all(), (where, g, "open")
    assert (((f & eng.CHILD_PRIOR32) != 0) == t["prior32"]).all(), (where, g, "prior kind")
    assert rc["root_n"][g] == root.n and rc["root_pending"][g] == root.pending, (where, g, "root n / pending")
    assert _f32(rc["root_w"][g]) == _f32(root.w) and _f32(rc["root_var"][g]) == _f32(root.var), (where, g, "root w / var")


def oracle_pv(root, depth):
    """The rule of tg_sp_pv over Vertex objects: most visits, ties to the lowest action (the order of `kids`); stops at a node
    that is not open, has no children, or whose best child was never visited.  Returns (actions, visits, w bits, ties met)."""
    node, acts, vis, ws, ties = root, [], [], [], 0
    while len(acts) < depth and node.open and node.kids:
        top = max(k.n for k in node.kids.values())
        if top == 0:
            break
        best = [a for a, k in node.kids.items() if k.n == top]         # ascending action, pass last
        ties += len(best) > 1
        node = node.kids[best[0]]
        acts.append(best[0]); vis.append(node.n); ws.append(_f32(node.w))
    return acts, vis, ws, ties


def assert_pv_equals_oracle(eng, orcs, depth, where):
    act, vis, w, ln = eng.principal_variation(depth)
    assert act.shape == vis.shape == w.shape == (eng.G, depth) and ln.shape == (eng.G,)
    ties = 0
    for g, (o, _) in enumerate(orcs):
        oa, ov, ow, t = oracle_pv(o.root, depth)
        ties += t
        m = len(oa)
        assert ln[g] == m, (where, g, depth, ln[g], m)
        assert list(act[g, :m]) == oa and list(vis[g, :m]) == ov and list(w[g, :m].view(np.uint32)) == ow, (where, g, depth)
        assert (act[g, m:] == -1).all() and (vis[g, m:] == 0).all() and (w[g, m:].view(np.uint32) == 0).all(), (where, g, "padding")
    return ties


@pytest.mark.parametrize("S,G,sims,moves,max_step", [(9, 6, 48, 6, 120), (19, 2, 40, 3, 450)])
def test_root_tables_equal_the_oracle_after_every_search_and_play(S, G, sims, moves, max_step):
    """The per-action tables and the root's own record after every search() and again after every play() (the re-rooted, copied
    sub-tree); at 19x19 A = 362 makes six lane passes, the last one partial.  The read-out disturbs nothing: the RNG positions
    still equal the oracle's after the last move."""
    fn = evaluators.sharp
    seeds = np.arange(100, 100 + G)
    eng = _engine(fn, G, sims, board_size=S, max_step=max_step)
    eng.reset(seeds)
    orcs = _oracles(fn, seeds, S, sims, max_step)
    rc = eng.root_children()
    for g, (o, _) in enumerate(orcs):
        assert_game_equals_oracle(eng, rc, g, o.root, "fresh root")
    for m in range(moves):
        eng.search()
        rc = eng.root_children()
        vis, st = eng.root_visits()
        assert (rc["n"] == vis).all()
        acts, _ = eng.choose_moves(vis, st)
        for g, (o, _) in enumerate(orcs):
            a, _, _, _ = o.search_move()
            assert a == acts[g], (g, m)
            assert_game_equals_oracle(eng, rc, g, o.root, ("search", m))
            o.advance(a)
        done = eng.play(acts)
        assert not done.any()
        rc = eng.root_children()
        for g, (o, _) in enumerate(orcs):
            assert_game_equals_oracle(eng, rc, g, o.root, ("play", m))
    for g, (o, rng) in enumerate(orcs):
        assert eng.rng_state(g)[1] == rng.get_state()[2], g
    assert eng.stats()["errors"] == 0
    eng.close()


@pytest.mark.parametrize("S,fn,sims,max_step", [(9, evaluators.sharp, 48, 120), (9, uniform, 48, 120), (9, evaluators.flat, 48, 120),
                                                (19, evaluators.sharp, 40, 450)], ids=["9-sharp", "9-uniform", "9-flat", "19-sharp"])
def test_principal_variation_equals_the_oracle_walk(S, fn, sims, max_step):
    """Depths 1, 8 and the path capacity, after a first search and after a second one on the re-rooted tree.  With equal priors the
    48 simulations spread over 81 children, so the most-visited count is shared: the walk must meet ties (else the rule that
    ties go to the lowest action is not tested)."""
    G = 3
    seeds = np.arange(40, 40 + G)
    eng = _engine(fn, G, sims, board_size=S, max_step=max_step)
    eng.reset(seeds)
    orcs = _oracles(fn, seeds, S, sims, max_step)
    assert eng.path_capacity == (128 if S == 9 else 512)
    ties = 0
    for m in range(2):                                                     # evaluation-mode searches: no noise, no move draw
        eng.search(selfplay=False)
        for o, _ in orcs:
            n0 = o.root.n
            while o.root.n < n0 + sims:
                o.wave()
        for depth in (1, 8, eng.path_capacity):
            ties += assert_pv_equals_oracle(eng, orcs, depth, ("search", m))
        acts = [oracle_pv(o.root, 1)[0][0] for o, _ in orcs]               # both sides play the line's first move
        for g, (o, _) in enumerate(orcs):
            o.advance(acts[g])
        eng.play(acts)
        assert_pv_equals_oracle(eng, orcs, 8, ("play", m))
    if fn is uniform:
        assert ties > 0, "no tie in visits met: the tie rule was not exercised"
    eng.close()


def test_mid_wave_read_out_reports_pending_counters_as_they_stand():
    """Between tg_sp_collect and tg_sp_absorb the WU-UCT counters of the paths in flight are up: the tables equal the oracle's
    after its collect(); after absorb they are all 0 again."""
    G, sims = 3, 48
    seeds = np.arange(7, 7 + G)
    eng = _engine(evaluators.sharp, G, sims)
    eng.reset(seeds)
    orcs = _oracles(evaluators.sharp, seeds, 9, sims, 120)
    eng.ctx.call("tg_sp_begin_move", 1, 0)
    for o, rng in orcs:
        o.root.add_root_noise(rng)
    seen_pending = 0
    for wave in range(5):
        act, rows = ctypes.c_int32(), ctypes.c_int32()
        eng.ctx.call("tg_sp_collect", ctypes.byref(act), ctypes.byref(rows))
        rc = eng.root_children()
        pv_mid = eng.principal_variation(8)
        flight = [o.collect() for o, _ in orcs]
        for g, (o, _) in enumerate(orcs):
            assert_game_equals_oracle(eng, rc, g, o.root, ("collect", wave))
            assert rc["root_pending"][g] == 2 * len(flight[g][0])
            oa, ov, _, _ = oracle_pv(o.root, 8)
            assert list(pv_mid[0][g, :pv_mid[3][g]]) == oa and list(pv_mid[1][g, :pv_mid[3][g]]) == ov
        seen_pending += int(rc["pending"].sum())
        eng._evaluate(rows.value)
        eng.ctx.call("tg_sp_absorb")
        for (o, _), (paths, leaves) in zip(orcs, flight):
            if paths:
                probs, values = o._eval(leaves)
                o.absorb(paths, leaves, probs, values)
        rc = eng.root_children()
        assert (rc["pending"] == 0).all() and (rc["root_pending"] == 0).all()
        for g, (o, _) in enumerate(orcs):
            assert_game_equals_oracle(eng, rc, g, o.root, ("absorb", wave))
    assert seen_pending > 0
    eng.close()


def _dense_position(seed, plies, max_step=120):
    """The same seeded random game (no passes) in the oracle's and the engine's rules: (oracle state, engine state blob)."""
    from oracle.go_oracle import OracleGoEnv
    from transgo_amd.environment import GoEnv
    oenv, genv = OracleGoEnv(max_step=max_step), GoEnv()
    rs = np.random.RandomState(seed)
    so, _ = oenv.reset()
    sg = genv.reset_batch(1)
    for _ in range(plies):
        legal = list(oenv.getLegalAction(so))
        a = int(legal[rs.randint(len(legal))])
        so, d1 = oenv.step(so, a)
        sg, d2, ok = genv.step_batch(sg, [a])
        assert ok[0] and not d1 and not d2[0]
    return so, sg[0]


def _searched_oracle(state, seed, sims, fn, max_step=120):
    """An oracle rooted at `state` with a fresh tree, searched in evaluation mode (no noise) for `sims` simulations."""
    from oracle.go_oracle import OracleGoEnv
    from oracle.wp_mcts import OracleSearch, Vertex
    o = OracleSearch(OracleGoEnv(max_step=max_step), fn, np.random.RandomState(int(seed)), num_simulation=sims)
    o.root = Vertex(0)
    o.root.state = state
    o._open_root(o.root)
    while o.root.n < sims:
        o.wave()
    return o


def test_parked_finished_and_error_slots_report_a_status_and_leave_the_others_alone():
    """One engine, five slots, a tree cap of two chunks (arena_slots as in test_arena_overflow_parks_the_game_and_the_slot_restarts)
    and 40 simulations.  Slot 0 starts from the empty board: its blocks hold 2 + 81 slots, twelve fit a chunk of 1024, and the 35 or
    more a 40-simulation search allocates do not fit two chunks -- the engine's own parking path puts it in error.  Slots 1 and 4
    start from boards with 60-odd stones: blocks of ~30 slots, whole search well inside the cap.  Slot 2 is left out by the reset
    mask (parked), slot 3 is a position finished by two passes.  Slots 1 and 4 must still equal the oracle."""
    from transgo_amd.environment import GoEnv
    sims = 40
    fn = evaluators.sharp
    seeds = np.arange(60, 65)
    eng = _engine(fn, 5, sims, arena_slots=6 * 84 + 16)
    eng.reset(seeds)
    genv = GoEnv()
    empty = genv.reset_batch(1)
    over, d, _ = genv.step_batch(genv.step_batch(empty, [81])[0], [81])
    assert d[0]
    dense = {1: _dense_position(11, 66), 4: _dense_position(12, 70)}
    states = np.stack([empty[0], dense[1][1], empty[0], over[0], dense[4][1]])
    eng.reset_from(states, mask=[1, 1, 0, 1, 1])
    eng.search(selfplay=False)
    err = eng.game_errors()
    print("game errors", err, "stats", eng.stats())
    assert list(err) == [1, 0, 0, 0, 0]
    rc = eng.root_children()
    act, vis, w, ln = eng.principal_variation(8)
    assert list(rc["status"]) == [eng.ROOT_ERROR, eng.ROOT_OK, eng.ROOT_PARKED, eng.ROOT_TERMINAL, eng.ROOT_OK]
    for g in (0, 2, 3):
        for k in ("n", "pending", "w", "var", "prior", "flags"):
            assert not rc[k][g].any(), (g, k)
        assert ln[g] == 0 and (act[g] == -1).all() and not vis[g].any() and not w[g].any()
    for g in (0, 2):
        assert rc["root_n"][g] == 0 and rc["root_pending"][g] == 0 and rc["root_w"][g] == 0 and rc["root_var"][g] == 0
    for g in (1, 4):
        o = _searched_oracle(dense[g][0], seeds[g], sims, fn)
        assert_game_equals_oracle(eng, rc, g, o.root, "dense")
        oa, ov, ow, _ = oracle_pv(o.root, 8)
        assert ln[g] == len(oa) >= 1 and list(act[g, :ln[g]]) == oa and list(vis[g, :ln[g]]) == ov
    eng.close()


def test_argument_errors_are_reported_and_leave_the_engine_usable():
    from transgo_amd._lib import TransgoError
    from transgo_amd.engine import SelfPlayEngine
    from transgo_amd.environment import GoEnv
    fresh = SelfPlayEngine(2, num_simulation=8, evaluator=evaluators.sharp)
    for call in (fresh.root_children, fresh.principal_variation):      # no tree yet: nothing was reset
        with pytest.raises(TransgoError, match="tg_sp_reset first"):
            call()
    fresh.reset([1, 2])
    eng = fresh
    for depth in (0, -3, eng.path_capacity + 1):
        with pytest.raises(TransgoError, match="depth must be 1"):
            eng.principal_variation(depth)
    rules = GoEnv()
    buf = np.zeros(82, np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    with pytest.raises(TransgoError, match="no engine"):
        rules.ctx.call("tg_sp_root_children", p, *[None] * 10)
    with pytest.raises(TransgoError, match="no engine"):
        rules.ctx.call("tg_sp_pv", 4, p, None, None, None)
    assert not buf.any()
    eng.search()
    rc = eng.root_children()
    vis, _ = eng.root_visits()
    assert (rc["n"] == vis).all() and (rc["status"] == eng.ROOT_OK).all()
    assert (eng.principal_variation(eng.path_capacity)[3] >= 1).all()
    # any output may be left out
    n = np.zeros((2, 82), np.int32); st = np.zeros(2, np.uint8)
    eng.ctx.call("tg_sp_root_children", n.ctypes.data_as(ctypes.c_void_p), *[None] * 9, st.ctypes.data_as(ctypes.c_void_p))
    assert (n == vis).all() and not st.any()
    eng.close()


class _NoMoveDraw:
    """select_action's last statement draws the move to play (self_play.py:683); analyse() plays nothing and draws nothing.  This
    stand-in for the oracle's RandomState makes that one draw on a copy, so the stream the NEXT position of the same engine slot
    starts from is the one the engine has; the tie-break draws (choice without p) go to the real stream."""

    def __init__(self, rng):
        self.rng = rng

    def choice(self, a, p=None):
        if p is None:
            return self.rng.choice(a)
        twin = np.random.RandomState()
        twin.set_state(self.rng.get_state())
        return twin.choice(a, p=p)


def test_analyse_equals_select_action_of_the_oracle():
    """Five positions on an engine of two games (chunks of 2, 2, 1): visits, q (float32 bits, NaN placement), priors and the PV of
    every record against OracleSearch.select_action from the same states with the same evaluator."""
    from oracle.go_oracle import OracleGoEnv
    from oracle.wp_mcts import OracleSearch
    from transgo_amd import analysis
    sims, fn = 48, evaluators.sharp
    positions = [_dense_position(20 + i, plies) for i, plies in enumerate((0, 3, 10, 25, 41))]
    eng = _engine(fn, 2, sims)
    eng.reset([5, 6])
    recs = analysis.analyse(eng, np.stack([p[1] for p in positions]), depth=8)
    assert len(recs) == 5
    streams = [_NoMoveDraw(np.random.RandomState(5)), _NoMoveDraw(np.random.RandomState(6))]
    for i, ((so, _), r) in enumerate(zip(positions, recs)):
        o = OracleSearch(OracleGoEnv(), fn, streams[i % 2], num_simulation=sims)
        o.select_action(so)
        t = oracle_tables(o.root, eng.A)
        assert r["status"] == 0 and (r["visits"] == t["n"]).all() and (r["legal"] == t["present"]).all(), i
        assert (r["prior"].view(np.uint64) == t["prior"]).all(), i
        q = np.full(eng.A, np.nan, np.float32)
        for a, k in o.root.kids.items():
            if k.n > 0:
                q[a] = -k.q()
                assert isinstance(-k.q(), np.float32)
        assert r["q"].dtype == np.float32 and (np.isnan(r["q"]) == np.isnan(q)).all(), i
        assert (r["q"].view(np.uint32)[~np.isnan(q)] == q.view(np.uint32)[~np.isnan(q)]).all(), i
        oa, ov, _, _ = oracle_pv(o.root, 8)
        assert r["pv"] == oa and r["pv_visits"] == ov and len(oa) >= 1, i
        assert np.float32(r["root_value"]) == np.float32(o.root.w) / np.float32(o.root.n + 1), i
    for g in range(2):
        assert eng.rng_state(g)[1] == streams[g].rng.get_state()[2]
    assert "visits" in analysis.format_analysis(recs[0], 9)
    eng.close()


def test_read_out_of_a_search_with_the_real_network():
    """No parity claim (the network's rounding is its own): shapes and invariants with random f32 weights."""
    from transgo_amd import model
    from transgo_amd.engine import SelfPlayEngine
    from transgo_amd.environment import GoEnv
    G = 4
    eng = SelfPlayEngine(G, num_simulation=32, net_blocks=2, net_filters=32)
    model.load_into(eng.ctx, model.random_weights(9, 10, 32, 2), 9, 10, 32, 2)
    eng.reset(np.arange(G))
    env = GoEnv()
    for m in range(2):
        eng.search()
        rc = eng.root_children()
        vis, rn, _, st, _ = eng.root_info(obs=False)
        assert (rc["status"] == eng.ROOT_OK).all() and (rc["n"] == vis).all() and (rc["root_n"] == rn).all()
        assert (rc["pending"] == 0).all() and np.isfinite(rc["w"]).all() and np.isfinite(rc["prior"]).all()
        states = eng.root_states()
        legal = env.query_batch(states, legal=True)["legal"].astype(bool)
        legal[:, -1] = ~legal[:, :-1].any(axis=1)                          # pass only when it is the only move (environment.py:121-129)
        assert (((rc["flags"] & eng.CHILD_PRESENT) != 0) == legal).all()
        act, pvn, _, ln = eng.principal_variation(16)
        assert (ln >= 1).all() and (ln <= 16).all()
        for g in range(G):
            s = states[g:g + 1]
            for a in act[g, :ln[g]]:
                s, _, ok = env.step_batch(s, [int(a)])
                assert ok[0], (g, a)
            assert (np.diff(pvn[g, :ln[g]]) <= 0).all() and pvn[g, 0] == vis[g].max() and act[g, 0] == vis[g].argmax()
        eng.play(eng.choose_moves(vis, st)[0])
    eng.close()
