"""tg_env_rollout (whole random playouts in one kernel launch) and what is built on it -- GoEnv.rollout_batch,
analysis.playout_ownership, SelfPlay.evaluate_random -- against games recorded from the reference's engine
(tests/golden/playouts.npz) and against tests/playout_ref.py over the CPU oracle.  Every comparison is exact: moves, plies, bytes of
state, score, territory, and the 624 key words + position of the MT19937 stream."""
import ctypes
import os

import numpy as np
import pytest

from oracle import evaluators
from oracle.go_oracle import OracleGoEnv
from tests import playout_ref

pytestmark = pytest.mark.gpu


def _env(size, max_step):
    from transgo_amd.configure import Config
    from transgo_amd.environment import GoEnv
    return GoEnv(Config(board_size=size, max_step=max_step))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _blob(rs):
    """RandomState -> the bytes of a tg_mt19937 (624 key words, position)."""
    s = rs.get_state()
    return np.concatenate([s[1].astype(np.uint32), np.array([s[2]], np.uint32)]).view(np.uint8)


def _advanced(seed, pos):
    """np.random.RandomState(seed) moved on until its position is `pos` (one 32-bit word per 4 bytes drawn)."""
    rs = np.random.RandomState(seed)
    rs.bytes(4 * pos)
    assert rs.get_state()[2] == pos
    return rs


def _pos(streams):
    return np.ascontiguousarray(streams)[:, -4:].copy().view(np.int32).reshape(-1)


def _step_replay(env, start, moves, plies):
    """The recorded moves through tg_env_step, ply by ply -> final states (a board is stepped for its own plies only)."""
    st = np.array(start, np.uint8)
    for p in range(int(plies.max()) if len(plies) else 0):
        live = plies > p
        nxt, _, ok = env.step_batch(st, np.where(live, moves[:, p], env.P))
        assert ok[live].all()
        st[live] = nxt[live]
    return st


def _oracle_state(orc, moves):
    st, done = orc.reset()
    for a in moves:
        st, done = orc.step(st, int(a))
    return st, done


@pytest.mark.parametrize("tag,size", [("s9_noeye", 9), ("s9_legal", 9), ("s19_noeye", 19)])
def test_fixture_games_replay_through_one_launch(golden_dir, tag, size):
    with np.load(os.path.join(golden_dir, "playouts.npz")) as z:
        f = {k.split("/")[1]: z[k] for k in z.files if k.startswith(tag + "/")}
    max_step, n = int(f["max_step"]), len(f["seeds"])
    env = _env(size, max_step)
    start = env.reset_batch(n)
    r = env.rollout_batch(start, seeds=f["seeds"], policy=tag.split("_")[1], record=True)
    assert r["moves"].shape == (n, max_step)
    assert (r["moves"] == f["moves"]).all() and (r["plies"] == f["plies"]).all() and (r["done"] == f["done"].astype(bool)).all()
    assert (r["states"] == _step_replay(env, start, r["moves"], r["plies"])).all()
    q = env.query_batch(r["states"], score=True, terr=True)
    assert (q["score"] == f["score"]).all() and (q["terr"].astype(np.int8) == f["terr"]).all()
    assert (_pos(r["streams"]) == f["pos"]).all()
    key = r["streams"][:, :-4].copy().view(np.uint32)
    assert [playout_ref.key_checksum_words(k) for k in key] == [int(v) for v in f["ksum"]]


@pytest.mark.parametrize("size,n,max_step,policy", [(9, 64, 160, "noeye"), (9, 64, 160, "legal"), (19, 8, 120, "noeye")])
def test_fresh_seeds_budgets_twist_and_finished_boards_against_the_oracle(size, n, max_step, policy):
    """Streams that start at positions 600..623 (the twist happens inside the kernel), budgets 0 / 1 / 7 / unlimited in one call,
    and boards that arrive terminated."""
    env, orc = _env(size, max_step), OracleGoEnv(board_size=size, max_step=max_step)
    P = size * size
    budgets = np.array([0, 1, 7, max_step], np.int32)[np.arange(n) % 4]
    n_term = 4                                                        # boards 0..3 arrive after a double pass, one per budget kind
    start = env.reset_batch(n)
    for _ in range(2):
        nxt, _, _ = env.step_batch(start, np.full(n, P))
        start[:n_term] = nxt[:n_term]
    assert env.query_batch(start, meta=True)["terminated"].tolist() == [1] * n_term + [0] * (n - n_term)
    rss = [_advanced(7000 + i, 600 + i % 24) for i in range(n)]
    streams = np.stack([_blob(rs) for rs in rss])
    r = env.rollout_batch(start, streams=streams, max_plies=budgets, policy=policy, record=True)
    assert r["moves"].shape == (n, max_step)
    twisted = 0
    for i in range(n):
        st, done = _oracle_state(orc, [P, P] if i < n_term else [])
        pos0 = rss[i].get_state()[2]
        st, moves, done, _ = playout_ref.playout(orc, st, rss[i], None if budgets[i] == max_step else int(budgets[i]), policy, done)
        twisted += rss[i].get_state()[2] < pos0
        assert r["plies"][i] == len(moves) and bool(r["done"][i]) == done, i
        assert list(r["moves"][i][:len(moves)]) == moves and (r["moves"][i][len(moves):] == -1).all(), i
        assert (r["streams"][i] == _blob(rss[i])).all(), i
    assert (r["plies"][:n_term] == 0).all() and (r["states"][:n_term] == start[:n_term]).all()
    assert (r["streams"][:n_term] == streams[:n_term]).all() and (r["plies"][budgets == 0] == 0).all()
    assert twisted >= n // 8                                         # the unlimited boards all cross word 624
    assert (r["states"] == _step_replay(env, start, r["moves"], r["plies"])).all()


@pytest.mark.parametrize("size,n,max_step", [(9, 64, 160), (19, 8, 120)])
def test_continuation_from_mid_game_in_place_and_without_a_move_record(size, n, max_step):
    """Two calls of 30 plies (states and streams handed on) equal one call of 60, which equals the oracle; in == out and
    moves == NULL change nothing."""
    env, orc = _env(size, max_step), OracleGoEnv(board_size=size, max_step=max_step)
    seeds = 300 + np.arange(n)
    start = env.reset_batch(n)
    a = env.rollout_batch(start, seeds=seeds, max_plies=30, record=True)
    b = env.rollout_batch(a["states"], streams=a["streams"], max_plies=30, record=True)
    c = env.rollout_batch(start, seeds=seeds, max_plies=60, record=True)
    assert (a["plies"] == 30).all() and (c["plies"] == 60).all() and not c["done"].any()
    assert (b["states"] == c["states"]).all() and (b["streams"] == c["streams"]).all()
    assert (np.concatenate([a["moves"], b["moves"]], axis=1) == c["moves"]).all()
    for i in range(n):
        rs = np.random.RandomState(int(seeds[i]))
        st, _ = orc.reset()
        st, moves, done, _ = playout_ref.playout(orc, st, rs, 60, "noeye")
        assert moves == list(c["moves"][i]) and not done and (c["streams"][i] == _blob(rs)).all(), i
    assert (c["states"] == _step_replay(env, start, c["moves"], c["plies"])).all()
    d = env.rollout_batch(start, seeds=seeds, max_plies=60)           # moves = NULL
    assert "moves" not in d and (d["states"] == c["states"]).all() and (d["streams"] == c["streams"]).all()
    assert (d["plies"] == c["plies"]).all()
    # in == out, through the C ABI itself, from the mid-game position
    buf, rng = a["states"].copy(), a["streams"].copy()
    budget = np.full(n, 30, np.int32); plies = np.zeros(n, np.int32); done = np.zeros(n, np.uint8)
    env.ctx.call("tg_env_rollout", _ptr(buf), _ptr(buf), n, _ptr(rng), _ptr(budget), 0, _ptr(plies), _ptr(done), None, 0)
    assert (buf == b["states"]).all() and (rng == b["streams"]).all() and (plies == 30).all() and not done.any()


def test_argument_refusals():
    env = _env(9, 40)
    n = 3
    st = env.reset_batch(n)
    rng = env.seed_streams([1, 2, 3])
    plies = np.zeros(n, np.int32); done = np.zeros(n, np.uint8)

    def rc(budget, policy, moves, cap):
        s, r = st.copy(), rng.copy()
        code = env.ctx.lib.tg_env_rollout(env.ctx.h, _ptr(s), _ptr(s), n, _ptr(r), _ptr(budget), policy, _ptr(plies), _ptr(done),
                                          _ptr(moves), cap)
        if code != 0:
            assert (s == st).all() and (r == rng).all()               # a refused call touches nothing
        return code

    ERR_ARG = -1
    b = np.array([5, 9, 0], np.int32)
    assert rc(b, 0, None, 0) == 0 and rc(b, 1, None, 0) == 0
    assert rc(b, 2, None, 0) == ERR_ARG and rc(b, -1, None, 0) == ERR_ARG                 # unknown policy
    assert rc(np.array([5, -1, 0], np.int32), 0, None, 0) == ERR_ARG                      # negative budget
    assert rc(b, 0, np.zeros((n, 8), np.int32), 8) == ERR_ARG                             # moves_cap < the largest budget
    assert rc(b, 0, np.zeros((n, 9), np.int32), 9) == 0
    assert rc(None, 0, np.zeros((n, 39), np.int32), 39) == ERR_ARG                        # moves_cap < max_step, no budgets
    assert rc(None, 0, np.zeros((n, 40), np.int32), 40) == 0
    with pytest.raises(ValueError):
        env.rollout_batch(st, seeds=[1, 2, 3], policy="eyes")
    with pytest.raises(ValueError):
        env.rollout_batch(st, seeds=[1, 2, 3], max_plies=[1, -2, 3])
    with pytest.raises(ValueError):
        env.rollout_batch(st)


def test_playout_ownership_equals_the_oracle_statistic():
    from transgo_amd import analysis
    max_step, K, seed = 160, 16, 5
    env, orc = _env(9, max_step), OracleGoEnv(max_step=max_step)
    mid = env.rollout_batch(env.reset_batch(3), seeds=[11, 12, 13], max_plies=[10, 25, 40], record=True)
    got = analysis.playout_ownership(env, mid["states"], playouts=K, seed=seed)
    assert len(got) == 3
    for i in range(3):
        terr, score = np.zeros(81, np.int64), []
        for k in range(K):
            st, done = _oracle_state(orc, mid["moves"][i][:mid["plies"][i]])
            st, _, _, _ = playout_ref.playout(orc, st, np.random.RandomState(seed + i * K + k), None, "noeye", done)
            s, t = orc.getScoreAndTerritory(st)
            terr += t.astype(np.int64); score.append(np.float64(s))
        assert got[i]["territory"].dtype == np.float64 and (got[i]["territory"] == terr / K).all(), i
        assert got[i]["score"] == float(np.sum(score) / K) and got[i]["black_win"] == float((np.array(score) > 0).sum() / K), i
        assert got[i]["playouts"] == K
    assert "playouts 16" in analysis.format_ownership(got[0], 9)


def test_playout_ownership_of_a_settled_position_is_its_tromp_taylor_map(golden_dir):
    """A position in which neither side has a no-eye move left (a recorded game that ended by double pass, without its two
    passes): every playout is pass, pass, so the mean territory is the Tromp-Taylor map itself."""
    from transgo_amd import analysis
    with np.load(os.path.join(golden_dir, "playouts.npz")) as z:
        moves, plies, max_step = z["s9_noeye/moves"], z["s9_noeye/plies"], int(z["s9_noeye/max_step"])
    i = int(np.flatnonzero(plies < max_step)[0])
    env = _env(9, max_step)
    n = int(plies[i]) - 2
    assert list(moves[i][n:n + 2]) == [81, 81]
    st = _step_replay(env, env.reset_batch(1), moves[i:i + 1].astype(np.int32), np.array([n]))
    after_pass, _, _ = env.step_batch(st, [81])
    for s in (st, after_pass):                                        # premise: only pass is left, for either side
        assert env.query_batch(s, noeye=True)["noeye"][0].nonzero()[0].tolist() == [81]
    assert not env.query_batch(st, meta=True)["terminated"][0]
    q = env.query_batch(st, score=True, terr=True)
    got = analysis.playout_ownership(env, st, playouts=8, seed=1)[0]
    assert (got["territory"] == q["terr"][0].astype(np.float64)).all() and got["score"] == float(q["score"][0])
    assert got["black_win"] == float(q["score"][0] > 0)
    assert (np.abs(got["territory"]) == 1).sum() > 60                 # a settled board, not an empty one


def test_evaluate_random_equals_the_oracle_twin():
    """SelfPlay.evaluate_random (all games at once on one engine, the random player through tg_env_rollout) against the sequential
    game after np.random.seed(seed + i): oracle.wp_mcts select_action for the network, np.random.choice over the pass-filtered
    getLegalAction for the bot, both on the one global stream."""
    from oracle.wp_mcts import OracleSearch
    from transgo_amd.configure import Config
    from transgo_amd.self_play import SelfPlay
    n_games, sims, max_step, seed = 4, 24, 30, 90
    cfg = Config(num_simulation=sims, max_step=max_step)
    sp = SelfPlay(cfg, n_games=2, evaluator=evaluators.sharp)
    ratio, winners, colours = sp.evaluate_random(n_games, seed=seed, evaluators={"train": evaluators.sharp})
    streams = sp.last_random_evaluation["streams"]
    sp.worker.engine.close()
    orc = OracleGoEnv(max_step=max_step)
    saved = np.random.get_state()
    try:
        for i in range(n_games):
            np.random.seed(seed + i)
            colour = 1 if i % 2 == 0 else 2
            net = OracleSearch(orc, evaluators.sharp, np.random.mtrand._rand, num_simulation=sims)
            state, done = orc.reset()
            while not done:
                if orc.getPlayer(state) == colour:
                    action = net.select_action(state)
                else:
                    action = np.random.choice(orc.getLegalAction(state))
                state, done = orc.step(state, action)
            assert winners[i] == orc.getWinner(state) and colours[i] == colour, i
            assert (streams[i] == _blob(np.random.mtrand._rand)).all(), i
    finally:
        np.random.set_state(saved)
    assert ratio == float((winners == colours).sum()) / n_games


def test_evaluate_random_runs_with_the_f32_tower():
    """End to end with the real 6x128 f32 network (random weights: no strength claim): no engine error, a ratio in [0, 1]."""
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import SelfPlay
    cfg = Config(num_simulation=16, max_step=40)
    sp = SelfPlay(cfg, n_games=2, evaluator=evaluators.flat)          # the worker's own engine is not the one that plays
    ratio, winners, colours = sp.evaluate_random(8, seed=3, weights=model.random_weights(9, 10, 128, 6, seed=1))
    sp.worker.engine.close()
    assert 0.0 <= ratio <= 1.0 and len(winners) == 8 and set(winners) <= {1, 2} and list(colours) == [1, 2] * 4
