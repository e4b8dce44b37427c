"""Pass-alive analysis on the device (csrc/pass_alive_dev.h, tg_env_pass_alive, tg_sp_root_pass_alive) against the
restatement transgo_amd/pass_alive.py, byte for byte; and the pass-alive end of self-play (tg_sp_pass_alive) against the mode-off
run of the same engine on the same seeds, with the restatement deciding where each game must end and how it is scored
(tests/test_gpu_pass_alive_engine.py compares the engine with the oracle search driver).

Positions and their restated results are computed once and shared."""
import functools

import numpy as np
import pytest

from tests.pass_alive_positions import HAND_9, HAND_19, states_of
from transgo_amd import pass_alive as pa

pytestmark = pytest.mark.gpu
KOMI = 7.5


@functools.lru_cache(maxsize=None)
def _env(S):
    from transgo_amd.environment import GoEnv
    # 19x19 playouts need more than the default 120 plies to reach positions where anything lives
    return GoEnv(config=type("C", (), dict(max_step={9: 120, 19: 510}[S], board_size=S))())


def _restate(states, S):
    b, w = pa.stones_of_states(states, S)
    status = np.stack([pa.pass_alive(b[i], w[i]) for i in range(len(b))])
    settled = np.array([pa.settled(s) for s in status])
    area = [pa.area_score(b[i], w[i], KOMI, status[i]) for i in range(len(b))]
    return dict(status=status, settled=settled, score=np.array([a[0] for a in area], np.float32), owner=np.stack([a[1] for a in area]))


def _assert_equal(got, want):
    assert got["status"].dtype == np.int8 and got["owner"].dtype == np.int8
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["settled"], want["settled"])
    assert np.array_equal(got["owner"], want["owner"])
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _playout_positions(S, n):
    """n positions taken at several depths of tg_env_rollout games, half under the no-eye and half under the plain policy."""
    env = _env(S)
    full = env.max_step
    out = []
    for k, policy in enumerate(("noeye", "legal")):
        m = n // 2
        depth = np.array([full, full - 1, full * 7 // 8, full * 3 // 4, full * 5 // 8, full // 2, full // 4, 8])[np.arange(m) % 8]
        r = env.rollout_batch(env.reset_batch(m), seeds=np.arange(m) + 500 * k + 7 * S, max_plies=depth, policy=policy)
        out.append(r["states"])
    return np.concatenate(out)


@pytest.mark.parametrize("S", [9, 19])
def test_hand_built_positions(S):
    env, hand = _env(S), (HAND_9 if S == 9 else HAND_19)
    names = sorted(hand)
    st = states_of([hand[k][0] for k in names], [hand[k][1] for k in names], env.ssz, S)
    got = env.pass_alive_batch(st)
    for i, k in enumerate(names):
        assert np.array_equal(got["status"][i], hand[k][2]), (k, got["status"][i].reshape(S, S))
    _assert_equal(got, _restate(st, S))
    assert list(got["settled"]) == [k == "settled" for k in names]


@pytest.mark.parametrize("S,n", [(9, 256), (19, 64)])
def test_playout_positions_equal_the_restatement(S, n):
    st = _playout_positions(S, n)
    want = _restate(st, S)
    got = _env(S).pass_alive_batch(st)
    _assert_equal(got, want)
    # the inputs exercise the analysis: live groups, territory, settled boards and boards where nothing lives
    alive = (np.abs(want["status"]) == 2).any(1)
    assert alive.sum() >= n // 8 and (~alive).sum() >= n // 8
    assert (np.abs(want["status"]) == 1).any()
    if S == 9:
        assert want["settled"].sum() >= 2
        tt = _env(S).query_batch(st, score=True)["score"]
        assert (want["score"] != tt).any()                              # somewhere the override changes the score


@pytest.mark.parametrize("S", [9, 19])
@pytest.mark.parametrize("n", [1, 65])
def test_batch_sizes(S, n):
    st = _playout_positions(S, 256 if S == 9 else 64)
    st = np.concatenate([st, st])[:n] if n > len(st) else st[:n]
    _assert_equal(_env(S).pass_alive_batch(st), _restate(st, S))


def test_optional_outputs_may_be_null():
    env = _env(9)
    st = _playout_positions(9, 256)[:5]
    status = np.zeros((5, 81), np.int8)
    env.ctx.call("tg_env_pass_alive", st.ctypes.data, 5, status.ctypes.data, None, None, None)
    assert np.array_equal(status, _env(9).pass_alive_batch(st)["status"])


# ---- the engine: read-outs and the pass-alive end --------------------------------------------------------------------------------
MAX_STEP = {9: 400, 19: 510}


def _engine(G, S=9, sims=8, max_step=None, **kw):
    from oracle import evaluators
    from transgo_amd.engine import SelfPlayEngine
    return SelfPlayEngine(G, board_size=S, num_simulation=sims, parallel_readouts=4, max_step=max_step or MAX_STEP[S], evaluator=evaluators.flat, **kw)


@functools.lru_cache(maxsize=None)
def _late_positions(S, G, back):
    """No-eye playouts stopped `back` plies before their end (max_step large enough not to interfere)."""
    from transgo_amd.environment import GoEnv
    env = GoEnv(config=type("C", (), dict(max_step=MAX_STEP[S], board_size=S))())
    seeds = np.arange(G) + 40
    full = env.rollout_batch(env.reset_batch(G), seeds=seeds, policy="noeye")
    assert full["done"].all()
    depth = np.maximum(full["plies"] - back, 0)
    return env.rollout_batch(env.reset_batch(G), seeds=seeds, max_plies=depth, policy="noeye")["states"]


def _play_out(eng, states, max_moves):
    """reset_from + searched moves until every game is over: per move (live, raw visits, actions, done)."""
    eng.reset(np.arange(eng.G) + 11)
    eng.reset_from(states)
    out = []
    for _ in range(max_moves):
        if eng.finished.all():
            break
        live = ~eng.finished
        eng.search(True)
        raw, _, _, st, _ = eng.root_info(obs=False)
        acts = eng.choose_moves(raw, st)[0]
        done = eng.play(acts)
        out.append(dict(live=live, raw=raw, acts=np.asarray(acts), done=np.asarray(done).copy(), roots=eng.root_states(),
                        harvest=_harvest(eng)))
    return out


def _harvest(eng):
    hv = eng.harvest()
    if hv is None or hv.n_games == 0:
        return None
    return {k: np.array(hv.view(k)) for k in ("slot", "n_moves", "winner", "score", "z", "own", "counts", "obs_bits")}


@functools.lru_cache(maxsize=None)
def _runs(S, G, back):
    states = _late_positions(S, G, back)
    out = {}
    for on in (False, True):
        eng = _engine(G, S, pass_alive_end=on)
        assert eng.get_pass_alive_end() == on
        out[on] = _play_out(eng, states, 3 * back + 8)
        out[on, "stats"] = eng.pass_alive_stats()
        assert eng.stats()["errors"] == 0
        eng.close()
    return states, out


@pytest.mark.parametrize("S,G,back", [(9, 8, 12), (19, 2, 6)])
def test_settled_games_end_and_are_scored_by_the_pass_alive_area(S, G, back):
    """With the mode on a game ends at the first root that the restatement calls settled, not before and not later; up to there visits
    and moves are the mode-off run's; z, ownership target, winner and score of every harvested game are the restatement's
    pass-alive-aware area of its last root."""
    states, runs = _runs(S, G, back)
    on, off = runs[True], runs[False]
    ended = {}
    b0, w0 = pa.stones_of_states(states, S)
    n_settled = sum(pa.settled(pa.pass_alive(b0[g], w0[g])) for g in range(G))      # (a start position that is settled already)
    assert n_settled == G - int(on[0]["live"].sum())
    n_override = 0
    for m, mv in enumerate(on):
        assert m < len(off)
        ref = off[m]
        for g in np.flatnonzero(mv["live"]):
            assert ref["live"][g]
            assert np.array_equal(mv["raw"][g], ref["raw"][g]) and mv["acts"][g] == ref["acts"][g], (g, m)
            b, w = pa.stones_of_states(mv["roots"][g], S)
            status = pa.pass_alive(b[0], w[0])
            if pa.settled(status) and not ref["done"][g]:
                assert mv["done"][g] == 1, (g, m, "a settled root did not end the game")
                n_settled += 1
            else:
                assert mv["done"][g] == ref["done"][g], (g, m)
            if mv["done"][g]:
                ended[g] = m
        hv = mv["harvest"]
        fin = [g for g in np.flatnonzero(mv["live"]) if mv["done"][g] == 1]
        assert (hv is None) == (len(fin) == 0)
        if hv is None:
            continue
        assert list(hv["slot"]) == fin
        at = 0
        for i, g in enumerate(fin):
            b, w = pa.stones_of_states(mv["roots"][g], S)
            score, own = pa.area_score(b[0], w[0], KOMI)
            n = int(hv["n_moves"][i])
            assert n == m + 1
            winner = 1 if score > 0 else 2
            assert hv["score"][i] == score and hv["winner"][i] == winner
            players = [int(x) for x in _players_of(on, g, m, states, S)]
            assert np.array_equal(hv["z"][at:at + n], np.array([1.0 if p == winner else -1.0 for p in players], np.float32))
            want_own = np.stack([own if p == 1 else -own for p in players]).astype(np.int8)
            assert np.array_equal(hv["own"][at:at + n].reshape(n, -1), want_own)
            tt = pa.tromp_taylor_owner(b[0], w[0])
            n_override += int(not np.array_equal(tt, own))
            at += n
    assert runs[True, "stats"]["games_settled"] == n_settled
    assert runs[False, "stats"]["games_settled"] == 0
    # the bars on the inputs at 19x19 (a game settles, a game does not, a settled game's score is not Tromp-Taylor's) are asserted in
    # tests/test_gpu_pass_alive_engine.py::test_engine_equals_the_oracle_driver, whose 19x19 games start at a hand-built position;
    # the random playout positions used here give no such guarantee at that size
    if S == 9:
        assert n_settled >= 1 and n_settled < G, n_settled               # some games end by settlement, some do not
        assert n_override >= 1                                           # and somewhere the override changes the area
    # the mode-off run goes on where the mode-on run stopped
    assert sum(int(mv["live"].sum()) for mv in off) >= sum(int(mv["live"].sum()) for mv in on)


def _players_of(run, g, last, states, S):
    """Side to move at every ply 0..last of game g: it alternates from the start position's."""
    first = int(np.asarray(states[g]).view(np.uint8)[2 * ((S * S + 63) // 64) * 8 + 11])
    return [first if t % 2 == 0 else 3 - first for t in range(last + 1)]


def test_root_read_out_equals_the_batched_kernel():
    states, _ = _runs(9, 8, 12)
    eng = _engine(8)
    eng.reset(np.arange(8) + 11)
    eng.reset_from(states)
    ro = eng.root_pass_alive()
    want = _env(9).pass_alive_batch(eng.root_states())
    assert np.array_equal(ro["status"], want["status"]) and np.array_equal(ro["settled"], want["settled"])
    from transgo_amd import analysis
    recs = analysis.analyse(eng, states, pass_alive=True)
    for g, r in enumerate(recs):
        assert np.array_equal(np.asarray(r["pass_alive"]).reshape(-1), want["status"][g]) and r["settled"] == bool(want["settled"][g])
        assert np.float32(r["pass_alive_score"]) == want["score"][g]
    eng.close()
