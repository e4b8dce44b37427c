"""The pass-alive end of self-play (tg_sp_pass_alive, k_pa_end, k_harvest_pa) against tests/pass_alive_ref.py driving the
oracle search with the same rule: moves, visit counts, the ply at which each game ends, done, tg_sp_finished and every byte of the
harvested z, own, counts, obs_bits and player -- plain, with the mode off, under the playout cap, forced playouts, Gumbel, search
ownership and policy surprise, and across a snapshot.

9x9 games start at no-eye playout positions twelve plies before their end; the 19x19 games at a hand-built position one dame away
from settled whose corner holds a dead stone (tests/pass_alive_positions.near_settled_19).  Oracle games and engine runs are
computed once and shared."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import evaluators
from tests import pass_alive_ref as ref
from tests.pass_alive_positions import move_sequence, near_settled_19

pytestmark = pytest.mark.gpu
SIMS, FAST = {9: 24, 19: 8}, 12           # simulations per move by board size (chosen on the CPU with the driver: see the bars below)
G9, BACK, MAX_STEP9 = 8, 12, 170
SEED0 = 11
RULES = {                      # name -> (oracle rule, oracle kwargs, engine kwargs, search ownership)
    "plain": ("plain", {}, {}, False),
    "forced": ("forced", dict(forced_k=2.0), dict(forced_playouts_k=2.0), False),
    "gumbel": ("gumbel", dict(gumbel_m=8), dict(gumbel_m=8), False),
    "ownership": ("plain", {}, dict(search_ownership=True), True),
    "cap": ("plain", {}, {}, False),
}


def _cap(g):
    return lambda t: ((t + g) % 2 == 0, SIMS[9] if (t + g) % 2 == 0 else FAST)


@functools.lru_cache(maxsize=None)
def _starts(S):
    """(device states [G][ssz], the plies that lead to them per game, max_step)"""
    from transgo_amd.environment import GoEnv
    if S == 9:
        env = GoEnv(config=type("C", (), dict(max_step=MAX_STEP9, board_size=9))())
        seeds = np.arange(G9) + 40
        full = env.rollout_batch(env.reset_batch(G9), seeds=seeds, policy="noeye")
        assert full["done"].all()
        r = env.rollout_batch(env.reset_batch(G9), seeds=seeds, max_plies=np.maximum(full["plies"] - BACK, 0), policy="noeye", record=True)
        return r["states"], [[int(a) for a in m[:n]] for m, n in zip(r["moves"], r["plies"])], MAX_STEP9
    seq = move_sequence(*near_settled_19(((9, 8),)), 19)
    max_step = len(seq) + 6                                            # six plies left: one game fills the dame, the other runs out
    env = GoEnv(config=type("C", (), dict(max_step=max_step, board_size=19))())
    st = env.reset_batch(1)
    for a in seq:
        st, done, ok = env.step_batch(st, [a])
        assert ok[0] and not done[0]
    return np.repeat(st, 2, axis=0), [seq, seq], max_step


def _evaluator(own):
    if not own:
        return evaluators.flat
    from tests import search_ownership_ref as so
    return so.with_own("flat", so.own_tenths)


@functools.lru_cache(maxsize=None)
def _oracle(S, rule="plain", on=True):
    _, moves, max_step = _starts(S)
    orule, okw, _, own = RULES[rule]
    return [ref.play_game(_evaluator(own), SEED0 + g, moves[g], SIMS[S], S, max_step, pass_alive=on, rule=orule, rule_kw=okw, ownership=own,
                          cap=_cap(g) if rule == "cap" else None) for g in range(len(moves))]


def _engine(S, rule, on, **kw):
    from transgo_amd.engine import SelfPlayEngine
    states, _, max_step = _starts(S)
    _, _, ekw, own = RULES[rule]
    return SelfPlayEngine(len(states), board_size=S, num_simulation=SIMS[S], parallel_readouts=ref.R, max_step=max_step,
                          evaluator=_evaluator(own), pass_alive_end=on, **ekw, **kw)


def _one_move(eng, rule, m, seeds=None):
    live = ~eng.finished
    if rule == "cap":
        full = np.array([_cap(g)(m)[0] for g in range(eng.G)])
        eng.search(True, np.where(full, SIMS[9], FAST), noise=full, record=full)
    else:
        eng.search(True)
    raw, _, _, st, _ = eng.root_info(obs=False)
    if rule == "forced":
        acts = eng.choose_moves(eng.root_visits(pruned=True)[0], st)[0]
    elif rule == "gumbel":
        acts = eng.choose_gumbel_moves(raw, st)[0]
    else:
        acts = eng.choose_moves(raw, st)[0]
    done = eng.play(acts)
    ng, npos = ctypes.c_int32(), ctypes.c_int32()
    eng.ctx.call("tg_sp_finished", ctypes.byref(ng), ctypes.byref(npos))
    hv = eng.harvest(seeds=seeds)
    keys = ("slot", "n_moves", "winner", "score", "terr", "z", "own", "counts", "obs_bits", "player")
    return dict(live=live, raw=raw, acts=np.asarray(acts).copy(), done=np.asarray(done).copy(), finished=(ng.value, npos.value),
                harvest=None if hv is None else {k: np.array(hv.view(k)) for k in keys})


def _run_engine(eng, S, rule, first=0, last=400, seeds=None):
    out = []
    for m in range(first, last):
        if eng.finished.all():
            break
        out.append(_one_move(eng, rule, m, seeds))
    return out


@functools.lru_cache(maxsize=None)
def _run(S, rule="plain", on=True):
    states, _, _ = _starts(S)
    eng = _engine(S, rule, on)
    eng.reset(np.arange(len(states)) + SEED0)
    eng.reset_from(states)
    start_live = ~eng.finished
    out = _run_engine(eng, S, rule)
    stats = eng.pass_alive_stats()
    assert eng.stats()["errors"] == 0
    eng.close()
    return start_live, out, stats


def _compare(run, games, first=0):
    """Every way the engine's moves and harvests differ from the oracle's games (empty = equal)."""
    bad = []
    for k, mv in enumerate(run):
        m = first + k
        fin = []
        for g in np.flatnonzero(mv["live"]):
            gm = games[g]
            if m >= len(gm["plies"]):
                bad.append((g, m, "the oracle's game is over")); continue
            ply = gm["plies"][m]
            if not np.array_equal(mv["raw"][g], ply["raw"]):
                bad.append((g, m, "raw root visits"))
            if int(mv["acts"][g]) != ply["action"]:
                bad.append((g, m, "action"))
            over = m == len(gm["plies"]) - 1 and gm["ended"] is not None
            if bool(mv["done"][g]) != over:
                bad.append((g, m, f"done {mv['done'][g]} but the oracle's game ended: {gm['ended']} at ply {len(gm['plies'])}"))
            if over:
                fin.append(g)
        want_fin = (len(fin), sum(games[g]["n_recorded"] for g in fin))
        if mv["finished"] != want_fin:
            bad.append((m, f"tg_sp_finished {mv['finished']} != {want_fin}"))
        hv = mv["harvest"]
        if (hv is None) != (len(fin) == 0):
            bad.append((m, "harvest present / absent")); continue
        if hv is None:
            continue
        if list(hv["slot"]) != fin or list(hv["n_moves"]) != [games[g]["n_recorded"] for g in fin]:
            bad.append((m, "slot / n_moves", list(hv["slot"]), list(hv["n_moves"]))); continue
        for i, g in enumerate(fin):
            if hv["winner"][i] != games[g]["winner"] or np.float32(hv["score"][i]) != games[g]["score"]:
                bad.append((g, m, "winner / score"))
            if not np.array_equal(hv["terr"][i].reshape(-1), games[g]["terr"]):
                bad.append((g, m, "terr"))
        for key in ("z", "own", "counts", "obs_bits", "player"):
            want = np.concatenate([games[g][key] for g in fin])
            got = hv[key].reshape(want.shape) if hv[key].size == want.size else hv[key]
            if got.shape != want.shape or got.tobytes() != want.astype(got.dtype).tobytes():
                bad.append((m, "harvested " + key))
    return bad


def _check(S, rule, on=True):
    start_live, run, stats = _run(S, rule, on)
    games = _oracle(S, rule, on)
    assert list(start_live) == [g["ended"] != "start" for g in games]
    assert _compare(run, games) == []
    assert sum(len(g["plies"]) for g in games) == sum(int(mv["live"].sum()) for mv in run)
    settled = [g for g in games if g["ended"] in ("settled", "start")]
    assert stats["games_settled"] == (len(settled) if on else 0)
    assert stats["plies_at_settlement_sum"] == (sum(len(g["plies"]) for g in settled) if on else 0)
    return games


@pytest.mark.parametrize("S", [9, 19])
def test_engine_equals_the_oracle_driver(S):
    games = _check(S, "plain")
    by_settlement = [g for g in games if g["ended"] == "settled"]
    # the bar on the inputs, both sizes: a game ends by settlement before max_step, a game does not, and for a game that ended by
    # settlement the score or the winner is not plain Tromp-Taylor's
    assert len(by_settlement) >= 1 and any(g["ended"] == "rules" for g in games)
    assert any(g["score"] != g["tt_score"] or g["winner"] != g["tt_winner"] for g in by_settlement)


@pytest.mark.parametrize("S", [9, 19])
def test_mode_off_is_the_existing_engine_path(S):
    """The mode-off run equals the oracle driver without the rule, and up to each game's settlement ply the mode-on run's visits and
    moves are the mode-off run's."""
    _check(S, "plain", on=False)
    _, on, _ = _run(S, "plain", True)
    _, off, _ = _run(S, "plain", False)
    assert len(off) >= len(on)
    for a, b in zip(on, off):
        live = a["live"]
        assert b["live"][live].all()
        assert np.array_equal(a["raw"][live], b["raw"][live]) and np.array_equal(a["acts"][live], b["acts"][live])


@pytest.mark.parametrize("rule", ["cap", "forced", "gumbel", "ownership"])
def test_combinations_equal_the_oracle_driver(rule):
    games = _check(9, rule)
    assert any(g["ended"] == "settled" for g in games)
    if rule == "cap":                                                  # a settled game with plies kept out of its record
        assert any(g["ended"] == "settled" and g["n_recorded"] < len(g["plies"]) for g in games)


def test_policy_surprise_harvest_of_settled_games():
    """With policy surprise weighting on, the resampled harvest equals the definition applied to the oracle driver's plain harvest."""
    from tests import policy_surprise_ref as psr
    from transgo_amd import records
    states, _, _ = _starts(9)
    games = _oracle(9, "plain", True)
    seeds = (np.arange(G9) + SEED0).astype(np.uint32)
    eng = _engine(9, "plain", True, policy_surprise_weight=0.5, policy_surprise_seed=3)
    eng.reset(seeds)
    eng.reset_from(states)
    n_games = 0
    for m in range(400):
        if eng.finished.all():
            break
        live = ~eng.finished
        eng.search(True)
        raw, _, _, st, _ = eng.root_info(obs=False)
        done = eng.play(eng.choose_moves(raw, st)[0])
        fin = [g for g in np.flatnonzero(live) if done[g]]
        assert fin == [g for g in np.flatnonzero(live) if m == len(games[g]["plies"]) - 1]
        hv = eng.harvest(seeds=seeds)
        assert (hv is None) == (len(fin) == 0)
        if hv is None:
            continue
        cat = lambda k: np.concatenate([games[g][k] for g in fin])
        plain = records.from_arrays(9, 10, np.array([games[g]["n_recorded"] for g in fin], np.int32), np.array([games[g]["winner"] for g in fin], np.int32),
                                    np.stack([games[g]["terr"] for g in fin]).astype(np.int8), cat("obs_bits"), cat("counts"), cat("z"), cat("own"),
                                    cat("player"), slot=np.array(fin, np.int32), seed=seeds[fin], score=np.array([games[g]["score"] for g in fin], np.float32))
        prior = np.ascontiguousarray(evaluators.flat(plain.observations())[0], np.float32)
        want, _ = psr.resample(plain, prior, 0.5, 3)
        for k in ("n_moves", "winner", "z", "own", "counts", "obs_bits", "player"):
            assert np.array(hv.view(k)).tobytes() == np.array(want.view(k)).tobytes(), (m, k)
        n_games += len(fin)
    eng.close()
    assert n_games == sum(g["ended"] in ("settled", "rules") for g in games) and any(g["ended"] == "settled" for g in games)


def test_snapshot_mid_run_with_the_mode_on():
    """A snapshot taken after two moves and restored into a fresh context with the mode set: the rest of the run -- moves, visits,
    ends and harvests -- is bit-identical, the games that k_pa_end terminated before the snapshot stay finished."""
    states, _, _ = _starts(9)
    _, whole, _ = _run(9, "plain", True)
    eng = _engine(9, "plain", True)
    eng.reset(np.arange(G9) + SEED0)
    eng.reset_from(states)
    head = _run_engine(eng, 9, "plain", 0, 2)
    snap, fin = eng.snapshot(), eng.finished.copy()
    eng.close()
    eng = _engine(9, "plain", True)                                    # the switch is context state: set before restoring
    eng.reset(np.arange(G9) + 99)
    eng.restore(snap)
    eng.finished = fin
    tail = _run_engine(eng, 9, "plain", 2)
    eng.close()
    assert len(head) + len(tail) == len(whole)
    for a, b in zip(head + tail, whole):
        assert np.array_equal(a["live"], b["live"]) and np.array_equal(a["raw"][a["live"]], b["raw"][b["live"]])
        assert np.array_equal(a["acts"][a["live"]], b["acts"][b["live"]]) and np.array_equal(a["done"], b["done"]) and a["finished"] == b["finished"]
        assert (a["harvest"] is None) == (b["harvest"] is None)
        if a["harvest"] is not None:
            for k in a["harvest"]:
                assert a["harvest"][k].tobytes() == b["harvest"][k].tobytes(), k
    assert any(mv["done"].any() for mv in tail)
