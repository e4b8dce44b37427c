"""Test helper: whole games of the oracle search (oracle/wp_mcts.py and its root-rule subclasses) from a given position, with the
pass-alive end and scoring of DESIGN.md 16 stated on top -- a game ends after the move that leaves a settled root
(transgo_amd/pass_alive.py), and every finished game is scored by the pass-alive-aware area -- and the arrays tg_sp_harvest must
deliver for them.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle.go_oracle import OracleGoEnv
from oracle.wp_mcts import OracleSearch, Vertex, temperature
from transgo_amd import pass_alive as pa

R = 4
KOMI = 7.5


def stones(env, state):
    """(black, white) bool[P] from the oracle's encoding: planes 0-2 the mover's stones by liberty class, 3-5 the opponent's."""
    obs = env.encode(state).reshape(env.encoded_dim, -1)
    mine, theirs = obs[0:3].sum(0) > 0, obs[3:6].sum(0) > 0
    return (mine, theirs) if env.getPlayer(state) == 1 else (theirs, mine)


def is_settled(env, state):
    b, w = stones(env, state)
    return pa.settled(pa.pass_alive(b, w))


def search_class(rule, ownership):
    if rule == "forced":
        from tests.forced_playouts_ref import ForcedOracleSearch as base
    elif rule == "gumbel":
        from tests.gumbel_ref import GumbelOracleSearch as base
    else:
        base = OracleSearch
    if ownership:
        from tests.search_ownership_ref import OwnershipMixin
        return type("Own" + base.__name__, (OwnershipMixin, base), {})
    return base


def raw_counts(o):
    return np.array([o.root.kids[a].n if a in o.root.kids else 0 for a in range(o.A)])


def fast_move(o):
    """A fast search of playout cap randomization: no root noise, the self-play temperature all the same."""
    n0 = o.root.n
    while o.root.n < n0 + o.num_simulation:
        o.wave()
    raw = raw_counts(o)
    counts = np.where(raw == 1, 0, raw)
    powed = np.power(counts, 1.0 / temperature(o.env.getStep(o.root.state)))
    return o.rng.choice(np.arange(o.A), p=np.array(powed) / np.sum(powed)), raw


def pack_obs(obs):
    """float planes [n][C][S][S] -> the bit-packed rows of the record (bit i = plane-major flat index i, u32 words)."""
    obs = np.asarray(obs)
    flat = obs.reshape(len(obs), int(np.prod(obs.shape[1:]))) != 0
    W = (flat.shape[1] + 31) // 32
    bits = np.zeros((len(obs), W * 32), np.uint8)
    bits[:, :flat.shape[1]] = flat
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(len(obs), W)


def play_game(evaluate, seed, start_moves, sims, board_size=9, max_step=400, pass_alive=True, rule="plain", rule_kw=None,
              ownership=False, cap=None, max_moves=400):
    """One game from the position behind `start_moves`, searched move by move until the rules or settlement end it.
    cap(t) -> (full, simulations) per ply (playout cap randomization: a fast ply has no root noise and is not recorded).
    -> dict(plies=[dict(raw, action, player, recorded)], ended 'start' | 'rules' | 'settled' | None, and the finished game's
    n_recorded, score, winner, tt_score, obs_bits, counts, z, own, player over its recorded plies)."""
    S = board_size
    env = OracleGoEnv(board_size=S, max_step=max_step)
    rng = np.random.RandomState(int(seed))
    o = search_class(rule, ownership)(env, evaluate, rng, num_simulation=sims, parallel_readouts=R, board_size=S, **(rule_kw or {}))
    state, _ = env.reset()
    for a in start_moves:
        state, done = env.step(state, int(a))
        assert not done
    o.root = Vertex(0)
    o.root.state = state
    o._open_root(o.root)
    out = dict(plies=[], ended=None)
    if pass_alive and is_settled(env, state):
        out["ended"] = "start"
        return out
    obs, counts = [], []
    while len(out["plies"]) < max_moves:
        full, o.num_simulation = cap(len(out["plies"])) if cap else (True, sims)
        player, ob = int(env.getPlayer(o.root.state)), env.encode(o.root.state)
        if full:
            a, _, _, info = o.search_move(True)
            raw = raw_counts(o)
            rec = info["pruned"] if info.get("forced") else np.asarray(info["record"]) if "record" in info else raw
        else:
            a, raw = fast_move(o)
            rec = raw
        done = o.advance(a)
        out["plies"].append(dict(raw=raw, action=int(a), player=player, recorded=bool(full)))
        if full:
            obs.append(ob); counts.append(np.asarray(rec, np.int64).astype(np.int32))
        if done:
            out["ended"] = "rules"
        elif pass_alive and is_settled(env, o.root.state):
            out["ended"] = "settled"
        if out["ended"]:
            break
    if out["ended"]:
        b, w = stones(env, o.root.state)
        tt_score = np.float32(env.getScore(o.root.state))
        if pass_alive:
            score, own = pa.area_score(b, w, KOMI)
        else:
            score, own = tt_score, np.asarray(env.getScoreAndTerritory(o.root.state)[1]).astype(np.int8)
        winner = 1 if score > 0 else 2
        pl = np.array([p["player"] for p in out["plies"] if p["recorded"]], np.uint8)
        n = len(pl)
        out.update(n_recorded=n, score=np.float32(score), winner=winner, tt_score=tt_score, tt_winner=1 if tt_score > 0 else 2, terr=own,
                   obs_bits=pack_obs(np.array(obs, np.float32).reshape(n, env.encoded_dim, S, S)),
                   counts=np.array(counts, np.int32).reshape(n, S * S + 1), player=pl,
                   z=np.where(pl == winner, 1.0, -1.0).astype(np.float32),
                   own=np.where((pl == 1)[:, None], own[None, :], -own[None, :]).astype(np.int8).reshape(n, S * S))
    return out
