"""transgo_amd/pass_alive.py, the restatement of Benson's algorithm the kernels are tested against: hand-built positions with the
expected status written out, and a soundness property checked through the oracle rules (no GPU)."""
import numpy as np
import pytest

from oracle.go_oracle import OracleGoEnv
from tests import playout_ref
from tests.pass_alive_positions import HAND_9, HAND_19
from transgo_amd import pass_alive as pa
from transgo_amd.configure import Config


@pytest.mark.parametrize("name", sorted(HAND_9))
def test_hand_built_9x9(name):
    b, w, want = HAND_9[name]
    got = pa.pass_alive(b, w)
    assert got.dtype == np.int8 and np.array_equal(got, want), (name, got.reshape(9, 9))
    assert pa.settled(got) == (name == "settled")


@pytest.mark.parametrize("name", sorted(HAND_19))
def test_hand_built_19x19(name):
    b, w, want = HAND_19[name]
    got = pa.pass_alive(b, w)
    assert np.array_equal(got, want), (name, got.reshape(19, 19))
    assert pa.settled(got) == (name == "settled")


def test_area_score_overrides_tromp_taylor_inside_territory():
    b, w, st = HAND_9["territory_one_interior"]
    tt = pa.tromp_taylor_owner(b, w)
    score, own = pa.area_score(b, w, 7.5)
    assert tt[10] == -1 and own[10] == 1                               # the dead white stone at (1,1) counts for Black
    assert tt[0] == 0 and own[0] == 1                                  # ... and so do the empty points next to it (dame by Tromp-Taylor)
    assert score.dtype == np.float32 and score == np.float32(int((own == 1).sum()) - int((own == -1).sum())) - np.float32(7.5)
    b, w, st = HAND_9["settled"]
    score, own = pa.area_score(b, w, 7.5)
    assert score == np.float32(36 - 45 - 7.5) and np.array_equal(own, np.sign(st))
    assert pa.area_score(np.zeros(81, bool), np.zeros(81, bool), 7.5)[0] == np.float32(-7.5)


def test_config_field_defaults_off():
    assert Config().pass_alive_end is False
    assert Config(pass_alive_end=True).pass_alive_end is True


# ---- soundness, independent of the restatement's logic: the opponent can neither capture a pass-alive stone nor live in territory ----
SEEDS = list(range(16))
OPPONENT_MOVES = 300


def _stones(env, state):
    """(black, white) bool[P] from the oracle's encoding: planes 0-2 the mover's stones by liberty class, 3-5 the opponent's."""
    obs = env.encode(state).reshape(env.encoded_dim, -1)
    mine, theirs = obs[0:3].sum(0) > 0, obs[3:6].sum(0) > 0
    return (mine, theirs) if env.getPlayer(state) == 1 else (theirs, mine)


def _sampled_positions():
    env = OracleGoEnv(max_step=30000)
    out = []
    for seed in SEEDS:
        rs = np.random.RandomState(seed)
        state, _ = env.reset()
        _, moves, done, _ = playout_ref.playout(env, state, rs)
        assert done and moves[-1] == 81 and moves[-2] == 81             # a no-eye playout ends by two passes
        state, _ = env.reset()
        for a in moves[:-2]:
            state, d = env.step(state, a)
            assert not d
        out.append(state)
    return env, out


def _two_eyed_groups(stones, nb):
    """Points of the groups of `stones` that have two empty points whose neighbours all belong to the group."""
    lab = pa.components(stones, nb)
    eyes = {}
    for p in range(len(stones)):
        if stones[p]:
            continue
        ls = {int(lab[q]) for q in nb[p]}
        if len(ls) == 1 and -1 not in ls:
            l = ls.pop()
            eyes[l] = eyes.get(l, 0) + 1
    out = np.zeros(len(stones), bool)
    for l, n in eyes.items():
        if n >= 2:
            out |= lab == l
    return out


def test_soundness_under_random_attack():
    env, positions = _sampled_positions()
    nb = pa.neighbours(9)
    n_alive = n_settled = 0
    for seed, start in zip(SEEDS, positions):
        b, w = _stones(env, start)
        status = pa.pass_alive(b, w)
        n_alive += bool((np.abs(status) == 2).any())
        n_settled += pa.settled(status)
        for X in (1, 2):
            sgn = 1 if X == 1 else -1
            safe = status == 2 * sgn
            terr = status == sgn
            if not safe.any():
                continue
            rs = np.random.RandomState(1000 + seed)
            state = start
            for _ in range(OPPONENT_MOVES):
                if env.getPlayer(state) == X:
                    state, done = env.step(state, 81)
                else:
                    acts = [int(a) for a in env.getLegalAction(state)]
                    state, done = env.step(state, acts[rs.randint(len(acts))])
                if done:
                    break
                nbk, nwh = _stones(env, state)
                mine, theirs = (nbk, nwh) if X == 1 else (nwh, nbk)
                assert mine[safe].all(), (seed, X, "a pass-alive stone was captured")
                assert not (_two_eyed_groups(theirs, nb) & terr).any(), (seed, X, "the opponent lives inside pass-alive territory")
    # the bar on the inputs: the playouts' ends must exercise the analysis
    assert n_alive * 4 >= len(SEEDS), n_alive
    assert n_settled >= 2, n_settled
