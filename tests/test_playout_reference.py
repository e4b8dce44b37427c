"""tests/playout_ref.py over the CPU oracle against random playouts recorded from the reference's own engine
(tests/golden/playouts.npz, tests/golden/gen_playouts.py): the loop tg_env_rollout must reproduce, pinned without a GPU."""
import os

import numpy as np
import pytest

from oracle.go_oracle import OracleGoEnv
from tests import playout_ref


@pytest.fixture(scope="module")
def fixture(golden_dir):
    with np.load(os.path.join(golden_dir, "playouts.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag,size", [("s9_noeye", 9), ("s9_legal", 9), ("s19_noeye", 19)])
def test_playout_ref_reproduces_every_fixture_game(fixture, tag, size):
    policy = tag.split("_")[1]
    max_step = int(fixture[f"{tag}/max_step"])
    env = OracleGoEnv(board_size=size, max_step=max_step)
    seeds = fixture[f"{tag}/seeds"]
    assert len(seeds) == (32 if size == 9 else 4)
    for i, seed in enumerate(seeds):
        rs = np.random.RandomState(int(seed))
        st, _ = env.reset()
        st, moves, done, ncand = playout_ref.playout(env, st, rs, None, policy)
        n = int(fixture[f"{tag}/plies"][i])
        assert len(moves) == n and done == bool(fixture[f"{tag}/done"][i]), (tag, i)
        assert moves == list(fixture[f"{tag}/moves"][i][:n]) and (fixture[f"{tag}/moves"][i][n:] == -1).all(), (tag, i)
        assert ncand == list(fixture[f"{tag}/ncand"][i][:n]), (tag, i)
        score, terr = env.getScoreAndTerritory(st)
        assert score == fixture[f"{tag}/score"][i] and (terr.astype(np.int8) == fixture[f"{tag}/terr"][i]).all(), (tag, i)
        assert rs.get_state()[2] == fixture[f"{tag}/pos"][i] and playout_ref.key_checksum(rs) == int(fixture[f"{tag}/ksum"][i]), (tag, i)


def test_fixture_exercises_the_no_draw_rule_and_the_double_pass(fixture):
    """At 9x9 at least one ply has exactly one candidate (a choice that makes no draw) and at least one has none (a pass), and
    not every game is cut by max_step: some end by double pass."""
    nc = fixture["s9_noeye/ncand"]
    assert (nc == 1).any() and (nc == 0).any()
    plies, max_step = fixture["s9_noeye/plies"], int(fixture["s9_noeye/max_step"])
    ended = plies < max_step
    assert ended.any()
    P = 81
    for i in np.flatnonzero(ended):
        assert list(fixture["s9_noeye/moves"][i][plies[i] - 2:plies[i]]) == [P, P] and fixture["s9_noeye/done"][i]


def test_a_one_element_choice_draws_nothing():
    """The rule the kernel's choice_index(1) follows: the stream stands still over a ply with one candidate."""
    env = OracleGoEnv(max_step=200)
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "playouts.npz")) as z:
        nc, moves, seed = z["s9_noeye/ncand"], z["s9_noeye/moves"], z["s9_noeye/seeds"]
    i, p = np.argwhere(nc == 1)[0]
    rs = np.random.RandomState(int(seed[i]))
    st, _ = env.reset()
    st, mv, _, _ = playout_ref.playout(env, st, rs, int(p), "noeye")
    before = (rs.get_state()[2], playout_ref.key_checksum(rs))
    st, one, _, n1 = playout_ref.playout(env, st, rs, 1, "noeye")
    assert n1 == [1] and one == [int(moves[i][p])] and before == (rs.get_state()[2], playout_ref.key_checksum(rs))
