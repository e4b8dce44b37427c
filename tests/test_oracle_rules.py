"""oracle/go_oracle.c against golden vectors recorded from the compiled reference rules engine
(tests/golden/gen_fixtures.py rules): legal sets, no-eye sets, checkAction, all 10 feature planes, player, step,
score, territory and done flags for every ply of 160 random + 6 crafted games (ko, suicide, double pass, illegal
moves left unchanged, stepping a finished game)."""
import os

import numpy as np

from oracle.go_oracle import OracleGoEnv
from tests import rules_replay


def test_rules_fixture(golden_dir):
    blob = rules_replay.load(golden_dir)
    n = rules_replay.replay(OracleGoEnv(), blob)
    assert n > 15000


def test_reset_and_empty_board():
    env = OracleGoEnv()
    s, done = env.reset()
    assert not done and env.getPlayer(s) == 1 and env.getStep(s) == 1
    assert env.getScore(s) == -7.5                      # board.cc:932-935 + go_env.cc:129
    assert list(env.getLegalAction(s)) == list(range(81))
    assert env.encode(s).sum() == 0


def test_pass_only_when_no_point_is_legal():
    """environment.py:121-129: pass is reported only when it is the only move."""
    env = OracleGoEnv()
    s, _ = env.reset()
    assert 81 not in list(env.getLegalAction(s))


def test_max_step_cutoff():
    env = OracleGoEnv(max_step=5)
    s, _ = env.reset()
    for i, a in enumerate([0, 1, 2, 3]):
        s, done = env.step(s, a)
        assert not done
    s, done = env.step(s, 4)                            # step_count becomes 6 > 5 (go_env.cc:67)
    assert done and env.isTerminated(s)


def test_against_compiled_reference_19x19_logic_is_size_generic(golden_dir):
    """Size-generic code paths: the same oracle binary at S=9 equals the compiled reference on 40 more random games (not the
    rules fixture's seeds), recorded ply by ply from the reference's C ABI in tests/golden/compiled_ref_s9.npz
    (tests/golden/gen_compiled_ref.py)."""
    with np.load(os.path.join(golden_dir, "compiled_ref_s9.npz")) as z:
        rec = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("generic/")}
    env = OracleGoEnv()
    game, off = rec["game"], rec["legal_off"]
    assert len(np.unique(game)) == 40
    b = None
    for i in range(len(game)):
        if i == 0 or game[i] != game[i - 1]:
            b, _ = env.reset()
        la = [int(x) for x in rec["legal"][off[i]:off[i + 1]]]
        assert la == [int(x) for x in env.getLegalAction(b)], i
        assert (rec["enc"][i] == env.encode(b).reshape(-1)).all(), i
        assert rec["score"][i] == env.getScore(b), i
        if env.getStep(b) % 16 == 1:                     # the reference prints a line for every refusal: sampled, not flooded
            assert (rec["check"][i] >= 0).all()
            for c, want in zip((81, -1, -2), rec["check"][i]):   # S*S is NOT translated to PASS here (only Step does that)
                assert bool(want) == bool(env.checkAction(b, c)), (i, c)
        assert bool(rec["terminated"][i]) == bool(env.isTerminated(b)), i
        assert rec["player"][i] == env.getPlayer(b) and rec["step"][i] == env.getStep(b), i
        b, d2 = env.step(b, int(rec["action"][i]))
        assert bool(rec["done"][i]) == d2, i
        assert d2 == (i + 1 == len(game) or game[i + 1] != game[i]), i


def test_rules_fixture_19x19(golden_dir):
    """19x19 games recorded from a 19x19 build of the reference engine (tests/golden/gen_rules19.py)."""
    blob = rules_replay.load(golden_dir, "rules_s19.npz")
    n = rules_replay.replay(OracleGoEnv(board_size=19, max_step=int(blob["max_step"])), blob)
    assert n > 1500


def test_encode_9_and_13_planes_match_the_reference_engine(golden_dir):
    from tests import rules_replay
    blob = rules_replay.load(golden_dir, "rules_enc_variants_s9.npz")
    n = rules_replay.replay_encode_variants(lambda d: OracleGoEnv(encode_dim=d), blob)
    assert n > 2000
