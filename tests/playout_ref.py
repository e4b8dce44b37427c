"""The random playout that tg_env_rollout must reproduce bit for bit, over any object with the reference GoEnv's method surface
(oracle.go_oracle.OracleGoEnv in the tests, the reference's own GoEnv in tests/golden/gen_playouts.py) and a
np.random.RandomState.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

NOEYE, LEGAL = "noeye", "legal"


def candidates(env, state, policy=NOEYE):
    """Ascending board points the random player draws from; pass is never among them.
    noeye: getLegalNoEye without its trailing pass (go_env.cc:171-181).  legal: the pass-filtered getLegalAction of
    environment.py:121-129 (a lone pass is filtered here too: pass is played only when the list is empty)."""
    P = env.board_size ** 2
    acts = env.getLegalNoEye(state) if policy == NOEYE else env.getLegalAction(state)
    return [int(a) for a in acts if int(a) != P]


def playout(env, state, rs, max_plies=None, policy=NOEYE, done=False):
    """-> (final state, moves, done, n_candidates per ply).  `done` = the state arrives terminated."""
    P = env.board_size ** 2
    moves, ncand = [], []
    while not done and (max_plies is None or len(moves) < max_plies):
        pts = candidates(env, state, policy)
        a = P if len(pts) == 0 else pts[0] if len(pts) == 1 else int(rs.choice(pts))     # a one-element choice makes NO draw
        state, done = env.step(state, a)
        moves.append(a); ncand.append(len(pts))
    return state, moves, bool(done), ncand


def key_checksum(rs):
    """A 64-bit digest of the 624 key words of a RandomState (position-weighted sum: any changed or moved word shows)."""
    return key_checksum_words(rs.get_state()[1])


def key_checksum_words(key):
    key = np.asarray(key, np.uint32).astype(np.uint64)
    return int((key * (np.arange(624, dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum())
