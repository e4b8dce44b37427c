"""Random-playout fixture: the loop of tests/playout_ref.py played on the REFERENCE's own GoEnv (9x9: GoEnv/environment.py over
the compiled reference engine, through ref_harness; 19x19: the scratch 19x19 build of gen_rules19.py, outside the repository,
behind a few lines of ctypes with the same method names).  Per game: the moves, the number of candidates at every ply, plies,
done, final score and territory, and the RandomState behind the last draw (position + key checksum).  Only the recorded data
(tests/golden/playouts.npz) is committed.

9x9: 32 seeds x both candidate policies at max_step 200 (the reference's default of 120 cuts every no-eye game before its double
pass); 19x19: 4 seeds, no-eye, max_step 450."""
import ctypes
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import playout_ref  # noqa: E402

MAX_STEP9, MAX_STEP19 = 200, 450
SEEDS9, SEEDS19 = list(range(1000, 1032)), [19, 20, 21, 22]


class Ref19:
    """The 19x19 build of the reference engine with the method names of GoEnv/environment.py."""
    board_size = 19

    def __init__(self, so, max_step):
        self.lib = ctypes.CDLL(so)
        self.St = ctypes.c_char * 32768
        self.lib.Init.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float]
        self.lib.Step.restype = ctypes.c_bool
        self.lib.getTerritory.restype = ctypes.c_float
        self.lib.Init(1, 10, max_step, 7.5)

    def reset(self):
        st = self.St(); self.lib.Reset(st)
        return st, False

    def step(self, state, action):
        nxt = self.St()
        return nxt, bool(self.lib.Step(state, nxt, ctypes.c_int(int(action))))

    def _list(self, fn, state):
        buf = (ctypes.c_int * 362)()
        return np.array(buf[:fn(state, buf)], np.int32)

    def getLegalNoEye(self, state):
        return self._list(self.lib.getLegalNoEye, state)

    def getLegalAction(self, state):
        acts = self._list(self.lib.getLegalAction, state)
        return acts if len(acts) == 1 else [a for a in acts if a != 361]

    def getScoreAndTerritory(self, state):
        terr = np.zeros(361, np.float32)
        return self.lib.getTerritory(state, terr.ctypes.data_as(ctypes.c_void_p)), terr


def play(env, seeds, policy, max_step, tag, out):
    P = env.board_size ** 2
    n = len(seeds)
    moves = np.full((n, max_step), -1, np.int16); ncand = np.full((n, max_step), -1, np.int16)
    plies = np.zeros(n, np.int32); done = np.zeros(n, np.uint8); score = np.zeros(n, np.float32)
    terr = np.zeros((n, P), np.int8); pos = np.zeros(n, np.int32); ksum = np.zeros(n, np.uint64)
    for i, seed in enumerate(seeds):
        rs = np.random.RandomState(seed)
        st, _ = env.reset()
        st, mv, d, nc = playout_ref.playout(env, st, rs, None, policy)
        plies[i], done[i] = len(mv), d
        moves[i, :len(mv)] = mv; ncand[i, :len(mv)] = nc
        s, t = env.getScoreAndTerritory(st)
        score[i] = s; terr[i] = np.asarray(t).astype(np.int8)
        pos[i], ksum[i] = rs.get_state()[2], playout_ref.key_checksum(rs)
    for k, v in dict(seeds=np.asarray(seeds, np.int64), moves=moves, ncand=ncand, plies=plies, done=done, score=score, terr=terr,
                     pos=pos, ksum=ksum, max_step=np.int64(max_step)).items():
        out[f"{tag}/{k}"] = v
    return moves, ncand, plies


def main():
    from ref_harness import load_reference
    from gen_rules19 import build as build19
    cwd = os.getcwd()
    ref = load_reference()
    out = {}
    env = ref.environment.GoEnv(ref.cfg)
    env.c_init(env.history_dim, env.encoded_dim, MAX_STEP9, env.komi)          # the reference's own Init, with a longer game
    env.max_step = MAX_STEP9
    for policy in (playout_ref.NOEYE, playout_ref.LEGAL):
        moves, ncand, plies = play(env, SEEDS9, policy, MAX_STEP9, f"s9_{policy}", out)
        print(policy, "plies", plies.min(), plies.max(), "one-candidate plies", int((ncand == 1).sum()), "no-candidate plies",
              int((ncand == 0).sum()), "ended before max_step", int((plies < MAX_STEP9).sum()))
    nc = out["s9_noeye/ncand"]
    assert (nc == 1).any() and (nc == 0).any(), "no-draw rule not exercised: add seeds"
    assert (out["s9_noeye/plies"] < MAX_STEP9).any(), "every 9x9 game is cut by max_step"
    os.chdir(cwd)
    tmp, so = build19()
    try:
        _, ncand, plies = play(Ref19(so, MAX_STEP19), SEEDS19, playout_ref.NOEYE, MAX_STEP19, "s19_noeye", out)
        print("19x19 plies", plies)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(HERE, "playouts.npz")
    np.savez_compressed(path, **out)
    print("playouts.npz bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
