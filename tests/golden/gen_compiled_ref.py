"""Fixture for the tests that used to call the compiled reference engine live (oracle/_ref/GoEnv/go_env.so, `make -C oracle ref`):
the same seeded call sequences, run through the reference's own C ABI once, every return value and output buffer recorded.  The
tests replay the recorded actions through this repository's engines and compare call by call, so they no longer need the
reference tree where they run.  Output: tests/golden/compiled_ref_s9.npz.

    subenc/*     getSubEncode on seeded random planes, window sizes 7 and 5, 1 / 4 / 5 cuts (test_cabi_symbols.py)
    generic/*    40 random games (seed 99): legal list, encoding, score, player, step, terminated, sampled checkAction, done per
                 ply (test_oracle_rules.py)
    lockstep/*   12 games (seed 515) over all 15 go_env.h symbols: refused moves, Step and the in-place Step_, two calls on every
                 finished game (test_gpu_rules.py)
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "GoEnv", "go_env.so")
P = 81
LOCKSTEP_CHECKS = (-2, -1, P, 0, 13, 40, 67, 80)
GENERIC_CHECKS = (81, -1, -2)


def _ragged(lists):
    """list of int lists -> (flat int16 values, int32 offsets of length n + 1); order kept."""
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int32)
    flat = np.array([v for x in lists for v in x], np.int16)
    return flat, off


def gen_subenc(lib):
    rs = np.random.RandomState(3)
    out = {}
    for sub_size in (7, 5):
        for cuts in (1, 4, 5):
            enc = (rs.rand(10, 9, 9) < 0.3).astype(np.float32)
            a = np.full((5, 10, sub_size, sub_size), -1, np.float32)
            lib.getSubEncode(enc.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p), sub_size, 10, cuts)
            out[f"subenc/{sub_size}_{cuts}/enc"] = enc.astype(np.uint8)
            out[f"subenc/{sub_size}_{cuts}/out"] = a
    return out


def gen_generic(lib):
    lib.Init(1, 10, 120, 7.5)
    rng = np.random.RandomState(99)
    rec = {k: [] for k in ("game", "legal", "enc", "score", "check", "terminated", "player", "step", "action", "done")}
    for g in range(40):
        a = ctypes.create_string_buffer(1200); lib.Reset(a)
        done = False
        while not done:
            buf = (ctypes.c_int * 82)()
            n = lib.getLegalAction(a, buf)
            la = list(buf[:n]); la = la if n == 1 else la[:-1]
            e = np.zeros(810, np.float32); lib.Encode(a, e.ctypes.data_as(ctypes.c_void_p))
            step = lib.getStep(a)
            chk = [int(bool(lib.checkAction(a, ctypes.c_int(c)))) for c in GENERIC_CHECKS] if step % 16 == 1 else [-1] * 3
            rec["game"].append(g); rec["legal"].append(la); rec["enc"].append(e.astype(np.uint8))
            rec["score"].append(lib.getScore(a)); rec["check"].append(chk); rec["terminated"].append(bool(lib.isTerminated(a)))
            rec["player"].append(lib.getPlayer(a) & 0xFF); rec["step"].append(step)
            act = la[rng.randint(len(la))] if rng.rand() > 0.04 else 81
            a2 = ctypes.create_string_buffer(1200)
            done = bool(lib.Step(a, a2, ctypes.c_int(act))); a = a2
            rec["action"].append(act); rec["done"].append(done)
    assert all((e <= 1).all() for e in rec["enc"])
    flat, off = _ragged(rec["legal"])
    return {"generic/game": np.array(rec["game"], np.int16), "generic/legal": flat, "generic/legal_off": off,
            "generic/enc": np.stack(rec["enc"]), "generic/score": np.array(rec["score"], np.float32),
            "generic/check": np.array(rec["check"], np.int8), "generic/terminated": np.array(rec["terminated"], np.uint8),
            "generic/player": np.array(rec["player"], np.int16), "generic/step": np.array(rec["step"], np.int16),
            "generic/action": np.array(rec["action"], np.int16), "generic/done": np.array(rec["done"], np.uint8)}


def gen_lockstep(lib):
    lib.Init(1, 10, 60, 7.5)
    rng = np.random.RandomState(515)
    new = lambda: ctypes.create_string_buffer(2048)
    keys = ("game", "reset", "legal", "noeye", "enc", "score", "terr_score", "terr", "sub", "check", "player", "step", "terminated",
            "action", "inplace", "done")
    rec = {k: [] for k in keys}
    for g in range(12):
        st = new()
        reset = bool(lib.Reset(st))
        done = False; extra = 2; first = True
        while extra:
            la = (ctypes.c_int * (P + 1))(); n1 = lib.getLegalAction(st, la)
            ne = (ctypes.c_int * (P + 1))(); n2 = lib.getLegalNoEye(st, ne)
            enc = np.zeros(10 * P, np.float32); lib.Encode(st, enc.ctypes.data_as(ctypes.c_void_p))
            ter = np.zeros(P, np.float32); sc2 = lib.getTerritory(st, ter.ctypes.data_as(ctypes.c_void_p))
            sub = np.zeros(5 * 10 * 49, np.float32)
            lib.getSubEncode(enc.ctypes.data_as(ctypes.c_void_p), sub.ctypes.data_as(ctypes.c_void_p), 7, 10, 5)
            chk = [int(bool(lib.checkAction(st, ctypes.c_int(c)))) for c in LOCKSTEP_CHECKS]
            rec["game"].append(g); rec["reset"].append(reset if first else False); first = False
            rec["legal"].append(list(la[:n1])); rec["noeye"].append(list(ne[:n2])); rec["enc"].append(enc.astype(np.uint8))
            rec["score"].append(float(lib.getScore(st))); rec["terr_score"].append(float(sc2)); rec["terr"].append(ter.astype(np.int8))
            rec["sub"].append(sub.astype(np.uint8)); rec["check"].append(chk); rec["player"].append(lib.getPlayer(st) & 0xFF)
            rec["step"].append(lib.getStep(st)); rec["terminated"].append(bool(lib.isTerminated(st)))
            assert (enc <= 1).all() and (sub <= 1).all() and (ter == ter.astype(np.int8)).all()
            legal = [c for c in la[:n1] if c != P] or [P]
            r = rng.rand()
            act = P if r < 0.05 else int(rng.randint(P)) if r < 0.10 else int(legal[rng.randint(len(legal))])
            inplace = not rng.rand() < 0.5
            if not inplace:
                nx = new()
                d = bool(lib.Step(st, nx, ctypes.c_int(act)))
                st = nx
            else:
                d = bool(lib.Step_(st, ctypes.c_int(act)))
            rec["action"].append(act); rec["inplace"].append(inplace); rec["done"].append(d)
            if done:
                extra -= 1                                   # two more calls on a finished game
            done = done or d
    out = {}
    for k in ("legal", "noeye"):
        out[f"lockstep/{k}"], out[f"lockstep/{k}_off"] = _ragged(rec[k])
    for k, dt in (("game", np.int16), ("reset", np.uint8), ("enc", np.uint8), ("score", np.float32), ("terr_score", np.float32),
                  ("terr", np.int8), ("sub", np.uint8), ("check", np.uint8), ("player", np.int16), ("step", np.int16),
                  ("terminated", np.uint8), ("action", np.int16), ("inplace", np.uint8), ("done", np.uint8)):
        out[f"lockstep/{k}"] = np.array(rec[k], dt)
    return out


def main():
    lib = ctypes.CDLL(SO)
    lib.Init.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float]
    for f in ("Step", "Step_", "checkAction", "isTerminated", "Reset", "Encode"):
        getattr(lib, f).restype = ctypes.c_bool
    lib.getScore.restype = ctypes.c_float; lib.getTerritory.restype = ctypes.c_float
    out = gen_subenc(lib)
    out.update(gen_generic(lib))
    out.update(gen_lockstep(lib))
    path = os.path.join(HERE, "compiled_ref_s9.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out["generic/game"]), "generic plies,", len(out["lockstep/game"]), "lockstep calls")


if __name__ == "__main__":
    main()
