#!/usr/bin/env python3
"""Full random no-eye games, 4096 boards at 9x9 and 1024 at 19x19, two ways on the same seeds:
  rollout   tg_env_rollout: the whole game in one kernel launch (GoEnv.rollout_batch)
  per-ply   what the engine offered before it: query_batch(noeye) + the host's choice (tg_host_mt_choice_index on the board's own
            stream) + step_batch, one round trip per ply
The two must end in the same states, plies and streams (asserted).  Wall time of the host call (it ends in a stream synchronise),
the rollout warmed up and repeated, alternating with nothing else; plies per second; and the kernel's VGPR / LDS / scratch figures
from the code object.  Needs an MI355X.
    python3 scripts/time_rollout.py [--out profiles/rollout_times.txt] [--boards9 4096] [--boards19 1024] [--reps 5]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from transgo_amd import _lib                                      # noqa: E402
from transgo_amd.configure import Config                          # noqa: E402
from transgo_amd.environment import GoEnv                         # noqa: E402


def per_ply(env, states, streams):
    """The parent's only way: one query + one step round trip per ply, the draw on the host."""
    lib = _lib.load()
    n, P = states.shape[0], env.P
    st = states.copy()
    rng = (_lib.TgMt19937 * n).from_buffer_copy(streams.tobytes())
    done = np.zeros(n, bool)
    plies = np.zeros(n, np.int32)
    while not done.all():
        mask = env.query_batch(st, noeye=True)["noeye"][:, :P]
        k = mask.sum(1)
        idx = np.zeros(n, np.int64)
        for g in np.flatnonzero(~done & (k > 1)):
            idx[g] = lib.tg_host_mt_choice_index(rng[int(g)], int(k[g]))
        act = np.where(k > 0, (np.cumsum(mask, axis=1) == (idx + 1)[:, None]).argmax(1), P)
        nxt, d, _ = env.step_batch(st, act)
        live = ~done
        st[live] = nxt[live]
        plies[live] += 1
        done |= d
    return st, plies, np.frombuffer(rng, np.uint8).reshape(n, -1).copy()


def measure(size, n, max_step, reps):
    env = GoEnv(Config(board_size=size, max_step=max_step))
    start = env.reset_batch(n)
    streams = env.seed_streams(np.arange(n))
    env.rollout_batch(start[:64], streams=streams[:64])          # code object load, scratch buffers
    r = env.rollout_batch(start, streams=streams)
    t_roll = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = env.rollout_batch(start, streams=streams)
        t_roll.append(time.perf_counter() - t0)
    env.query_batch(start, noeye=True); env.step_batch(start, np.zeros(n, np.int32))      # warm the per-ply kernels too
    t0 = time.perf_counter()
    st, plies, rng = per_ply(env, start, streams)
    t_loop = time.perf_counter() - t0
    assert (st == r["states"]).all() and (plies == r["plies"]).all() and (rng == r["streams"]).all(), "results differ"
    assert r["done"].all()
    total = int(plies.sum())
    tr = float(np.median(t_roll))
    return [f"{size}x{size}  boards {n}  max_step {max_step}  plies {total} (mean {total / n:.1f} per game, longest {int(plies.max())})",
            f"  tg_env_rollout   median {tr * 1e3:9.2f} ms  (min {min(t_roll) * 1e3:.2f}, max {max(t_roll) * 1e3:.2f}, {reps} runs)  "
            f"{total / tr / 1e6:8.2f} M plies/s",
            f"  per-ply loop     once   {t_loop * 1e3:9.2f} ms  {total / t_loop / 1e6:8.3f} M plies/s   ratio {t_loop / tr:.1f}x",
            "  results identical: states, plies, streams"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_times.txt"))
    ap.add_argument("--boards9", type=int, default=4096)
    ap.add_argument("--boards19", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lines = ["Random no-eye playouts to the end of the game: one launch (tg_env_rollout) against the per-ply loop (scripts/time_rollout.py)",
             "host wall time around calls that end in a stream synchronise; host <-> device copies of states and streams included", ""]
    lines += measure(9, a.boards9, 200, a.reps) + [""]
    lines += measure(19, a.boards19, 450, a.reps) + [""]
    try:
        import kernel_meta
        for k in kernel_meta.kernels(_lib.LIB_PATH):
            if "k_env_rollout" in k["name"] or "k_env_step" in k["name"]:
                nm = k["name"].split("(anonymous namespace)::")[-1].split("(")[0]
                lines.append(f"{nm:20s} vgpr {k['vgpr']:>4} sgpr {k['sgpr']:>4} lds {k['lds']:>6} B  scratch {k['scratch']:>4} B  "
                             f"vgpr spills {k['vspill']}  sgpr spills {k['sspill']}")
    except Exception as e:                                        # the timing stands without the code-object note
        lines.append(f"kernel metadata not read: {e}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
