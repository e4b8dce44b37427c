#!/usr/bin/env python3
"""A/B of playout cap randomization at the headline configuration: 9x9, 400 simulations, 6x128 tower, f32, 4096 boards staggered
over the game length (bench.py's set-up, shared by import).  Arms -- cap off, then p_full = 0.25 with every --fast budget
(default 64 and 100) -- alternate in fresh child processes on the same GPU; every child runs under its own time limit and the first
non-zero status ends the run.  The report goes to profiles/ab_playout_cap.txt (or --out):

    python scripts/ab_playout_cap.py --rounds 2 --steps 6 --warmup 2

A child (--arm off | a fast budget) prints one JSON line over its timed steps: games and recorded positions per hour, simulations
per second, the mean rows per network launch, and the share of waves in which fewer than half of the boards were still searching
(fast games idle while the full ones of the same move finish: that is the cap's cost, and it is measured here, not guessed).  To
see the waves the child drives collect / evaluate / absorb itself (what tg_sp_search does inside the library) in every arm."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", help="(child) 'off' or the fast budget of a capped arm")
    ap.add_argument("--rounds", type=int, default=2, help="alternations over all arms")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--p-full", type=float, default=0.25)
    ap.add_argument("--fast", default="64,100", help="fast budgets of the capped arms")
    ap.add_argument("--cap-seed", type=int, default=0)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds one child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_playout_cap.txt"))
    return ap.parse_args(argv)


def watch_waves(eng, log):
    """tg_sp_search spelt out on the host, so that every wave's (boards still searching, rows evaluated) can be logged."""
    inner = eng.ctx.call

    def call(name, *args):
        if name != "tg_sp_search":
            return inner(name, *args)
        waves = 0
        while True:
            act, rows = ctypes.c_int32(), ctypes.c_int32()
            inner("tg_sp_collect", ctypes.byref(act), ctypes.byref(rows))
            if rows.value:
                inner("tg_sp_eval")
            inner("tg_sp_absorb")
            log.append((act.value, rows.value))
            if act.value == 0:
                break
            waves += 1
        args[0]._obj.value = waves
    eng.ctx.call = call


def child(a):
    import torch
    import bench
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    torch.cuda.set_device(0)
    capped = a.arm != "off"
    cfg = Config(num_simulation=a.sims, num_features=a.filters, num_blocks=a.blocks, board_size=9, max_step=120)
    if capped:
        cfg.playout_cap_p_full, cfg.playout_cap_fast, cfg.playout_cap_seed = a.p_full, 16, a.cap_seed
    sp = BatchedSelfPlay(cfg, a.games, device=0)
    sp.set_weights(model.random_weights(9, 10, a.filters, a.blocks, seed=1234))
    sp.start()
    bench.stagger(sp, cfg.max_step)          # cheap searches of both kinds (16 simulations); the records are marked by the schedule
    if capped:
        cfg.playout_cap_fast = int(a.arm)
    eng = sp.engine
    log = []
    watch_waves(eng, log)
    for _ in range(a.warmup):
        sp.advance(device=True)
    torch.cuda.synchronize()
    del log[:]
    st0, g0, m0, f0, t0 = eng.stats(), sp.games_finished, sp.moves_played, sp.full_moves, time.perf_counter()
    positions = 0
    for _ in range(a.steps):
        h = sp.advance(device=True)
        if h is not None:
            positions += h.n_positions
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st1 = eng.stats()
    launches = [r for _, r in log if r > 0]
    line = {"arm": a.arm, "p_full": a.p_full if capped else 1.0, "fast": int(a.arm) if capped else None, "steps": a.steps,
            "wall_s": round(wall, 3), "games_per_hour": round((sp.games_finished - g0) / wall * 3600, 1),
            "positions_per_hour": round(positions / wall * 3600, 1), "moves_per_s": round((sp.moves_played - m0) / wall, 1),
            "full_move_share": round((sp.full_moves - f0) / max(sp.moves_played - m0, 1), 4) if capped else 1.0,
            "sims_per_s": round((st1["sims"] - st0["sims"]) / wall, 1), "waves": len(log), "network_launches": len(launches),
            "rows_per_launch": round(sum(launches) / max(len(launches), 1), 1),
            "waves_under_half_active": round(sum(1 for act, _ in log if act < a.games / 2) / max(len(log), 1), 4),
            "errors": st1["errors"]}
    print(json.dumps(line), flush=True)


def run_child(a, arm):
    cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, f"--p-full={a.p_full}", f"--cap-seed={a.cap_seed}"] + \
          [f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "games", "sims", "filters", "blocks")]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit(f"arm {arm}: exit status {p.returncode}\n{p.stderr[-2000:]}")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def report(a, rows, arms):
    out = [f"playout cap randomization A/B: 9x9, {a.sims} simulations, {a.blocks}x{a.filters} tower f32, {a.games} boards staggered over 120 plies,",
           f"{a.warmup} warm-up + {a.steps} timed steps per child, arms alternating in fresh processes; capped arms: p_full = {a.p_full}, cap seed {a.cap_seed}.",
           "Every arm drives collect / evaluate / absorb from the host (one more host round trip per wave than tg_sp_search), so the",
           "columns compare the arms with each other, not with bench.py's line.  Games finishing inside the timed steps were staggered",
           "in with 16-simulation searches under the same schedule: positions/hour counts their unmarked plies.", ""]
    out.append("round  arm        games/h   positions/h     sims/s   moves/s  full share  rows/launch  waves  waves < half active")
    for i, r in enumerate(rows):
        for arm in arms:
            x = r[arm]
            name = "off" if arm == "off" else f"fast {arm}"
            out.append(f"{i:5d}  {name:9s} {x['games_per_hour']:9.1f} {x['positions_per_hour']:13.1f} {x['sims_per_s']:10.1f} {x['moves_per_s']:9.1f} "
                       f"{x['full_move_share']:11.4f} {x['rows_per_launch']:12.1f} {x['waves']:6d} {x['waves_under_half_active']:19.4f}")
    out.append("")
    for arm in arms[1:]:
        g = [r[arm]["games_per_hour"] / r["off"]["games_per_hour"] for r in rows if r["off"]["games_per_hour"] > 0]
        p = [r[arm]["positions_per_hour"] / r["off"]["positions_per_hour"] for r in rows if r["off"]["positions_per_hour"] > 0]
        m = [r[arm]["moves_per_s"] / r["off"]["moves_per_s"] for r in rows]
        out.append(f"fast {arm} / off, per round: moves/s " + " ".join(f"{v:.3f}" for v in m) + "; games/h " + " ".join(f"{v:.3f}" for v in g) +
                   "; positions/h " + " ".join(f"{v:.3f}" for v in p))
    return "\n".join(out) + "\n"


def main(argv=None):
    a = parse_args(argv)
    if a.arm:
        return child(a)
    arms = ["off"] + [s.strip() for s in a.fast.split(",") if s.strip()]
    rows = []
    for _ in range(a.rounds):
        r = {}
        for arm in arms:
            r[arm] = run_child(a, arm)
            print(json.dumps(r[arm]), flush=True)
        rows.append(r)
    txt = report(a, rows, arms)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
