#!/usr/bin/env python3
"""A/B of the pass-alive end at the headline configuration: 9x9, 400 simulations, 6x128 tower, f32, 4096 boards
staggered over the game length (bench.py's set-up, shared by import).  The two arms -- mode off, mode on -- alternate in fresh child
processes on the same GPU; every child runs under its own time limit and the first non-zero status ends the run.  The report goes to
profiles/ab_pass_alive.txt (or --out; --append adds it to a file that already holds other lines):

    python scripts/ab_pass_alive.py --pairs 3 --steps 6 --warmup 2

A child (--arm off|on) prints one JSON line: simulations/s and games/hour over the timed steps, the mean plies of the games that
finished in them (every finished game, either arm), and (on) how many ended by settlement.  The boards are staggered at fixed offsets
and the timed window is a few moves, so which games finish inside it -- and their lengths -- is a sample of those offsets, not a
game-length distribution; a steady-state games/hour needs a run over several game lengths (--steps 300 or more).  --kernel times
tg_env_pass_alive for 4096 boards at 9x9 and 19x19 and the root read-out (k_root_pass_alive does the work of the launch behind
k_play) instead.

The weights are random: play is then near random and games rarely settle before the step limit, so the games/hour effect of a
trained network is NOT what this measures; the kernel times and the cost of the mode are."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["off", "on"], help="(child) run one arm and print its line")
    ap.add_argument("--kernel", action="store_true", help="(child) time the kernels and print one line")
    ap.add_argument("--pairs", type=int, default=3, help="alternations off / on")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds one child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_pass_alive.txt"))
    ap.add_argument("--append", action="store_true")
    return ap.parse_args(argv)


def child(a):
    import torch
    import bench
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    torch.cuda.set_device(0)
    cfg = Config(num_simulation=a.sims, num_features=a.filters, num_blocks=a.blocks, board_size=9, max_step=120,
                 pass_alive_end=a.arm == "on")
    sp = BatchedSelfPlay(cfg, a.games, device=0)
    sp.set_weights(model.random_weights(9, 10, a.filters, a.blocks, seed=1234))
    sp.start()
    bench.stagger(sp, cfg.max_step)
    eng = sp.engine
    assert eng.get_pass_alive_end() == (a.arm == "on")
    for _ in range(a.warmup):
        sp.advance(device=True)
    torch.cuda.synchronize()
    st0, pa0, t0 = eng.stats(), eng.pass_alive_stats(), time.perf_counter()
    g0, m0 = sp.games_finished, sp.moves_played
    fin = [0, 0]                                   # games and recorded plies of the games the timed steps finished (tg_sp_finished)
    harvest = eng.harvest

    def counted(*args, **kw):
        import ctypes
        ng, npos = ctypes.c_int32(), ctypes.c_int32()
        eng.ctx.call("tg_sp_finished", ctypes.byref(ng), ctypes.byref(npos))
        fin[0] += ng.value; fin[1] += npos.value
        return harvest(*args, **kw)
    eng.harvest = counted
    for _ in range(a.steps):
        sp.advance(device=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st1, pa1 = eng.stats(), eng.pass_alive_stats()
    games = sp.games_finished - g0
    line = {"arm": a.arm, "steps": a.steps, "wall_s": round(wall, 3), "sims_per_s": round((st1["sims"] - st0["sims"]) / wall, 1),
            "games_finished": int(games), "games_per_hour": round(3600.0 * games / wall, 1),
            "moves_played": int(sp.moves_played - m0), "plies_per_finished_game": round(fin[1] / max(fin[0], 1), 2),
            "games_settled": pa1["games_settled"] - pa0["games_settled"],
            "settled_plies_sum": pa1["plies_at_settlement_sum"] - pa0["plies_at_settlement_sum"], "errors": int(st1["errors"])}
    print(json.dumps(line), flush=True)


def kernel_child(a):
    import numpy as np
    import torch
    from transgo_amd.engine import SelfPlayEngine
    from transgo_amd.environment import GoEnv
    torch.cuda.set_device(0)
    line = {"kernel": True}
    for S in (9, 19):
        env = GoEnv(config=type("C", (), dict(board_size=S, max_step={9: 120, 19: 510}[S]))())
        n = 4096
        depth = (np.arange(n) % 8 + 1) * env.max_step // 8
        st = env.rollout_batch(env.reset_batch(n), seeds=np.arange(n), max_plies=depth)["states"]
        env.pass_alive_batch(st)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter(); r = env.pass_alive_batch(st); ts.append(time.perf_counter() - t0)
        line[f"env_pass_alive_4096_s{S}_ms"] = round(1e3 * min(ts), 3)          # copies in and out included (a host-array call)
        line[f"settled_s{S}"] = int(r["settled"].sum())
        if S == 9:
            from oracle import evaluators
            eng = SelfPlayEngine(n, board_size=9, num_simulation=8, evaluator=evaluators.flat, record_games=False)
            eng.reset(np.arange(n)); eng.reset_from(st)
            eng.root_pass_alive()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter(); eng.root_pass_alive(); ts.append(time.perf_counter() - t0)
            line["root_pass_alive_4096_s9_ms"] = round(1e3 * min(ts), 3)
            eng.close()
    print(json.dumps(line), flush=True)


def run_child(a, arm):
    cmd = [sys.executable, os.path.abspath(__file__)] + (["--kernel"] if arm == "kernel" else ["--arm", arm]) + \
          [f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "games", "sims", "filters", "blocks")]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit(f"arm {arm}: exit status {p.returncode}\n{p.stderr[-2000:]}")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def report(a, rows, kern):
    out = [f"pass-alive end A/B: 9x9, {a.sims} simulations, {a.blocks}x{a.filters} tower f32 (RANDOM weights), {a.games} boards staggered over "
           f"120 plies,", f"{a.warmup} warm-up + {a.steps} timed steps per child, arms alternating in fresh processes", ""]
    out.append("pair  sims/s off   sims/s on    on/off   games/h off  games/h on   plies/finished game off  on   settled share on")
    for i, (off, on) in enumerate(rows):
        out.append(f"{i:4d}  {off['sims_per_s']:11.1f}  {on['sims_per_s']:11.1f}  {on['sims_per_s'] / off['sims_per_s']:7.4f}  "
                   f"{off['games_per_hour']:11.1f}  {on['games_per_hour']:10.1f}   "
                   f"{off['plies_per_finished_game']:16.2f}  {on['plies_per_finished_game']:6.2f}   {on['games_settled'] / max(on['games_finished'], 1):8.4f}")
    out.append("")
    for off, on in rows:
        out.append(json.dumps(off)); out.append(json.dumps(on))
    out.append(json.dumps(kern))
    return "\n".join(out) + "\n"


def main(argv=None):
    a = parse_args(argv)
    if a.kernel:
        return kernel_child(a)
    if a.arm:
        return child(a)
    rows = []
    for _ in range(a.pairs):
        off = run_child(a, "off"); print(json.dumps(off), flush=True)
        on = run_child(a, "on"); print(json.dumps(on), flush=True)
        rows.append((off, on))
    kern = run_child(a, "kernel"); print(json.dumps(kern), flush=True)
    txt = report(a, rows, kern)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + txt)
    print(txt)


if __name__ == "__main__":
    main()
