#!/usr/bin/env python3
"""A/B of search ownership at the headline configuration: 9x9, 400 simulations, 6x128 tower, f32, 4096 boards
staggered over the game length (bench.py's set-up, shared by import).  The two arms -- mode off, mode on -- alternate in fresh child
processes on the same GPU; every child runs under its own time limit and the first non-zero status ends the run.  The report goes to
profiles/ab_search_ownership.txt (or --out; --append adds it to a file that already holds other lines):

    python scripts/ab_search_ownership.py --pairs 2 --steps 6 --warmup 2

A child (--arm off|on) prints one JSON line: simulations/s over the timed steps and the HIP-event time of the tree stage
(tg_prof_read_tree: collect_ms, absorb_ms, waves); the "on" arm also reads the ownership out once and reports the evaluations per
game the means of the last step rest on."""
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
    ap.add_argument("--arm", choices=["off", "on"], help="(child) run one arm and print its line")
    ap.add_argument("--pairs", type=int, default=2, help="alternations off / on")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--symmetry", choices=["none", "position"], default="none")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds one child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_search_ownership.txt"))
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
                 eval_symmetry=a.symmetry, search_ownership=a.arm == "on")
    sp = BatchedSelfPlay(cfg, a.games, device=0)
    sp.set_weights(model.random_weights(9, 10, a.filters, a.blocks, seed=1234))
    sp.start()
    bench.stagger(sp, cfg.max_step)
    eng = sp.engine
    assert eng.get_search_ownership() == (a.arm == "on")
    for _ in range(a.warmup):
        sp.advance(device=True)
    eng.ctx.call("tg_prof_enable_tree", 1, 8192)
    torch.cuda.synchronize()
    st0, t0 = eng.stats(), time.perf_counter()
    for _ in range(a.steps):
        sp.advance(device=True)
        eng.ctx.call("tg_prof_read_tree", None, None, None, None)      # drain the event pool (sized for one step) into the totals
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st1 = eng.stats()
    c, ab, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    eng.ctx.call("tg_prof_read_tree", ctypes.byref(c), ctypes.byref(ab), ctypes.byref(w), None)
    line = {"arm": a.arm, "symmetry": a.symmetry, "steps": a.steps, "wall_s": round(wall, 3),
            "sims_per_s": round((st1["sims"] - st0["sims"]) / wall, 1), "collect_ms": round(c.value, 3), "absorb_ms": round(ab.value, 3),
            "waves": int(w.value), "errors": int(st1["errors"])}
    if a.arm == "on":
        t1 = time.perf_counter()
        ro = eng.root_ownership()
        line["readout_ms"] = round(1e3 * (time.perf_counter() - t1), 3)
        line["evals_per_game_mean"] = round(float(ro["n"].mean()), 1)
    print(json.dumps(line), flush=True)


def run_child(a, arm):
    cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm] + [f"--{k}={getattr(a, k)}" for k in
           ("steps", "warmup", "games", "sims", "filters", "blocks", "symmetry")]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit(f"arm {arm}: exit status {p.returncode}\n{p.stderr[-2000:]}")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def report(a, rows):
    out = [f"search ownership A/B: 9x9, {a.sims} simulations, {a.blocks}x{a.filters} tower f32, eval_symmetry {a.symmetry}, {a.games} boards "
           f"staggered over 120 plies,", f"{a.warmup} warm-up + {a.steps} timed steps per child, arms alternating in fresh processes", ""]
    out.append("pair  sims/s off   sims/s on    on/off   collect ms/wave off  on      absorb ms/wave off  on")
    for i, (off, on) in enumerate(rows):
        wo, wn = max(off["waves"], 1), max(on["waves"], 1)
        out.append(f"{i:4d}  {off['sims_per_s']:11.1f}  {on['sims_per_s']:11.1f}  {on['sims_per_s'] / off['sims_per_s']:7.4f}   "
                   f"{off['collect_ms'] / wo:15.4f}  {on['collect_ms'] / wn:6.4f}   {off['absorb_ms'] / wo:14.4f}  {on['absorb_ms'] / wn:6.4f}")
    out.append("")
    for off, on in rows:
        out.append(json.dumps(off)); out.append(json.dumps(on))
    return "\n".join(out) + "\n"


def main(argv=None):
    a = parse_args(argv)
    if a.arm:
        return child(a)
    rows = []
    for _ in range(a.pairs):
        off = run_child(a, "off"); print(json.dumps(off), flush=True)
        on = run_child(a, "on"); print(json.dumps(on), flush=True)
        rows.append((off, on))
    txt = report(a, rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + txt)
    print(txt)


if __name__ == "__main__":
    main()
