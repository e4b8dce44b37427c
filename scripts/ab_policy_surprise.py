#!/usr/bin/env python3
"""A/B of policy surprise weighting at the headline configuration: 9x9, 400 simulations, 6x128 tower, f32, 4096 boards staggered over
the game length (bench.py's set-up, shared by import).  The two arms -- weight 0, weight 0.5 -- alternate in fresh child processes on
the same GPU; every child runs under its own time limit and the first non-zero status ends the run.  The report goes to
profiles/ab_policy_surprise.txt (or --out):

    python scripts/ab_policy_surprise.py --pairs 3 --steps 6 --warmup 2

A child (--arm off|on) prints one JSON line: sims/s over the timed steps, the positions harvested, and for the weighted arm the
HIP-event times of the three stages (prior forward, k_psw_surprise + k_psw_plan, k_psw_gather) with the positions in and out."""
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
    ap.add_argument("--pairs", type=int, default=3, help="alternations off / on")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--weight", type=float, default=0.5, help="policy_surprise_weight of the weighted arm")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds one child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_policy_surprise.txt"))
    return ap.parse_args(argv)


def child(a):
    import torch
    import bench
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    torch.cuda.set_device(0)
    cfg = Config(num_simulation=a.sims, num_features=a.filters, num_blocks=a.blocks, board_size=9, max_step=120,
                 policy_surprise_weight=a.weight if a.arm == "on" else 0.0, policy_surprise_seed=1)
    sp = BatchedSelfPlay(cfg, a.games, device=0)
    sp.set_weights(model.random_weights(9, 10, a.filters, a.blocks, seed=1234))
    sp.start()
    bench.stagger(sp, cfg.max_step)
    eng = sp.engine
    for _ in range(a.warmup):
        sp.advance(device=True)
    torch.cuda.synchronize()
    st0, p0, t0 = eng.stats(), eng.policy_surprise_stats(), time.perf_counter()
    harvests = positions = 0
    for _ in range(a.steps):
        h = sp.advance(device=True)
        if h is not None:
            harvests += 1; positions += h.n_positions
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st1, p1 = eng.stats(), eng.policy_surprise_stats()
    line = {"arm": a.arm, "steps": a.steps, "wall_s": round(wall, 3), "sims_per_s": round((st1["sims"] - st0["sims"]) / wall, 1),
            "harvests": harvests, "positions_harvested": positions, "game_end_s": round(sp.phase_s.get("game_end", 0.0), 4)}
    if a.arm == "on":
        line["policy_surprise"] = {k: p1[k] - p0[k] for k in p1}
    print(json.dumps(line), flush=True)


def run_child(a, arm):
    cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm] + [f"--{k}={getattr(a, k)}" for k in
           ("steps", "warmup", "games", "sims", "filters", "blocks", "weight")]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit(f"arm {arm}: exit status {p.returncode}\n{p.stderr[-2000:]}")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def report(a, rows):
    out = [f"policy surprise weighting A/B: 9x9, {a.sims} simulations, {a.blocks}x{a.filters} tower f32, {a.games} boards staggered over 120 plies,",
           f"{a.warmup} warm-up + {a.steps} timed steps per child, arms alternating in fresh processes; weight {a.weight} against 0", ""]
    out.append("pair  sims/s off   sims/s on    on/off")
    for i, (off, on) in enumerate(rows):
        out.append(f"{i:4d}  {off['sims_per_s']:11.1f}  {on['sims_per_s']:11.1f}  {on['sims_per_s'] / off['sims_per_s']:7.4f}")
    offs = [off["sims_per_s"] for off, _ in rows]
    ons = [on["sims_per_s"] for _, on in rows]
    mean = lambda v: sum(v) / len(v)
    out.append("")
    out.append(f"off arm: mean {mean(offs):.1f}, scatter (max - min) / mean {(max(offs) - min(offs)) / mean(offs):.4f}")
    out.append(f"on arm:  mean {mean(ons):.1f}, on / off of the means {mean(ons) / mean(offs):.4f}")
    out.append("")
    for i, (off, on) in enumerate(rows):
        p, n = on["policy_surprise"], max(on["policy_surprise"]["plans"], 1)
        out.append(f"pair {i}, weighted arm, timed region: {p['plans']} harvests planned, {p['games']} games")
        out.append(f"  positions in {p['positions_in']}, out {p['positions_out']} (out / in {p['positions_out'] / max(p['positions_in'], 1):.4f}); "
                   f"rows forwarded for the prior {p['rows_forwarded']}; plain arm harvested {off['positions_harvested']} positions")
        out.append(f"  per harvest, HIP events: prior forward {p['prior_ms'] / n:.4f} ms, surprise + plan {p['plan_ms'] / n:.4f} ms, "
                   f"gather {p['gather_ms'] / n:.4f} ms (plan + gather {(p['plan_ms'] + p['gather_ms']) / n:.4f} ms)")
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
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
