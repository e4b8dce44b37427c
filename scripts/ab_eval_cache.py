#!/usr/bin/env python3
"""A/B of the evaluation cache at the headline configuration: 9x9, 400 simulations, 6x128 tower, f32, 4096 boards staggered over
the game length (bench.py's set-up, shared by import).  The two arms -- cache off, cache on -- alternate in fresh child processes
on the same GPU; every child runs under its own time limit and the first non-zero status ends the run.  The report goes to
profiles/ab_eval_cache.txt (or --out):

    python scripts/ab_eval_cache.py --pairs 2 --steps 6 --warmup 2 --entries 4194304
    python scripts/ab_eval_cache.py --pairs 1 --network transgo          # the shipped MainNetwork's weights layout

A child (--arm off|on) prints one JSON line: sims/s over the timed steps, and for the cached arm the counters of the timed region
and the HIP-event times of the cache's stages next to the forward's (tg_prof_enable_eval_cache)."""
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
    ap.add_argument("--network", choices=["tower", "transgo"], default="tower")
    ap.add_argument("--entries", type=int, default=1 << 22, help="table size of the cached arm")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds one child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_eval_cache.txt"))
    return ap.parse_args(argv)


def child(a):
    import torch
    import bench
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    torch.cuda.set_device(0)
    cfg = Config(num_simulation=a.sims, num_features=a.filters, num_blocks=a.blocks, board_size=9, max_step=120,
                 network=a.network, eval_cache_entries=a.entries if a.arm == "on" else 0)
    arena = 2 * (4 * a.sims + 256) * (2 + 82) if a.network == "transgo" else 0          # as bench.py sizes it for that network
    sp = BatchedSelfPlay(cfg, a.games, device=0, arena_slots=arena)
    sp.set_weights(model.random_transgo_weights(9, 10, a.filters, seed=1234) if a.network == "transgo"
                   else model.random_weights(9, 10, a.filters, a.blocks, seed=1234))
    sp.start()
    bench.stagger(sp, cfg.max_step)
    eng = sp.engine
    for _ in range(a.warmup):
        sp.advance(device=True)
    if a.arm == "on":
        eng.ctx.call("tg_prof_enable_eval_cache", 1, 4096)
    torch.cuda.synchronize()
    st0, c0, t0 = eng.stats(), eng.eval_cache_stats(), time.perf_counter()
    prof = [0.0] * 4
    batches = 0
    for _ in range(a.steps):
        sp.advance(device=True)
        if a.arm == "on":                                  # drain the event pool (sized for one step) into the running totals
            v = [ctypes.c_double() for _ in range(4)]; n = ctypes.c_int64()
            eng.ctx.call("tg_prof_read_eval_cache", *[ctypes.byref(x) for x in v], ctypes.byref(n))
            prof, batches = [x.value for x in v], n.value
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st1, c1 = eng.stats(), eng.eval_cache_stats()
    line = {"arm": a.arm, "network": a.network, "steps": a.steps, "wall_s": round(wall, 3),
            "sims_per_s": round((st1["sims"] - st0["sims"]) / wall, 1), "rows_requested": st1["evals"] - st0["evals"]}
    if a.arm == "on":
        line["cache"] = {k: (c1[k] if k in ("entries", "bytes") else c1[k] - c0[k]) for k in c1}
        line["cache_since_creation"] = c1
        line["event_ms"] = dict(zip(("probe", "readback", "net", "insert"), [round(x, 3) for x in prof]))
        line["batches_timed"] = batches
    print(json.dumps(line), flush=True)


def run_child(a, arm):
    cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm] + [f"--{k}={getattr(a, k)}" for k in
           ("steps", "warmup", "games", "sims", "filters", "blocks", "network", "entries")]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit(f"arm {arm}: exit status {p.returncode}\n{p.stderr[-2000:]}")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def report(a, rows):
    net = f"MainNetwork (attention) x{a.filters}" if a.network == "transgo" else f"{a.blocks}x{a.filters} tower"
    out = [f"evaluation cache A/B: 9x9, {a.sims} simulations, {net} f32, {a.games} boards staggered over 120 plies,",
           f"{a.warmup} warm-up + {a.steps} timed steps per child, arms alternating in fresh processes; table {a.entries} entries", ""]
    out.append("pair  sims/s off   sims/s on    on/off")
    for i, (off, on) in enumerate(rows):
        out.append(f"{i:4d}  {off['sims_per_s']:11.1f}  {on['sims_per_s']:11.1f}  {on['sims_per_s'] / off['sims_per_s']:7.4f}")
    out.append("")
    for i, (_, on) in enumerate(rows):
        c, ev, n = on["cache"], on["event_ms"], max(on["batches_timed"], 1)
        out.append(f"pair {i}, cached arm, timed region: {n} batches (waves and root batches) timed")
        out.append(f"  rows requested {c['lookups']}, evaluated {c['evaluated']} ({c['evaluated'] / max(c['lookups'], 1):.4f} of requested)")
        out.append(f"  per batch: lookups {c['lookups'] / n:.1f}, hits {c['hits'] / n:.1f}, batch duplicates {c['batch_duplicates'] / n:.1f}")
        out.append(f"  inserts {c['inserts']}, dropped inserts {c['dropped_inserts']}")
        out.append(f"  per batch, HIP events: probe + duplicates + list {ev['probe'] / n:.4f} ms, read-back gap {ev['readback'] / n:.4f} ms, "
                   f"scatter + insert {ev['insert'] / n:.4f} ms, network {ev['net'] / n:.4f} ms")
        out.append(f"  table: {c['entries']} entries, {c['bytes']} bytes with staging")
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
    mode = "a" if a.network == "transgo" and os.path.exists(a.out) else "w"           # the transgo pair is appended to the tower's report
    with open(a.out, mode) as f:
        f.write(txt if mode == "w" else "\n" + txt)
    print(txt)


if __name__ == "__main__":
    main()
