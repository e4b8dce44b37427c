#!/usr/bin/env python3
"""Gumbel root search at the headline configuration: 9x9, 400 simulations, 6x128 tower, f32, 4096 boards staggered over the game
length (bench.py's set-up, shared by import).  One process, one JSON line over the timed steps: simulations per second with
gumbel_m = --m, the host time spent in begin_move (the draws and the top-m on the host, or the Dirichlet noise with --m 0), and
the share of root selections (in Gumbel moves) that fell back to the smallest effort.

    python scripts/time_gumbel.py --m 16 --steps 4 --warmup 1        (--m 0: the same loop with the feature off)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    a = ap.parse_args(argv)
    import torch
    import bench
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    torch.cuda.set_device(0)
    cfg = Config(num_simulation=a.sims, num_features=a.filters, num_blocks=a.blocks, board_size=9, max_step=120)
    sp = BatchedSelfPlay(cfg, a.games, device=0)
    sp.set_weights(model.random_weights(9, 10, a.filters, a.blocks, seed=1234))
    sp.start()
    bench.stagger(sp, cfg.max_step)              # cheap searches with the feature off
    eng = sp.engine
    eng.set_gumbel(a.m)
    for _ in range(a.warmup):
        sp.advance(device=True)
    torch.cuda.synchronize()
    st0, g0, m0, b0, sel0, t0 = eng.stats(), eng.gumbel_stats(), sp.moves_played, eng.begin_move_s, sp.phase_s.get("select", 0.0), time.perf_counter()
    for _ in range(a.steps):
        sp.advance(device=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st1, g1 = eng.stats(), eng.gumbel_stats()
    sel = g1["root_selections"] - g0["root_selections"]
    print(json.dumps({"m": a.m, "steps": a.steps, "wall_s": round(wall, 3), "sims_per_s": round((st1["sims"] - st0["sims"]) / wall, 1),
                      "moves_per_s": round((sp.moves_played - m0) / wall, 1),
                      "begin_move_ms_per_step": round((eng.begin_move_s - b0) / a.steps * 1e3, 2),
                      "select_ms_per_step": round((sp.phase_s.get("select", 0.0) - sel0) / a.steps * 1e3, 2),
                      "root_selections": sel,
                      "fallback_share": round((g1["fallback_selections"] - g0["fallback_selections"]) / sel, 4) if sel else None,
                      "errors": st1["errors"]}), flush=True)


if __name__ == "__main__":
    main()
