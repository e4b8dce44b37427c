#!/usr/bin/env python3
"""Forced playouts at the headline configuration: 9x9, 400 simulations, 6x128 tower, f32, 4096 boards staggered over the game
length (bench.py's set-up, shared by import).  One process, one JSON line over the timed steps: simulations per second with
forced_playouts_k = --k, the share of root selections (in forced moves) that met a forced child, and the mean number of visits
the pruning took per searched position.

    python scripts/time_forced_playouts.py --k 2 --steps 4 --warmup 1        (--k 0: the same loop with the feature off)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    a = ap.parse_args(argv)
    import numpy as np
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
    eng.set_forced_playouts(a.k)
    cut = {"visits": 0, "positions": 0}
    if a.k > 0:                                  # raw counts next to the pruned ones at every move selection: one more 1.3 MB read-out per ~3 s step
        choose = eng.choose_moves

        def spy(vis, steps, selfplay=True):
            raw = eng.root_visits()[0]
            live = ~eng.finished
            cut["visits"] += int((raw[live].astype(np.int64) - vis[live]).sum()); cut["positions"] += int(live.sum())
            return choose(vis, steps, selfplay)
        eng.choose_moves = spy
    for _ in range(a.warmup):
        sp.advance(device=True)
    torch.cuda.synchronize()
    cut["visits"] = cut["positions"] = 0
    st0, f0, m0, t0 = eng.stats(), eng.forced_playouts_stats(), sp.moves_played, time.perf_counter()
    for _ in range(a.steps):
        sp.advance(device=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st1, f1 = eng.stats(), eng.forced_playouts_stats()
    sel = f1["root_selections"] - f0["root_selections"]
    print(json.dumps({"k": a.k, "steps": a.steps, "wall_s": round(wall, 3), "sims_per_s": round((st1["sims"] - st0["sims"]) / wall, 1),
                      "moves_per_s": round((sp.moves_played - m0) / wall, 1), "root_selections": sel,
                      "forced_share": round((f1["forced_selections"] - f0["forced_selections"]) / sel, 4) if sel else None,
                      "pruned_visits_per_position": round(cut["visits"] / cut["positions"], 3) if cut["positions"] else None,
                      "errors": st1["errors"]}), flush=True)


if __name__ == "__main__":
    main()
