#!/usr/bin/env python3
"""Time of the tree read-out calls next to the existing root_info, after one full search (profiles/tree_readout_times.txt).

    python3 scripts/time_tree_readout.py [--games 4096] [--sims 400] [--reps 20] [--out FILE]

Each call is bracketed by two device events and by the host clock.  The calls are synchronous (they end by waiting for the
context's stream), so an event recorded on the otherwise idle default stream right before and right after a call brackets
everything the call did on the device: kernel, device -> host copies and the launch gaps between them.  The first call of each
kind is a warm-up (it loads the code object and, for the read-out, allocates the staging buffer) and is not counted.
Per-kernel times come from a separate run of this script under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transgo_amd import model                                     # noqa: E402
from transgo_amd.engine import SelfPlayEngine                     # noqa: E402


def timed(fn, reps):
    fn()                                                          # warm-up
    dev, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return np.array(dev), np.array(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    eng = SelfPlayEngine(a.games, num_simulation=a.sims, net_blocks=a.blocks, net_filters=a.filters)
    model.load_into(eng.ctx, model.random_weights(9, 10, a.filters, a.blocks), 9, 10, a.filters, a.blocks)
    eng.reset(np.arange(a.games))
    t0 = time.perf_counter()
    eng.search()
    search_s = time.perf_counter() - t0
    rc = eng.root_children()
    ln = eng.principal_variation(16)[3]
    A = eng.A
    calls = [("root_info(obs=False)", lambda: eng.root_info(obs=False), a.games * (4 * A + 12)),
             ("root_children()", eng.root_children, a.games * (25 * A + 17)),
             ("principal_variation(16)", lambda: eng.principal_variation(16), a.games * (12 * 16 + 4))]
    lines = [f"tree read-out, {a.games} games 9x9, after one {a.sims}-simulation search ({a.blocks}x{a.filters} f32 tower, random weights; "
             f"search {search_s:.2f} s), {a.reps} timed calls each after one warm-up",
             f"root visits per game {int(rc['root_n'].mean())}, status ok {int((rc['status'] == 0).sum())}, mean PV length {ln.mean():.2f} (max {int(ln.max())})",
             f"{'call':<26}{'device events ms: median':>26}{'min':>8}{'max':>8}{'host clock ms: median':>24}{'bytes to host':>16}"]
    for name, fn, nbytes in calls:
        dev, host = timed(fn, a.reps)
        lines.append(f"{name:<26}{np.median(dev):>26.3f}{dev.min():>8.3f}{dev.max():>8.3f}{np.median(host):>24.3f}{nbytes:>16}")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
