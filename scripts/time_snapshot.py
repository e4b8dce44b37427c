#!/usr/bin/env python3
"""What a snapshot costs at bench.py's headline shape (profiles/snapshot_headline.txt).

    python3 scripts/time_snapshot.py [--games 4096] [--sims 400] [--moves 20] [--reps 3] [--out FILE]

Plays `--moves` moves of a BatchedSelfPlay population with the f32 tower (random weights), then times tg_sp_snapshot to a host
buffer and to a device buffer and tg_sp_restore from both, with the host clock around the (synchronous) calls; the first call of
each kind is a warm-up that allocates the staging buffer and is not counted.  The yardstick printed next to them is one move of
the population, the mean over the last five moves of the same run.  A final move after the last restore checks that the restored
engine still plays."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transgo_amd import model, snapshot                           # noqa: E402
from transgo_amd.configure import Config                          # noqa: E402
from transgo_amd.self_play import BatchedSelfPlay                 # noqa: E402


def timed(fn, reps):
    fn()                                                          # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    cfg = Config(num_simulation=a.sims, num_features=a.filters, num_blocks=a.blocks)
    sp = BatchedSelfPlay(cfg, a.games)
    sp.set_weights(model.random_weights(9, 10, a.filters, a.blocks, seed=1234))
    move_s = []
    for m in range(a.moves):
        t0 = time.perf_counter()
        sp.advance(device=True)
        move_s.append(time.perf_counter() - t0)
        print(f"move {m + 1}: {move_s[-1]:.2f} s", flush=True)
    eng = sp.engine
    pool = eng.pool_stats()
    n = ctypes.c_uint64()
    eng.ctx.call("tg_sp_snapshot_size", ctypes.byref(n))
    host = np.empty(n.value, np.uint8)
    host[:] = 0                                                   # touch the pages: the timed copies should not pay for page faults
    dev = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    w = ctypes.c_uint64()
    vp = ctypes.c_void_p
    t_host = timed(lambda: eng.ctx.call("tg_sp_snapshot", vp(host.ctypes.data), n.value, 0, ctypes.byref(w)), a.reps)
    t_dev = timed(lambda: eng.ctx.call("tg_sp_snapshot", vp(dev.data_ptr()), n.value, 1, ctypes.byref(w)), a.reps)
    r_host = timed(lambda: eng.ctx.call("tg_sp_restore", vp(host.ctypes.data), n.value, 0), a.reps)
    r_dev = timed(lambda: eng.ctx.call("tg_sp_restore", vp(dev.data_ptr()), n.value, 1), a.reps)
    hdr = snapshot.parse_header(host)
    t0 = time.perf_counter()
    sp.advance(device=True)
    after = time.perf_counter() - t0
    one_move = float(np.mean(move_s[-5:]))
    fmt = lambda t: f"median {np.median(t):8.4f} s   min {t.min():8.4f}   max {t.max():8.4f}"
    lines = [
        f"snapshot cost, {a.games} boards 9x9, {a.sims} simulations, {a.blocks}x{a.filters} f32 tower (random weights), after {a.moves} moves; "
        f"{a.reps} timed calls each after one warm-up, host clock around the synchronous call; the host buffer is a pageable NumPy "
        f"array whose pages were touched beforehand; file writes and the replay store's save are not part of any figure",
        f"snapshot bytes              {n.value:>14}   ({n.value / 2 ** 20:.1f} MiB; tree section {hdr['sections']['tree'][1] / 2 ** 20:.1f} MiB in "
        f"{hdr['tree_chunks']} chunks, record {sum(hdr['sections'][k][1] for k in ('hist_obs', 'hist_cnt', 'hist_pl')) / 2 ** 20:.1f} MiB, "
        f"RNG {hdr['sections']['rng'][1] / 2 ** 20:.1f} MiB)",
        f"pool in use                 {pool['pool_in_use'] * 32:>14}   bytes of {pool['pool_slots'] * 32} provisioned "
        f"({100.0 * pool['pool_in_use'] / pool['pool_slots']:.1f} %; high water {100.0 * pool['pool_high_water'] / pool['pool_slots']:.1f} %)",
        f"tg_sp_snapshot to host      {fmt(t_host)}   ({n.value / np.median(t_host) / 1e9:.2f} GB/s)",
        f"tg_sp_snapshot to device    {fmt(t_dev)}   ({n.value / np.median(t_dev) / 1e9:.2f} GB/s)",
        f"tg_sp_restore from host     {fmt(r_host)}",
        f"tg_sp_restore from device   {fmt(r_dev)}",
        f"one move of the population  {one_move:8.4f} s   (mean of the last five moves of this run; the move after the last restore took {after:.4f} s)",
    ]
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
