"""Playout cap randomization (KataGo, arXiv:1902.10565 section 3.1): which moves of a self-play game are searched in full.

Every game draws, independently at every ply, whether the move is a *full* search (Config.num_simulation simulations, root
noise, recorded as a training position) or a *fast* one (Config.playout_cap_fast simulations, no root noise, not recorded).
The draw is a pure function of (game seed, ply, cap seed) -- a counter-based hash, the splitmix64 finaliser applied twice --
so it never touches the game's NumPy-legacy MT19937 stream, which is what keeps a game bit-identical to the reference's:

    mix(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;  x ^ x >> 31
    draw(seed, ply, cap_seed) = mix(mix(cap_seed << 32 | seed) ^ ply) >> 40          (24 bits)
    full(seed, ply)           = draw < floor(p_full * 2**24)

`tg_host_cap_draw` (csrc/rng_host.cpp) is the same function in C; tests/test_playout_cap_host.py holds the two together.
"""
import math

import numpy as np


def _mix(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draw(seeds, plies, cap_seed=0):
    """The 24-bit draw of every (seed, ply) pair: uint32 array, seeds and plies broadcast against each other."""
    seeds = np.asarray(seeds).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    plies = np.asarray(plies).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    key = (np.uint64(int(cap_seed) & 0xFFFFFFFF) << np.uint64(32)) | seeds
    return (_mix(_mix(key) ^ plies) >> np.uint64(40)).astype(np.uint32)


def threshold(p_full):
    return int(math.floor(float(p_full) * (1 << 24)))


def schedule(seeds, plies, p_full, cap_seed=0):
    """bool[G]: True where ply plies[g] of the game seeded seeds[g] is a full search.  p_full = 1.0: every move is."""
    return draw(seeds, plies, cap_seed) < np.uint32(threshold(p_full))         # a draw is below 2**24 = threshold(1.0)


def enabled(config):
    return float(getattr(config, "playout_cap_p_full", 1.0)) < 1.0


def check_config(config):
    """Refuses a playout-cap configuration that cannot be played; the message names the field."""
    p = getattr(config, "playout_cap_p_full", 1.0)
    if not (isinstance(p, (int, float)) and 0.0 < float(p) <= 1.0):
        raise ValueError(f"playout_cap_p_full must lie in (0, 1] (1.0 = playout cap off), got {p!r}")
    if float(p) < 1.0:
        n = getattr(config, "playout_cap_fast", 0)
        if not (isinstance(n, (int, np.integer)) and int(n) > 0):
            raise ValueError(f"playout_cap_fast must be a positive number of simulations when playout_cap_p_full < 1, got {n!r}")
