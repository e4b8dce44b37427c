"""Test helper for policy surprise weighting: the synthetic fixtures of the kernel tests, the margin condition on them, and the
restatement (transgo_amd/policy_surprise.py, the definition) applied to a plain harvest.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from transgo_amd import policy_surprise as psw

MARGIN = 1e-9
GAME_LENGTHS = (0, 1, 40, 7, 0, 3, 12)               # T = 0, T = 1 and T = 40 among them; an empty game in the middle too
KERNEL_CASES = [(9, 0.5), (9, 1.0), (19, 0.5), (19, 1.0)]


@functools.lru_cache(maxsize=None)
def kernel_fixture(S, lam):
    """Synthetic games for the kernel tests at board size S: counts rows that hold 1s, a row whose counts are all <= 1 (n = 0), a
    game of nothing but such rows (sum of surprises 0), priors with exact zeros under visited moves (the FLT_MIN floor) and a few
    positions the prior knows nothing about, so that copies of 0 and of >= 2 both occur."""
    A = S * S + 1
    rs = np.random.RandomState(1000 * S + int(lam * 10))
    n_moves = np.array(GAME_LENGTHS, np.int32)
    n = int(n_moves.sum())
    counts = np.zeros((n, A), np.int32)
    prior = np.zeros((n, A), np.float32)
    for t in range(n):
        k = rs.randint(3, 12)
        acts = rs.choice(A, k, replace=False)
        counts[t, acts] = rs.randint(2, 60, k)
        ones = rs.choice(A, rs.randint(1, 6), replace=False)            # single visits: 1 -> 0
        counts[t, ones] = np.where(counts[t, ones] == 0, 1, counts[t, ones])
        logits = rs.randn(A) * 2.0
        if t % 5 == 0:                                                  # a prior that agrees with the search: little surprise
            logits = np.log(np.where(counts[t] > 1, counts[t], 0.01)) + rs.randn(A) * 0.05
        p = np.exp(logits - logits.max()); p /= p.sum()
        prior[t] = p.astype(np.float32)
    start = np.cumsum(n_moves) - n_moves
    g40 = int(start[2])
    prior[g40 + 5, np.argmax(counts[g40 + 5])] = 0.0                   # exact zeros under the most visited move: the floor
    prior[g40 + 17, counts[g40 + 17] > 1] = 0.0
    counts[g40 + 9] = 0; counts[g40 + 9, :4] = 1                        # all counts <= 1: n = 0
    g3 = int(start[5])
    counts[g3:g3 + 3] = 0; counts[g3:g3 + 3, 2] = 1                     # a whole game without a twice-visited move: w = 1
    seeds = (rs.randint(0, 2 ** 31, len(n_moves)).astype(np.uint32) * np.uint32(2)) + np.uint32(1)
    return dict(S=S, A=A, lam=float(lam), seed=7 + S, n_moves=n_moves, seeds=seeds, counts=counts, prior=prior)


def reference_plan(fx):
    return psw.plan(fx["counts"], fx["prior"], fx["n_moves"], fx["seeds"], fx["lam"], fx["seed"])


def abs_terms(counts, prior):
    """sum_a |term_a| of every position: the scale of the surprise bound."""
    return np.array([float(np.abs(psw.surprise_terms(c, p)).sum()) for c, p in zip(counts, prior)], np.float64)


def margin(plan):
    """The least distance of any w_t + u_t to an integer (inf for an empty plan)."""
    x = plan["weight"] + plan["u"]
    return float(np.min(np.abs(x - np.rint(x)))) if len(x) else float("inf")


def resample(plain, prior, lam, seed):
    """(the resampled host Harvest, the plan) of a plain harvest under the definition; the margin condition is asserted, since
    without it exact equality of the copies is not a fair demand on another f64 log."""
    out, plan = psw.resample(plain, prior, lam, seed)
    assert margin(plan) > MARGIN, margin(plan)
    return out, plan
