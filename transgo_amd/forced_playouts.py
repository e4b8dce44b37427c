"""Forced playouts and policy target pruning (KataGo, arXiv:1902.10565 section 3.2): the definition the device code is held to.

Root noise only helps if the noised moves get visited, so in a search whose move began with root noise every root child that
was visited at all is *forced* up to a number of visits proportional to the square root of its noised prior.  Visits that
were only forced are taken out again before the counts become the policy target: the target carries what the search found
out, not what it was made to look at.  One constant k (Config.forced_playouts_k; 0.0 = off, KataGo uses 2.0).

Forced selection, at the root only, in a search whose move began with root noise.  When a root child is picked, child c is
forced iff

    c.n >= 1   and   (c.n + c.pending) < sqrt(k * c.prior * (root.n + root.pending))            (float64)

with `prior` the noised prior as stored; a forced child's score is +inf.  Everything else of the selection stays: the maximum,
the tie list in ascending action order, one rng.choice over it (no draw when it has one entry).  `pending` (the WU-UCT
counters) is counted so that the read-outs of one wave do not pile onto one child.

Pruning, when the search is over (every pending counter is 0 again).  c* = the root child with the most visits (ties: the
lowest action), S* = score(root, c*).  For every other child c with c.n >= 1, f = floor(sqrt(k * c.prior * root.n)); visits
are taken from c.n one at a time, at most min(f, c.n) of them, each one only if the reduced count n' still has
score'(c, n') < S*, where score' is the score with n' + 1 as the denominator of its exploration term and the child's
q = w / (n + 1) and variance term at their final values.  c* and unvisited children keep their counts; the tree keeps n, w and
var as searched.  The reference's counts == 1 -> 0 step is applied on top by the caller, as ever.

Every function keeps the scalar kinds of the reference statement it restates (SURVEY.md note N), so that the oracle search
written with them (tests/forced_playouts_ref.py) and the kernels (csrc/engine.hip: collect_body<S, true>, pruned_counts)
agree bit for bit: `n`, `pending` are Python ints, a noised `prior` is a float64, `w` / `var` are float32 once a backup went
through the node.
"""
import numpy as np


def check_k(k):
    """Refuses a constant that is not a finite number >= 0; the message names the field."""
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not (0.0 <= float(k) < float("inf")):
        raise ValueError(f"forced_playouts_k must be a finite number >= 0 (0.0 = forced playouts off), got {k!r}")
    return float(k)


def score(c1, c2, prior, n, pending, w, var, parent_total, denom_n=None):
    """ucb_score of one child (self_play.py:716-725) as OracleSearch.score / puct_score compute it.  parent_total = parent.n +
    parent.pending.  denom_n: the visit count in the exploration term's denominator instead of n + pending (score')."""
    n = int(n)
    d = n + int(pending) if denom_n is None else int(denom_n)
    u = c1 * prior * np.sqrt(parent_total) / (d + 1)
    v = np.clip(var, 0, 3)
    s = c2 * np.sqrt(1 + v)
    return u + s + (-(w / (n + 1)))


def is_forced(k, prior, n, pending, root_total):
    """The forced rule for one root child; root_total = root.n + root.pending."""
    n, pending = int(n), int(pending)
    return n >= 1 and (n + pending) < np.sqrt(float(k) * prior * int(root_total))


def forced_budget(k, prior, root_n):
    """f: the most visits pruning may take from a child."""
    return int(np.floor(np.sqrt(float(k) * prior * int(root_n))))


def best_child(ns):
    """Index of c*: the most visits, the first (lowest action) on a tie; -1 for no children."""
    best = -1
    for i, n in enumerate(ns):
        if best < 0 or int(n) > int(ns[best]):
            best = i
    return best


def prune(k, c1, c2, children, root_n):
    """children: (prior, n, w, var) per root child in ascending action order, as searched; root_n = root.n.  Returns the pruned
    visit count of every child (a list of ints)."""
    ns = [int(c[1]) for c in children]
    out = list(ns)
    star = best_child(ns)
    if star < 0 or ns[star] < 1 or float(k) <= 0.0:
        return out
    p, n, w, var = children[star]
    s_star = score(c1, c2, p, n, 0, w, var, int(root_n))
    for i, (p, n, w, var) in enumerate(children):
        n = int(n)
        if i == star or n < 1:
            continue
        lim = min(forced_budget(k, p, root_n), n)
        m = n
        while n - m < lim and score(c1, c2, p, n, 0, w, var, int(root_n), denom_n=m - 1) < s_star:
            m -= 1
        out[i] = m
    return out


def prune_tables(k, c1, c2, tables, forced_games=None):
    """prune() over the dense [G, A] arrays of SelfPlayEngine.root_children() (a search that is over: pending all 0): the pruned
    visit counts as int32 [G, A].  forced_games bool[G]: only these games are pruned (default: all)."""
    n = np.asarray(tables["n"])
    out = n.astype(np.int32).copy()
    for g in range(n.shape[0]):
        if forced_games is not None and not forced_games[g]:
            continue
        acts = np.flatnonzero(np.asarray(tables["flags"])[g] & 1)
        kids = [(tables["prior"][g, a] if not (tables["flags"][g, a] & 4) else np.float32(tables["prior"][g, a]),
                 int(n[g, a]), tables["w"][g, a], tables["var"][g, a] if n[g, a] else 0.) for a in acts]
        out[g, acts] = prune(k, c1, c2, kids, int(tables["root_n"][g]))
    return out
