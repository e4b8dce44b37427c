"""Gumbel root search ("Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022): the definition the device
code is held to.

At small budgets (n simulations over ~80 or ~360 root children) visit counts are a poor policy target.  The Gumbel rule samples
m root actions without replacement (Gumbel-top-k), spends the budget on them by sequential halving, plays the winner, and trains
the policy towards softmax(logits + sigma(q)) -- an improvement over the prior at any n.  Three parameters (Config.gumbel_m,
gumbel_c_visit, gumbel_c_scale): m = the number of considered actions (0 = off), sigma(q) = (c_visit + max_b N(b)) * c_scale * q.

A move that would begin with root noise is a *Gumbel move* while m > 0: it gets no Dirichlet noise.  At its start one
random_sample() u per root child (ascending action, pass last) is taken from the game's stream, g = -log(-log(u)),
gl = g + log(prior); the m_eff = min(m, nchild) children with the largest gl (ties: the lower action) are *considered*, every other
child's gl is -inf.  n0[c] = c.n and N0 = root.n are the base counts; with wu the WU-UCT loss (a path in flight adds exactly wu
to `pending` of every node it passes),

    e(c) = (c.n - n0[c]) + c.pending / wu          the search effort on c in this move, read-outs in flight included
    t    = (root.n - N0) + root.pending / wu

Root selection: the eligible children are the considered ones with e(c) == v(t), v = considered_visit(m_eff, budget, t), the
sequential-halving table in closed form; if there are none (a wave overshot the budget, a simulation was dropped) the considered
ones with the smallest e(c).  score(c) = gl[c] + (c_visit + maxN) * c_scale * qhat(c), maxN = the largest c.n over all root
children, qhat(c) = -(c.w / (c.n + 1)) in w's kind; the maximum over the eligible children, the tie list in ascending action order
and the one rng.choice over it are the plain search's.  Below the root nothing changes.

The move, when the search is over: argmax score over the considered children with the largest e(c), ties to the lower action; no
draw.  The policy target: softmax over all root children of log(prior) + (c_visit + maxN) * c_scale * qhat, stored in the record
as round_half_up(pi' * 2**24).

Every function keeps the scalar kinds of the oracle (SURVEY.md note N): n, pending are Python ints, a root child's prior and w are
float32, everything named float64 here is a Python float.  math.log / math.exp (libm), never the vectorised NumPy ones.
"""
import math

import numpy as np

FIXED_ONE = 1 << 24
NEG_INF = float("-inf")


def check_params(m, c_visit=50.0, c_scale=1.0):
    """Refuses parameters the engine would refuse; the message names the Config field."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) < 0:
        raise ValueError(f"gumbel_m must be an integer >= 0 (0 = Gumbel root search off), got {m!r}")
    for name, c in (("gumbel_c_visit", c_visit), ("gumbel_c_scale", c_scale)):
        if isinstance(c, bool) or not isinstance(c, (int, float, np.integer, np.floating)) or not math.isfinite(float(c)):
            raise ValueError(f"{name} must be a finite number, got {c!r}")
    return int(m), float(c_visit), float(c_scale)


def draw(rng, n):
    """n Gumbel(0, 1) variates from a RandomState: one random_sample() each, g = -log(-log(u)); u == 0 gives -inf."""
    out = []
    for _ in range(n):
        u = float(rng.random_sample())
        out.append(NEG_INF if u == 0.0 else -math.log(-math.log(u)))
    return out


def log_prior(prior):
    p = float(prior)
    return math.log(p) if p > 0.0 else NEG_INF


def table(g, priors, m):
    """gl per root child (ascending action order): g + log(prior) for the min(m, nchild) largest (ties: the lower action), -inf
    for every other child."""
    gl = [gi + log_prior(p) for gi, p in zip(g, priors)]
    m_eff = min(int(m), len(gl))
    keep = sorted(range(len(gl)), key=lambda i: (-gl[i], i))[:m_eff]
    out = [NEG_INF] * len(gl)
    for i in keep:
        out[i] = gl[i]
    return out


def considered_visit(m_eff, n, t):
    """v(t): the considered-visit value of step min(t, n - 1) of the sequential-halving schedule for m_eff considered actions and a
    budget of n simulations, in closed form with integers only (the table of the paper's public implementation, restated)."""
    m_eff, n, t = int(m_eff), int(n), int(t)
    if m_eff <= 1:
        return t
    s = max(0, min(t, n - 1))
    L = max(1, (m_eff - 1).bit_length())           # ceil(log2(m_eff))
    k, base = m_eff, 0
    while True:
        x = max(1, n // (L * k))
        if s < x * k:
            return base + s // k
        s -= x * k
        base += x
        k = max(2, k // 2)


def effort(n, n0, pending, wu):
    return (int(n) - int(n0)) + (int(pending) // int(wu) if int(wu) > 0 else 0)


def qhat(w, n):
    """The child's value seen from the root, as a float64: -(w / (n + 1)) computed in w's kind."""
    return float(-(w / (int(n) + 1)))


def score(gl, c_visit, c_scale, max_n, q):
    return gl + (c_visit + int(max_n)) * c_scale * q


def select(gl, kids, n0, root_n, root_pending, base_n, wu, m, budget, c_visit, c_scale):
    """One root selection.  kids: (n, pending, w) per root child in ascending action order.  Returns (scores, eligible, fallback):
    eligible = the indices the maximum is taken over, scores[i] their scores (None elsewhere)."""
    t = effort(root_n, base_n, root_pending, wu)
    v = considered_visit(min(int(m), len(kids)), budget, t)
    cons = [i for i in range(len(kids)) if gl[i] > NEG_INF]
    e = [effort(k[0], n0[i], k[1], wu) for i, k in enumerate(kids)]
    elig = [i for i in cons if e[i] == v]
    fallback = not elig
    if fallback and cons:
        lo = min(e[i] for i in cons)
        elig = [i for i in cons if e[i] == lo]
    max_n = max((int(k[0]) for k in kids), default=0)
    scores = [None] * len(kids)
    for i in elig:
        scores[i] = score(gl[i], c_visit, c_scale, max_n, qhat(kids[i][2], kids[i][0]))
    return scores, elig, fallback


def pick_move(gl, kids, n0, c_visit, c_scale):
    """The move of a search that is over.  kids: (n, w) per root child; the index of the chosen child, -1 without a considered one."""
    cons = [i for i in range(len(kids)) if gl[i] > NEG_INF]
    if not cons:
        return -1
    top = max(int(kids[i][0]) - int(n0[i]) for i in cons)
    max_n = max(int(k[0]) for k in kids)
    best, best_s = -1, None
    for i in cons:
        if int(kids[i][0]) - int(n0[i]) != top:
            continue
        s = score(gl[i], c_visit, c_scale, max_n, qhat(kids[i][1], kids[i][0]))
        if best < 0 or s > best_s:
            best, best_s = i, s
    return best


def improved_policy_row(kids, c_visit, c_scale):
    """pi' over the root children.  kids: (prior, n, w) in ascending action order; a list of float64."""
    if not kids:
        return []
    max_n = max(int(k[1]) for k in kids)
    logits = [log_prior(p) + (c_visit + max_n) * c_scale * qhat(w, n) for p, n, w in kids]
    mx = max(logits)
    if mx == NEG_INF:
        return [1.0 / len(kids)] * len(kids)
    ex = [math.exp(l - mx) for l in logits]
    tot = 0.0
    for x in ex:
        tot += x
    return [x / tot for x in ex]


def improved_policy(tables, c_visit=50.0, c_scale=1.0, games=None):
    """improved_policy_row over the dense [G, A] arrays of SelfPlayEngine.root_children(): pi' as float64 [G, A] (0 for an action
    that is not legal at the root).  games bool[G]: only these rows are computed (default: all); the others are 0."""
    n = np.asarray(tables["n"])
    out = np.zeros(n.shape, np.float64)
    for g in range(n.shape[0]):
        if games is not None and not games[g]:
            continue
        acts = np.flatnonzero(np.asarray(tables["flags"])[g] & 1)
        kids = [(tables["prior"][g, a], int(n[g, a]), tables["w"][g, a]) for a in acts]
        out[g, acts] = improved_policy_row(kids, float(c_visit), float(c_scale))
    return out


def fixed_point(pi):
    """round_half_up(pi * 2**24) as int32: what the integer record keeps of a float64 policy."""
    return np.floor(np.asarray(pi, np.float64) * FIXED_ONE + 0.5).astype(np.int32)
