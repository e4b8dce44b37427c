"""Policy surprise weighting (KataGo, arXiv:1902.10565 appendix; its `policySurpriseDataWeight`): how often a recorded position of
a finished game is written to the training data.

Half of a game's weight (lambda = 0.5 in KataGo) is spread evenly over its recorded positions, the other half in proportion to
how much the search changed the network's mind there, KL(search target || raw network policy); a position of weight w is then
written floor(w) or floor(w) + 1 times.  Everything is float64 unless said otherwise.  For a harvested position with counts row c
(int32[A] as recorded: under forced playouts the pruned counts, under Gumbel the fixed-point improved policy) and the network's
float32 policy row p for that position (softmax over all A actions, NOT renormalised over the legal ones):

    c' = c with 1 -> 0,  n = sum(c')                                      (the rule of records.Harvest.pis)
    s  = 0                                                    if n == 0
       = max(0, sum over a with c'_a > 0 of pi_a * (log pi_a - log max(p_a, FLT_MIN))),  pi_a = c'_a / n

and for a game with T harvested positions t = 0..T-1 in recorded order (plies the playout cap kept out of the record are already
compacted away and do not count), S = s_0 + s_1 + ... taken sequentially:

    w_t = (1 - lambda) + lambda * T * s_t / S      if S > 0, else 1
    u_t = draw(game seed, t, seed ^ 0x50535731) / 2**24                   (playout_cap.draw: no game's MT19937 stream is touched)
    k_t = floor(w_t + u_t)                                                copies of position t, possibly 0

The output is a harvest batch in which position t stands k_t times in a row; games and plies keep their order, n_moves[g] = sum of
the game's k_t, the per-game tables do not change, and the expected size of the batch is the size of the input.

The engine does all of this on the device before a batch leaves `SelfPlayEngine.harvest` (csrc/policy_surprise.hip,
tg_sp_policy_surprise*); this module is the definition the kernels are tested against, and the host path for nothing else.

Interplay with the other self-play modes, in one place:
  * playout cap randomization -- only recorded positions (full searches) exist in a harvest, so only they are weighted, and t
    indexes them, not the game's plies: a fast ply neither takes weight nor shifts the draw of the positions behind it;
  * forced playouts, Gumbel root search -- the recorded target is used as it stands (pruned counts, fixed-point improved policy);
  * checkpoints -- the feature adds no engine state: a plan is computed from the finished games and dropped with them, so games
    that were finished but not harvested when a snapshot was taken resample identically after a restore.
"""
import numpy as np

from . import playout_cap

DOMAIN = 0x50535731                                    # "PSW1": keeps these draws apart from the playout cap's under the same seed
FLT_MIN = float(np.finfo(np.float32).tiny)             # 2**-126: the floor of a prior entry


def check_config(config):
    """Refuses a configuration whose policy surprise fields cannot be used; the message names the field."""
    w = getattr(config, "policy_surprise_weight", 0.0)
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not (0.0 <= float(w) <= 1.0):
        raise ValueError(f"policy_surprise_weight must lie in [0, 1] (0.0 = off, KataGo uses 0.5), got {w!r}")
    s = getattr(config, "policy_surprise_seed", 0)
    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not (0 <= int(s) < 2 ** 32):
        raise ValueError(f"policy_surprise_seed must be an integer in [0, 2**32), got {s!r}")
    return float(w), int(s)


def enabled(config):
    return float(getattr(config, "policy_surprise_weight", 0.0)) > 0.0


def surprise_terms(counts_row, prior_row):
    """The terms pi_a * (log pi_a - log p_a) of one position over the actions with c'_a > 0 (empty when n == 0)."""
    c = np.asarray(counts_row).astype(np.int64)
    c = np.where(c == 1, 0, c)
    n = int(c.sum())
    if n == 0:
        return np.zeros(0, np.float64)
    keep = c > 0
    pi = c[keep] / float(n)
    p = np.maximum(np.asarray(prior_row, np.float32).astype(np.float64)[keep], FLT_MIN)
    return pi * (np.log(pi) - np.log(p))


def surprise(counts, prior):
    """s f64[n] of every position: counts int[n][A], prior f32[n][A]."""
    counts = np.asarray(counts); prior = np.asarray(prior, np.float32)
    out = np.zeros(len(counts), np.float64)
    for t in range(len(counts)):
        terms = surprise_terms(counts[t], prior[t])
        out[t] = max(0.0, float(np.sum(terms))) if len(terms) else 0.0
    return out


def weights(s, lam):
    """w f64[T] of one game from its surprises, in recorded order."""
    s = np.asarray(s, np.float64)
    T = len(s)
    tot = 0.0
    for x in s:                                        # sequentially over t
        tot = tot + float(x)
    if not tot > 0.0:
        return np.ones(T, np.float64)
    lam = float(lam)
    return np.array([(1.0 - lam) + lam * T * float(x) / tot for x in s], np.float64)


def uniforms(game_seed, T, seed=0):
    """u f64[T] of one game: the 24-bit counter hash of (game seed, t, seed ^ DOMAIN) over 2**24."""
    d = playout_cap.draw(int(game_seed), np.arange(T), (int(seed) ^ DOMAIN) & 0xFFFFFFFF)
    return np.asarray(d, np.float64).reshape(T) / float(1 << 24)


def plan(counts, prior, n_moves, game_seeds, lam, seed=0):
    """The whole rule for a batch of games laid out as in a harvest (positions game after game): dict of surprise, weight, u
    (f64[n]), copies (int32[n]), n_moves (int32[g], the resampled lengths), src (int32[n_out], the source row of every output row)
    and n_out."""
    n_moves = np.asarray(n_moves, np.int64)
    n = int(n_moves.sum())
    s = surprise(np.asarray(counts)[:n], np.asarray(prior, np.float32)[:n])
    w = np.ones(n, np.float64); u = np.zeros(n, np.float64)
    o = 0
    for g, T in enumerate(n_moves):
        T = int(T)
        w[o:o + T] = weights(s[o:o + T], lam)
        u[o:o + T] = uniforms(game_seeds[g], T, seed)
        o += T
    copies = np.floor(w + u).astype(np.int32)
    out_moves = np.array([int(copies[a:b].sum()) for a, b in zip(np.cumsum(n_moves) - n_moves, np.cumsum(n_moves))], np.int32)
    src = np.repeat(np.arange(n, dtype=np.int32), copies)
    return dict(surprise=s, weight=w, u=u, copies=copies, n_moves=out_moves, src=src, n_out=int(copies.sum()))


def resample(harvest, prior, lam, seed=0):
    """records.Harvest (host) -> the resampled host Harvest: every position section gathered through plan()'s src, n_moves
    replaced, every other per-game table as it was.  The game seeds are the batch's own `seed` table."""
    from . import records
    h = harvest.to_host()
    p = plan(h.view("counts"), prior, h.view("n_moves"), h.view("seed"), lam, seed)
    sec, total = records.layout(h.S, h.C, h.n_games, p["n_out"])
    out = records.Harvest(h.S, h.C, h.n_games, p["n_out"], np.zeros(total, np.uint8))
    for k in ("winner", "slot", "seed", "score", "terr"):
        out.view(k)[...] = h.view(k)
    out.view("n_moves")[...] = p["n_moves"]
    for k in ("obs_bits", "counts", "z", "own", "player"):
        out.view(k)[...] = h.view(k)[p["src"]]
    return out, p
