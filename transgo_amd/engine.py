"""SelfPlayEngine -- host driver of the batched WP_MCTS engine in libtransgo_hip.so.

Mirrors, for G games at once, the per-game objects of the reference: `WP_MCTS.reset_root / get_action_probs /
update_with_action` (self_play.py:595-605, :657-687, :857-872).  Tree search, rules and the network run on the GPU;
this class only sequences the phases and does the one part the reference itself does in NumPy float64 on the host --
turning visit counts into pi and the sampled move (self_play.py:666-683) -- with the same NumPy calls, so those are
bit-identical by construction.  The random numbers for it come from the game's own MT19937 stream inside the library.
"""
import ctypes
import math
import time

import numpy as np

from . import _lib
from . import symmetry as _symmetry


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def temperature(game_step):
    """Config.epsilon_by_frame (configure.py:75-79)."""
    return 0.65 + (1.0 - 0.65) * math.exp(-1. * game_step / 10)


def choose_moves_reference(visits, steps, u, live, selfplay=True):
    """Literal per-game form of self_play.py:666-683 (the definition choose_moves_batch is tested against)."""
    G, A = visits.shape
    actions = np.zeros(G, np.int32)
    pis = np.zeros((G, A), np.float64)
    for g in np.flatnonzero(live):
        counts = np.array([int(c) for c in visits[g]])
        counts = np.where(counts == 1, 0, counts)
        pis[g] = counts / np.sum(counts)
        tau = temperature(int(steps[g])) if selfplay else 0.12
        powed = np.power(counts, 1.0 / tau)
        probs = np.array(powed) / np.sum(powed)
        cdf = probs.cumsum(); cdf /= cdf[-1]
        actions[g] = cdf.searchsorted(u[g], side="right")
    return actions, pis


def _choose_rows(counts_raw, steps, u, selfplay):
    """self_play.py:666-683 for a block of live rows (see choose_moves_batch)."""
    counts = counts_raw.astype(np.int64)
    counts = np.where(counts == 1, 0, counts)
    # No child visited twice (only possible when num_simulation is far below the number of legal moves): the reference
    # divides 0 by 0 here and np.random.choice raises on the NaN probabilities (self_play.py:671-683).  A batched engine
    # cannot afford one degenerate board stopping thousands, so such a row keeps its raw counts instead.
    dead = np.sum(counts, axis=1) == 0
    if dead.any():
        counts[dead] = counts_raw[dead]
    tot = np.sum(counts, axis=1)
    empty = tot == 0                                     # a slot that was never searched (parked / already over): pi = 0, action 0
    if empty.any():
        counts = counts.copy(); counts[empty, 0] = 1
        tot = np.sum(counts, axis=1)
    pis = counts / tot[:, None]
    if selfplay:
        inv_tau = 1.0 / (0.65 + (1.0 - 0.65) * np.array([math.exp(-1. * int(s) / 10) for s in steps]))     # configure.py:75-79, per game
    else:
        inv_tau = np.full(len(steps), 1.0 / 0.12)
    powed = np.power(counts, inv_tau[:, None])
    probs = powed / np.sum(powed, axis=1)[:, None]
    cdf = np.cumsum(probs, axis=1)
    cdf /= cdf[:, -1][:, None]
    acts = (cdf <= u[:, None]).sum(axis=1)                      # searchsorted(u, 'right') on a non-decreasing row
    if empty.any():
        acts[empty] = 0; pis[empty] = 0.0
    return acts, pis


_POOL = None


def choose_moves_batch(visits, steps, u, live, selfplay=True):
    """Every operation is element-wise or a last-axis reduction, so each row equals the per-game 1-D computation bit for bit;
    large batches are cut into row blocks handled by a few threads (NumPy releases the GIL inside its loops)."""
    global _POOL
    G, A = visits.shape
    actions = np.zeros(G, np.int32)
    pis = np.zeros((G, A), np.float64)
    idx = np.flatnonzero(live)
    if len(idx) == 0:
        return actions, pis
    nblk = min(8, len(idx) // 256)
    if nblk <= 1:
        actions[idx], pis[idx] = _choose_rows(visits[idx], steps[idx], u[idx], selfplay)
        return actions, pis
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=8)
    parts = np.array_split(idx, nblk)
    for part, (a, p) in zip(parts, _POOL.map(lambda ix: _choose_rows(visits[ix], steps[ix], u[ix], selfplay), parts)):
        actions[part] = a; pis[part] = p
    return actions, pis


def eval_cache_stats(engine):
    """The evaluation-cache counters of a SelfPlayEngine (or of anything that holds one as `.engine`) as a dict."""
    eng = getattr(engine, "engine", engine)
    ctx = getattr(eng, "ctx", None)
    if ctx is None or not getattr(ctx, "h", None):
        raise _lib.TransgoError("eval_cache_stats: no engine context (the engine was never created or is closed)")
    v = [ctypes.c_uint64() for _ in SelfPlayEngine.EVAL_CACHE_STATS]
    ctx.call("tg_sp_eval_cache_stats", *[ctypes.byref(x) for x in v])
    return {k: int(x.value) for k, x in zip(SelfPlayEngine.EVAL_CACHE_STATS, v)}


class SelfPlayEngine:
    def __init__(self, n_games, board_size=9, num_simulation=210, parallel_readouts=4, c_puct1=3, c_puct2=0.05,
                 wu_loss=2, komi=7.5, max_step=120, encode_dim=10, net_blocks=6, net_filters=128, arena_slots=0,
                 device=0, evaluator=None, net_precision="f32", record_games=True, pool_slots=0, eval_symmetry="none",
                 symmetry_seed=0, eval_cache_entries=0, forced_playouts_k=0.0, gumbel_m=0, gumbel_c_visit=50.0,
                 gumbel_c_scale=1.0, search_ownership=False, policy_surprise_weight=0.0, policy_surprise_seed=0,
                 pass_alive_end=False):
        cfg = _lib.default_config()
        cfg.record_games = 1 if record_games else 0       # per-move records in HBM for tg_sp_harvest (self-play); evaluation matches need none
        cfg.net_precision = {"f32": 0, "f16": 1, "f16r": 2, "f32x3": 3}[net_precision]
        cfg.board_size, cfg.encode_dim, cfg.max_step, cfg.komi = board_size, encode_dim, max_step, komi
        cfg.n_games, cfg.num_simulation, cfg.parallel_readouts, cfg.wu_loss = n_games, num_simulation, parallel_readouts, wu_loss
        cfg.c_puct1, cfg.c_puct2, cfg.arena_slots = c_puct1, c_puct2, arena_slots
        cfg.pool_slots = pool_slots                       # tree memory: slots per game ON AVERAGE in the pool all games share (0 = default)
        cfg.net_blocks, cfg.net_filters, cfg.device = net_blocks, net_filters, device
        self.ctx = _lib.Context(cfg)
        self.G, self.S, self.P, self.A, self.C = n_games, board_size, board_size ** 2, board_size ** 2 + 1, encode_dim
        self.num_simulation = num_simulation
        self.path_capacity = (max_step + 2 + 63) // 64 * 64      # SearchCfg::maxd: the deepest line principal_variation can return
        self.evaluator = evaluator           # None -> network on the GPU; callable(obs)->(policy, value) -> injected
                                             # (-> (policy, value, own) while search ownership is on)
        self.finished = np.zeros(n_games, bool)      # slots that take no part in the next search (game over, parked, in error)
        self.errored = np.zeros(n_games, bool)       # slots parked by a tree-arena overflow (restart them with reset(mask))
        self.device = device
        self.begin_move_s = 0.0                      # wall clock spent in tg_sp_begin_move (root noise on the host), for bench.py
        self._host_symmetry = (0, 0)
        if _symmetry.parse_mode(eval_symmetry, symmetry_seed)[0] != 0:
            self.set_symmetry(eval_symmetry, symmetry_seed)
        if eval_cache_entries:
            self.set_eval_cache(eval_cache_entries)
        self.forced_playouts_k = 0.0
        if forced_playouts_k:
            self.set_forced_playouts(forced_playouts_k)
        self.gumbel_m, self.gumbel_c_visit, self.gumbel_c_scale = 0, 50.0, 1.0
        if gumbel_m:
            self.set_gumbel(gumbel_m, gumbel_c_visit, gumbel_c_scale)
        self.search_ownership = False
        if search_ownership:
            self.set_search_ownership(True)
        self.policy_surprise_weight, self.policy_surprise_seed = 0.0, 0
        self.policy_surprise_ms = {}                 # HIP-event milliseconds of the last resampled harvest (prior, plan, gather)
        if policy_surprise_weight:
            self.set_policy_surprise(policy_surprise_weight, policy_surprise_seed)
        self.pass_alive_end = False
        if pass_alive_end:
            self.set_pass_alive_end(True)

    def close(self):
        self.ctx.close()

    def set_symmetry(self, mode, arg=0):
        """Symmetry-aware evaluation (transgo_amd.symmetry): "none" | "position" | "mean8" or an int s = 0..7; arg = the seed of
        "position".  With the network on the GPU this sets the context's mode (tg_net_set_symmetry); a host `evaluator` is
        wrapped with symmetry.evaluate_with_symmetry, so both kinds of engine mean the same thing.  Legal at a move boundary
        only (no evaluation batch pending)."""
        m, a = _symmetry.parse_mode(mode, arg)
        if self.evaluator is None:
            self.ctx.call("tg_net_set_symmetry", m, a)
        else:
            self._host_symmetry = (m, a)

    def get_symmetry(self):
        """(mode number 0..3, arg) in force: the context's (tg_net_get_symmetry), or the host evaluator's wrapper's."""
        if self.evaluator is not None:
            return self._host_symmetry
        m, a = ctypes.c_int(), ctypes.c_uint32()
        self.ctx.call("tg_net_get_symmetry", ctypes.byref(m), ctypes.byref(a))
        return int(m.value), int(a.value)

    # ---- evaluation cache (tg_sp_eval_cache) ------------------------------------------------------------------
    EVAL_CACHE_STATS = ("lookups", "hits", "batch_duplicates", "evaluated", "inserts", "dropped_inserts", "entries", "bytes")

    def set_eval_cache(self, entries):
        """An exact cache of network outputs keyed by the full bit-packed position: rows already evaluated under the live weights
        and symmetry mode, and rows that repeat inside one batch, skip the forward; results are bit-identical to the uncached
        engine.  `entries` is rounded up to whole 4-way buckets (452 B per entry at 9x9, 1920 B at 19x19); 0 frees the cache.
        Legal at a move boundary only.  A host `evaluator` is never cached (it is not known to be pure)."""
        self.ctx.call("tg_sp_eval_cache", int(entries))

    def clear_eval_cache(self):
        """Every entry written so far becomes a miss (a generation bump; weight loads and symmetry changes do it themselves)."""
        self.ctx.call("tg_sp_eval_cache_clear")

    def eval_cache_stats(self):
        """tg_sp_eval_cache_stats as a dict (EVAL_CACHE_STATS): cumulative since the cache was created, all 0 without one."""
        return eval_cache_stats(self)

    # ---- forced playouts and policy target pruning (tg_sp_forced_playouts) ------------------------------------
    def set_forced_playouts(self, k):
        """k > 0 (KataGo: 2.0): a search that begins with root noise forces every visited root child up to sqrt(k * prior * N)
        visits, and the counts that become the pi target and the move choice are pruned of the visits that were only forced
        (transgo_amd.forced_playouts holds the definition).  0.0 = off.  Context state: a restored snapshot does not carry it."""
        from . import forced_playouts as _fp
        k = _fp.check_k(k)
        self.ctx.call("tg_sp_forced_playouts", ctypes.c_double(k))
        self.forced_playouts_k = k

    def get_forced_playouts(self):
        k = ctypes.c_double()
        self.ctx.call("tg_sp_forced_playouts_get", ctypes.byref(k))
        return float(k.value)

    def forced_playouts_stats(self):
        """Root selections made in forced moves so far, and how many of them met a forced child."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx.call("tg_sp_forced_playouts_stats", ctypes.byref(a), ctypes.byref(b))
        return dict(root_selections=int(a.value), forced_selections=int(b.value))

    # ---- Gumbel root search (tg_sp_gumbel) --------------------------------------------------------------------
    def set_gumbel(self, m, c_visit=50.0, c_scale=1.0):
        """m > 0: a search that would begin with root noise is a Gumbel move instead -- no Dirichlet noise, m root actions sampled
        with the Gumbel-top-k trick, the budget spent on them by sequential halving (transgo_amd.gumbel holds the definition).
        0 = off.  Context state: a restored snapshot does not carry it.  Refused together with forced playouts."""
        from . import gumbel as _gb
        m, c_visit, c_scale = _gb.check_params(m, c_visit, c_scale)
        self.ctx.call("tg_sp_gumbel", m, ctypes.c_double(c_visit), ctypes.c_double(c_scale))
        self.gumbel_m, self.gumbel_c_visit, self.gumbel_c_scale = m, c_visit, c_scale

    def get_gumbel(self):
        m, cv, cs = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        self.ctx.call("tg_sp_gumbel_get", ctypes.byref(m), ctypes.byref(cv), ctypes.byref(cs))
        return int(m.value), float(cv.value), float(cs.value)

    def gumbel_moves(self):
        """(actions int32[G], gumbel_game bool[G]): the deterministic move of every game inside a Gumbel move whose search is over
        (-1 / False for every other game)."""
        act = np.full(self.G, -1, np.int32); gg = np.zeros(self.G, np.uint8)
        self.ctx.call("tg_sp_gumbel_move", _ptr(act), _ptr(gg))
        return act, gg != 0

    def gumbel_table(self):
        """The gl table of the Gumbel moves in progress as the engine uses it, by action: float64 [G, A], -inf for a child that is
        not considered and for an action that is not legal; rows of games that are not in a Gumbel move are all -inf."""
        raw = np.zeros((self.G, self.A), np.float64)
        self.ctx.call("tg_sp_gumbel_table", _ptr(raw))
        legal = (self.root_children()["flags"] & self.CHILD_PRESENT) != 0
        gg = self.gumbel_moves()[1]
        out = np.full((self.G, self.A), -np.inf)
        for g in np.flatnonzero(gg):
            acts = np.flatnonzero(legal[g])
            out[g, acts] = raw[g, :len(acts)]
        return out

    def gumbel_targets(self, games=None):
        """(pi' float64 [G, A], counts int32 [G, A]) of the games in a Gumbel move (default: gumbel_moves()'s): the improved policy
        (gumbel.improved_policy over root_children()) and its fixed-point form, 0 for the other games."""
        from . import gumbel as _gb
        if games is None:
            games = self.gumbel_moves()[1]
        pi = _gb.improved_policy(self.root_children(), self.gumbel_c_visit, self.gumbel_c_scale, games)
        return pi, _gb.fixed_point(pi)

    def stage_gumbel_targets(self, counts, games):
        """tg_sp_gumbel_target: the counts play() records for `games` (bool[G]) in place of their visit counts."""
        self.ctx.call("tg_sp_gumbel_target", _ptr(np.ascontiguousarray(counts, np.int32)), _ptr(np.ascontiguousarray(games, np.uint8)))

    def gumbel_stats(self):
        """Root selections made in Gumbel moves so far, and how many of them found no considered child at the schedule's value."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx.call("tg_sp_gumbel_stats", ctypes.byref(a), ctypes.byref(b))
        return dict(root_selections=int(a.value), fallback_selections=int(b.value))

    def choose_gumbel_moves(self, visits, steps, selfplay=True):
        """Move selection while gumbel_m > 0: the games in a Gumbel move take gumbel_moves()'s action, their pi is the improved
        policy, which is staged for play() to record, and their streams are not touched; every other game goes through
        choose_moves.  Returns (actions, pis, gumbel_game)."""
        gact, gg = self.gumbel_moves()
        actions, pis = self.choose_moves(visits, steps, selfplay, skip=gg)
        if gg.any():
            pi, counts = self.gumbel_targets(gg)
            self.stage_gumbel_targets(counts, gg)
            actions[gg] = gact[gg]; pis[gg] = pi[gg]
        return actions, pis, gg

    # ---- search ownership (tg_sp_search_ownership) --------------------------------------------------------------
    def set_search_ownership(self, on):
        """on: every simulation a search backs up also adds its leaf's ownership (the network's third head), turned to Black's
        point of view, to a per-game sum that root_ownership() reads as a mean -- KataGo's ownership map.  The search itself is
        unchanged.  Off is the default.  Refused while an evaluation cache is attached (it stores no ownership) and while a leaf
        batch is pending.  A host `evaluator` must return (policy, value, own) while it is on.  Context state: a snapshot carries
        neither the switch nor the sums."""
        self.ctx.call("tg_sp_search_ownership", 1 if on else 0)
        self.search_ownership = bool(on)

    def get_search_ownership(self):
        on = ctypes.c_int()
        self.ctx.call("tg_sp_search_ownership_get", ctypes.byref(on))
        return bool(on.value)

    def root_ownership(self):
        """tg_sp_root_ownership after a search with the mode on: "mean" float32 [G, S, S], the mean ownership over the evaluations
        the last search backed up (+1 Black ... -1 White), "n" int32 [G], how many those were (terminal simulations, the root's own
        evaluation and a reused sub-tree's earlier evaluations are not among them; a mean over 0 is all 0), and "score_lead"
        float32 [G] = float32 sum of the mean in point order - komi, Black's lead."""
        mean = np.zeros((self.G, self.S, self.S), np.float32); n = np.zeros(self.G, np.int32); lead = np.zeros(self.G, np.float32)
        self.ctx.call("tg_sp_root_ownership", _ptr(mean), _ptr(n), _ptr(lead))
        return dict(mean=mean, n=n, score_lead=lead)

    # ---- pass-alive end (tg_sp_pass_alive) ------------------------------------------------------------------------
    def set_pass_alive_end(self, on):
        """on: a game whose new root is settled after play() -- every point a pass-alive stone or pass-alive territory
        (transgo_amd/pass_alive.py) -- ends there like a game that ended by double pass, reset_from treats a settled position as a
        finished game, and harvest() / final() score every game with the pass-alive-aware area.  The search itself is unchanged.
        Off is the default.  Context state: a snapshot does not carry the switch, set it before restoring."""
        self.ctx.call("tg_sp_pass_alive", 1 if on else 0)
        self.pass_alive_end = bool(on)

    def get_pass_alive_end(self):
        on = ctypes.c_int()
        self.ctx.call("tg_sp_pass_alive_get", ctypes.byref(on))
        return bool(on.value)

    def pass_alive_stats(self):
        """-> dict(games_settled, plies_at_settlement_sum) since the mode was first turned on."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx.call("tg_sp_pass_alive_stats", ctypes.byref(a), ctypes.byref(b))
        return dict(games_settled=int(a.value), plies_at_settlement_sum=int(b.value))

    def root_pass_alive(self):
        """tg_sp_root_pass_alive: "status" int8 [G, P] and "settled" bool [G] of the games' current roots (a read-out; the mode
        need not be on)."""
        status = np.zeros((self.G, self.P), np.int8); settled = np.zeros(self.G, np.uint8)
        self.ctx.call("tg_sp_root_pass_alive", _ptr(status), _ptr(settled))
        return dict(status=status, settled=settled.astype(bool))

    # ---- policy surprise weighting (tg_sp_policy_surprise) ------------------------------------------------------
    POLICY_SURPRISE_STATS = ("positions_in", "positions_out", "games", "rows_forwarded")

    def set_policy_surprise(self, weight, seed=0):
        """weight > 0 (KataGo: 0.5): harvest() returns the finished games resampled on the device -- a position is written
        floor(w) or floor(w) + 1 times, w = (1 - weight) + weight * T * KL(search target || raw network policy) / the game's sum of
        those (transgo_amd.policy_surprise holds the definition).  0.0 = off: harvest() is tg_sp_harvest as ever.  No part of the
        search changes.  Context state: a restored snapshot does not carry it."""
        from types import SimpleNamespace
        from . import policy_surprise as _psw
        w, s = _psw.check_config(SimpleNamespace(policy_surprise_weight=weight, policy_surprise_seed=seed))
        self.ctx.call("tg_sp_policy_surprise", ctypes.c_double(w), s)
        self.policy_surprise_weight, self.policy_surprise_seed = w, s

    def get_policy_surprise(self):
        w, s = ctypes.c_double(), ctypes.c_uint32()
        self.ctx.call("tg_sp_policy_surprise_get", ctypes.byref(w), ctypes.byref(s))
        return float(w.value), int(s.value)

    def policy_surprise_stats(self):
        """tg_sp_policy_surprise_stats as a dict (POLICY_SURPRISE_STATS), plus the cumulative HIP-event milliseconds of the three
        stages (prior_ms, plan_ms, gather_ms) and the number of plans."""
        v = [ctypes.c_uint64() for _ in self.POLICY_SURPRISE_STATS]
        self.ctx.call("tg_sp_policy_surprise_stats", *[ctypes.byref(x) for x in v])
        out = {k: int(x.value) for k, x in zip(self.POLICY_SURPRISE_STATS, v)}
        ms = [ctypes.c_double() for _ in range(3)]; n = ctypes.c_int64()
        self.ctx.call("tg_prof_read_policy_surprise", *[ctypes.byref(x) for x in ms], ctypes.byref(n))
        out.update(prior_ms=ms[0].value, plan_ms=ms[1].value, gather_ms=ms[2].value, plans=int(n.value))
        return out

    def policy_surprise_plan(self, seeds, prior=None, readout=False):
        """tg_sp_policy_surprise_plan for the games the last play() finished: seeds uint32[G] by slot, prior float32 [n, A] host rows
        or None (the loaded network runs).  Returns n_out, or with readout=True a dict of n_out, surprise, weight, copies and the
        prior rows used."""
        ng, npos = ctypes.c_int32(), ctypes.c_int32()
        self.ctx.call("tg_sp_finished", ctypes.byref(ng), ctypes.byref(npos))
        npos = npos.value
        seeds = np.ascontiguousarray(seeds, np.uint32)
        assert seeds.shape == (self.G,), "seeds: one per slot"
        if prior is not None:
            prior = np.ascontiguousarray(prior, np.float32)
            assert prior.shape == (npos, self.A), (prior.shape, (npos, self.A))
            if npos == 0:
                prior = np.zeros((1, self.A), np.float32)              # no rows to read, but not the NULL that asks for the network
        n_out = ctypes.c_int32()
        if not readout:
            self.ctx.call("tg_sp_policy_surprise_plan", _ptr(prior), _ptr(seeds), ctypes.byref(n_out), None, None, None, None)
            return n_out.value
        r = dict(surprise=np.zeros(npos, np.float64), weight=np.zeros(npos, np.float64), copies=np.zeros(npos, np.int32),
                 prior=np.zeros((npos, self.A), np.float32))
        self.ctx.call("tg_sp_policy_surprise_plan", _ptr(prior), _ptr(seeds), ctypes.byref(n_out), _ptr(r["surprise"]),
                      _ptr(r["weight"]), _ptr(r["copies"]), _ptr(r["prior"]))
        r["n_out"] = n_out.value
        return r

    # ---- evaluation of the pending batch --------------------------------------------------------------------------------
    def _evaluate(self, rows=None):
        if self.evaluator is None:
            self.ctx.call("tg_sp_eval")
            return
        if rows is None:
            n = ctypes.c_int32()
            self.ctx.call("tg_sp_batch_rows", ctypes.byref(n))
            rows = n.value
        if rows == 0:
            return
        obs = np.empty((rows, self.C, self.S, self.S), np.float32)
        self.ctx.call("tg_sp_batch_obs", _ptr(obs), rows)
        m, a = self._host_symmetry
        out = (self.evaluator(obs) if m == 0 else
               _symmetry.evaluate_with_symmetry(self.evaluator, obs, ("none", "fixed", "position", "mean8")[m], a))
        policy, value = out[:2]
        policy = np.ascontiguousarray(policy, np.float32); value = np.ascontiguousarray(value, np.float32).reshape(-1)
        assert policy.shape == (rows, self.A) and value.shape == (rows,)
        if not self.search_ownership:
            self.ctx.call("tg_sp_set_eval", _ptr(policy), _ptr(value), rows)
            return
        if len(out) < 3 or out[2] is None:
            raise ValueError("search ownership is on: the evaluator must return (policy, value, own) with own [rows, S*S] from the side "
                             "to move's point of view, it returned a two-tuple")
        own = np.ascontiguousarray(out[2], np.float32).reshape(rows, -1)
        assert own.shape == (rows, self.P)
        self.ctx.call("tg_sp_set_eval_own", _ptr(policy), _ptr(value), _ptr(own), rows)

    # ---- reference-shaped operations, G games at a time -------------------------------------------------------------------
    def reset(self, seeds, mask=None):
        """reset_root (self_play.py:595-605) + np.random.seed(seed) per game."""
        seeds = np.ascontiguousarray(seeds, np.uint32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.ctx.call("tg_sp_reset", _ptr(seeds), _ptr(m))
        self._evaluate()
        self.ctx.call("tg_sp_expand_roots")
        if mask is None:
            self.finished[:] = False; self.errored[:] = False
        else:
            self.finished[np.asarray(mask, bool)] = False; self.errored[np.asarray(mask, bool)] = False

    def reset_from(self, states, mask=None):
        """Fresh roots at given positions: the first half of select_action (self_play.py:689-700).  states: [G, state_size]
        uint8 blobs (transgo_amd.environment.GoEnv states); unmasked slots are parked."""
        st = np.ascontiguousarray(states, np.uint8)
        assert st.shape[0] == self.G
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.ctx.call("tg_sp_reset_from", _ptr(st), _ptr(m))
        self._evaluate()
        self.ctx.call("tg_sp_expand_roots")
        self.finished = np.zeros(self.G, bool) if mask is None else ~np.asarray(mask, bool)
        if self.pass_alive_end:
            self.finished |= self.root_pass_alive()["settled"]        # pass-alive end: a settled position is a finished game

    def root_states(self):
        st = np.zeros((self.G, self.ctx.state_size), np.uint8)
        self.ctx.call("tg_sp_root_states", _ptr(st))
        return st

    def select_action(self, states, mask=None):
        """WP_MCTS.select_action (self_play.py:689-703) for G positions at once: fresh tree, no root noise, temperature
        0.12.  Returns the chosen actions (0 for parked slots)."""
        self.reset_from(states, mask)
        self.search(selfplay=False)
        vis, _, _, steps, _ = self.root_info(obs=False)
        actions, _ = self.choose_moves(vis, steps, selfplay=False)
        return actions

    def search(self, selfplay=True, num_simulation=0, noise=None, record=None):
        """The search part of get_action_probs (self_play.py:659-664).  Per-game arrays select tg_sp_begin_move_games (playout cap
        randomization): `noise` bool[G] = which games get root noise (default: all when selfplay, none otherwise; a game without
        noise draws nothing from its stream), `num_simulation` int[G] = every game's own budget (<= 0: the configured one),
        `record` bool[G] = False keeps the ply this move plays out of the game's training positions.  With none of them given
        the call is tg_sp_begin_move, as ever."""
        t0 = time.perf_counter()
        if noise is None and record is None and np.ndim(num_simulation) == 0:
            self.ctx.call("tg_sp_begin_move", 1 if selfplay else 0, num_simulation)
        else:
            sims = np.ascontiguousarray(np.broadcast_to(np.asarray(num_simulation), (self.G,)), np.int32)
            if noise is None:
                noise = np.full(self.G, bool(selfplay))
            nz = np.ascontiguousarray(np.broadcast_to(np.asarray(noise), (self.G,)) != 0, np.uint8)
            rec = None if record is None else np.ascontiguousarray(np.broadcast_to(np.asarray(record), (self.G,)) != 0, np.uint8)
            self.ctx.call("tg_sp_begin_move_games", _ptr(nz), _ptr(sims), _ptr(rec))
        self.begin_move_s += time.perf_counter() - t0
        if self.evaluator is None:
            w = ctypes.c_int32()
            self.ctx.call("tg_sp_search", ctypes.byref(w))
            return w.value
        waves = 0
        while True:
            act, rows = ctypes.c_int32(), ctypes.c_int32()
            self.ctx.call("tg_sp_collect", ctypes.byref(act), ctypes.byref(rows))
            self._evaluate(rows.value)
            self.ctx.call("tg_sp_absorb")
            if act.value == 0:
                return waves
            waves += 1

    def root_info(self, obs=True):
        vis = np.zeros((self.G, self.A), np.int32)
        rn = np.zeros(self.G, np.int32); pl = np.zeros(self.G, np.int32); st = np.zeros(self.G, np.int32)
        ob = np.zeros((self.G, self.C, self.S, self.S), np.float32) if obs else None
        self.ctx.call("tg_sp_root_info", _ptr(vis), _ptr(rn), _ptr(pl), _ptr(st), _ptr(ob))
        return vis, rn, pl, st, ob

    def root_visits(self, pruned=False):
        """Visit counts and ply counters only (what move selection needs): 4*(A+1) bytes per game across PCIe.  pruned=True
        (tg_sp_root_visits_pruned): the games whose move in progress is a forced one (forced playouts) report their pruned counts,
        every other game its raw ones -- what choose_moves is fed with while forced_playouts_k > 0."""
        vis = np.zeros((self.G, self.A), np.int32); st = np.zeros(self.G, np.int32)
        if pruned:
            self.ctx.call("tg_sp_root_info", None, None, None, _ptr(st), None)
            self.ctx.call("tg_sp_root_visits_pruned", _ptr(vis), None)
        else:
            self.ctx.call("tg_sp_root_info", _ptr(vis), None, None, _ptr(st), None)
        return vis, st

    def pruned_games(self):
        """bool[G]: the games tg_sp_root_visits_pruned prunes right now (their move began with root noise while k > 0)."""
        pg = np.zeros(self.G, np.uint8)
        self.ctx.call("tg_sp_root_visits_pruned", None, _ptr(pg))
        return pg != 0

    def root_plies(self):
        """Moves played so far in every slot's game (the state's step counter starts at 1, go_env.cc:67; a parked slot reads 0)."""
        st = np.zeros(self.G, np.int32)
        self.ctx.call("tg_sp_root_info", None, None, None, _ptr(st), None)
        return np.maximum(st - 1, 0)

    # ---- tree read-out (analysis; reads only, legal between any two engine calls) ------------------------------------------
    CHILD_PRESENT, CHILD_OPEN, CHILD_PRIOR32, CHILD_WIN, CHILD_LOSS = 1, 2, 4, 8, 16        # TG_CHILD_* bits of "flags"
    ROOT_OK, ROOT_PARKED, ROOT_UNEVALUATED, ROOT_TERMINAL, ROOT_ERROR = 0, 1, 2, 3, 4        # TG_ROOT_* values of "status"

    def root_children(self):
        """tg_sp_root_children: the Node_V fields (self_play.py:51-63) of every root child as dense [G, A] arrays -- "n", "pending",
        "w", "var" (float32 as stored), "prior" (float64), "flags" (CHILD_* bits; 0 = the action is not legal at the root) -- and
        per game "root_n", "root_pending", "root_w", "root_var" and "status" (ROOT_*)."""
        G, A = self.G, self.A
        r = dict(n=np.zeros((G, A), np.int32), pending=np.zeros((G, A), np.int32), w=np.zeros((G, A), np.float32),
                 var=np.zeros((G, A), np.float32), prior=np.zeros((G, A), np.float64), flags=np.zeros((G, A), np.uint8),
                 root_n=np.zeros(G, np.int32), root_pending=np.zeros(G, np.int32), root_w=np.zeros(G, np.float32),
                 root_var=np.zeros(G, np.float32), status=np.zeros(G, np.uint8))
        self.ctx.call("tg_sp_root_children", *[_ptr(a) for a in r.values()])
        return r

    def principal_variation(self, depth=16):
        """tg_sp_pv: per game the line of most-visited children (ties: lowest action) from the root, at most `depth` moves.
        Returns (actions [G, depth] padded with -1, visits [G, depth], w [G, depth], lengths [G])."""
        depth = int(depth)
        shape = (self.G, max(depth, 0))
        act = np.full(shape, -1, np.int32); n = np.zeros(shape, np.int32); w = np.zeros(shape, np.float32)
        ln = np.zeros(self.G, np.int32)
        self.ctx.call("tg_sp_pv", depth, _ptr(act), _ptr(n), _ptr(w), _ptr(ln))
        return act, n, w, ln

    def choose_moves(self, visits, steps, selfplay=True, skip=None):
        """self_play.py:666-683 for every live game, in NumPy float64 with the reference's own operations:
        counts==1 -> 0, pi = counts/sum, p ~ counts**(1/tau), and np.random.choice(A, p) spelt out as NumPy implements it
        (mtrand.pyx: cdf = p.cumsum(); cdf /= cdf[-1]; cdf.searchsorted(random_sample(), 'right')) with the uniform
        drawn from the game's own stream.  Vectorised over games; every operation is element-wise or a last-axis
        reduction, so each row equals the per-game 1-D computation bit for bit (tests/test_host_logic.py checks it
        against the literal per-game form, choose_moves_reference).  skip bool[G]: games that choose otherwise (a Gumbel move):
        no draw from their streams, action 0 and pi 0 here."""
        live = ~self.finished
        if skip is not None:
            live = live & ~np.asarray(skip, bool)
        u = np.zeros(self.G, np.float64)
        self.ctx.call("tg_sp_draw_uniform", _ptr(u), _ptr(live.astype(np.uint8)))
        return choose_moves_batch(visits, steps, u, live, selfplay)

    def play(self, actions):
        """update_with_action (self_play.py:857-872); the move's record entry is written on the device first.  Returns the
        mask of games that are over; `self.errored` marks slots parked by an arena overflow (neither over nor playable)."""
        done = np.zeros(self.G, np.uint8)
        self.ctx.call("tg_sp_play", _ptr(np.ascontiguousarray(actions, np.int32)), _ptr(done))
        self._evaluate()
        self.ctx.call("tg_sp_expand_roots")
        self.finished = done != 0
        self.errored = done == 2
        return done == 1

    def game_errors(self):
        n = ctypes.c_int32(); err = np.zeros(self.G, np.int32)
        self.ctx.call("tg_sp_game_errors", ctypes.byref(n), _ptr(err))
        return err

    def harvest(self, device=False, seeds=None):
        """The games the last play() finished, as one position-major batch (transgo_amd.records.Harvest), or None.
        device=True: the batch is a torch uint8 tensor in this GPU's memory and only the per-game tables cross PCIe.
        While policy_surprise_weight > 0 the batch is the resampled one (set_policy_surprise) and `seeds` is required."""
        from . import records
        ng, npos = ctypes.c_int32(), ctypes.c_int32()
        self.ctx.call("tg_sp_finished", ctypes.byref(ng), ctypes.byref(npos))
        ng, npos = ng.value, npos.value
        if ng == 0:
            return None
        fn = "tg_sp_harvest"
        if self.policy_surprise_weight > 0.0:
            # policy surprise weighting: the batch is resampled on the device before it leaves; everything behind this call keeps
            # seeing a position batch, only with other per-game lengths
            if seeds is None:
                raise ValueError("policy surprise weighting is on: harvest() needs the games' seeds (seeds=, one per slot) for the copy draws")
            prior = None
            if self.evaluator is not None and npos > 0:
                # a host evaluator stands in for the network: its policy rows for the harvested positions, identity orientation
                plain = records.Harvest(self.S, self.C, ng, npos, np.zeros(records.layout(self.S, self.C, ng, npos)[1], np.uint8))
                self.ctx.call("tg_sp_harvest", plain.ptr("obs_bits"), plain.ptr("counts"), plain.ptr("z"), plain.ptr("own"),
                              plain.ptr("player"), 0, None, None, None, None, None)
                prior = np.ascontiguousarray(self.evaluator(plain.observations())[0], np.float32)
            elif self.evaluator is not None:
                prior = np.zeros((0, self.A), np.float32)
            npos = self.policy_surprise_plan(seeds, prior)
            fn = "tg_sp_policy_surprise_harvest"
        sec, total = records.layout(self.S, self.C, ng, npos)
        hdr = records.header_bytes(self.S, self.C, ng)
        if device:
            import torch
            # zeros, not empty: the layout has alignment padding nobody writes, and the batch is compared / hashed / sent as bytes
            buf = torch.zeros(total, dtype=torch.uint8, device=torch.device("cuda", self.device))
            host = records.Harvest(self.S, self.C, ng, 0, np.zeros(hdr, np.uint8))        # per-game tables are written on the host
        else:
            buf = np.zeros(total, np.uint8)
        h = records.Harvest(self.S, self.C, ng, npos, buf)
        t = host if device else h
        self.ctx.call(fn, h.ptr("obs_bits"), h.ptr("counts"), h.ptr("z"), h.ptr("own"), h.ptr("player"),
                      1 if device else 0, t.ptr("slot"), t.ptr("n_moves"), t.ptr("winner"), t.ptr("score"), t.ptr("terr"))
        if seeds is not None:
            t.view("seed")[:] = np.asarray(seeds, np.uint32)[t.view("slot")]
        if device:
            buf[:hdr].copy_(torch.from_numpy(host.buf))
        return h

    # ---- checkpoint and resume ------------------------------------------------------------------------------------------------
    def snapshot(self, device=False):
        """tg_sp_snapshot: the whole engine -- every game's tree, control record, RNG stream and move record, the tree pool's ring
        and statistics, the counters, finished games not harvested yet -- as one flat uint8 buffer: a NumPy array, or with
        device=True a torch tensor in this GPU's memory (fork / migrate without a host bounce).  Legal at a move boundary only
        (between play() / reset() and the next search()).  The tree pool is packed: the buffer costs what the trees use, not what
        the pool was provisioned with.  Network weights are not part of it.  (Two library calls: the size first, because the buffer
        is allocated here; each runs the small scan kernel and one stream sync -- tens of microseconds next to the copy.  A host
        snapshot leaves a staging buffer of its size in HBM with the context, for the next one.)"""
        n = ctypes.c_uint64()
        self.ctx.call("tg_sp_snapshot_size", ctypes.byref(n))
        w = ctypes.c_uint64()
        if device:
            import torch
            buf = torch.empty(n.value, dtype=torch.uint8, device=torch.device("cuda", self.device))
            self.ctx.call("tg_sp_snapshot", ctypes.c_void_p(buf.data_ptr()), n.value, 1, ctypes.byref(w))
        else:
            buf = np.empty(n.value, np.uint8)
            self.ctx.call("tg_sp_snapshot", _ptr(buf), n.value, 0, ctypes.byref(w))
        return buf[:w.value]

    def restore(self, buf):
        """tg_sp_restore: take a snapshot() back -- into this engine or into another one created with the same geometry (board,
        n_games, parallel_readouts, max_step, komi, search constants, record_games, arena_slots, pool_slots; num_simulation and the
        device may differ) -- and with it `finished` / `errored`.  A damaged or mismatched buffer raises and leaves the engine as
        it was.  Weights are the caller's to load, before or after."""
        from . import snapshot as _snap
        if isinstance(buf, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(buf, np.uint8)
        on_gpu = not isinstance(buf, np.ndarray) and buf.is_cuda
        if not isinstance(buf, np.ndarray) and not on_gpu:
            buf = buf.numpy()
        if on_gpu:
            if buf.device.index != self.device:
                raise ValueError(f"the snapshot tensor lives on GPU {buf.device.index}, this engine on GPU {self.device}: move it with "
                                 f".to('cuda:{self.device}') first (tg_sp_restore reads device buffers of its own GPU only)")
            assert buf.dtype.itemsize == 1 and buf.is_contiguous()
            self.ctx.call("tg_sp_restore", ctypes.c_void_p(buf.data_ptr()), buf.numel(), 1)
            hdr = _snap.parse_header(buf[:_snap.HEADER_BYTES].cpu().numpy())
            off, size = hdr["sections"]["game_ctl"]
            ctl = buf[off:off + size].cpu().numpy().view(_snap.GAME_CTL)
        else:
            buf = np.ascontiguousarray(buf, np.uint8)
            self.ctx.call("tg_sp_restore", _ptr(buf), buf.size, 0)
            hdr = _snap.parse_header(buf)
            ctl = _snap.section(buf, hdr, "game_ctl", _snap.GAME_CTL)
        self.finished, self.errored = _snap.game_flags(ctl)

    def final(self):
        score = np.zeros(self.G, np.float32); terr = np.zeros((self.G, self.P), np.float32); win = np.zeros(self.G, np.int32)
        self.ctx.call("tg_sp_final", _ptr(score), _ptr(terr), _ptr(win))
        return score, terr, win

    def rng_state(self, game):
        s = _lib.TgMt19937()
        self.ctx.call("tg_sp_rng_state", int(game), ctypes.byref(s))
        return np.frombuffer(s.key, np.uint32).copy(), int(s.pos)

    def rng_streams(self):
        """All G MT19937 streams as a uint8 array [G][sizeof(tg_mt19937)] (opaque; hand it to set_rng_streams)."""
        out = np.zeros((self.G, ctypes.sizeof(_lib.TgMt19937)), np.uint8)
        self.ctx.call("tg_sp_rng_get", _ptr(out))
        return out

    def set_rng_streams(self, streams, mask=None):
        st = np.ascontiguousarray(streams, np.uint8)
        assert st.shape == (self.G, ctypes.sizeof(_lib.TgMt19937))
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.ctx.call("tg_sp_rng_set", _ptr(st), _ptr(m))

    def stats(self):
        v = [ctypes.c_uint64() for _ in range(4)]; e = ctypes.c_int32(); m = ctypes.c_int32()
        self.ctx.call("tg_sp_stats", *[ctypes.byref(x) for x in v], ctypes.byref(e), ctypes.byref(m))
        tr = ctypes.c_uint64()
        self.ctx.call("tg_sp_tree_truncations", ctypes.byref(tr))
        out = dict(sims=v[0].value, evals=v[1].value, depth_sum=v[2].value, tie_draws=v[3].value, errors=e.value,
                   max_slots=m.value, truncated_blocks=tr.value, fp16_overflows=0)
        out.update(self.pool_stats())
        if self.evaluator is None:
            out["fp16_overflows"] = self.net_range()["fp16_overflows"]
        return out

    def pool_stats(self):
        """tg_sp_pool_stats: the tree pool all games share -- its size, the most that was in use at once, what is in use now (32-byte
        slots) and how often a game found it empty."""
        v = [ctypes.c_uint64() for _ in range(4)]
        self.ctx.call("tg_sp_pool_stats", *[ctypes.byref(x) for x in v])
        return dict(pool_slots=v[0].value, pool_high_water=v[1].value, pool_in_use=v[2].value, pool_exhausted=v[3].value)

    def net_range(self):
        """tg_net_range: sticky count of output tiles in which a value beyond +-65504 was rounded to fp16 (net_precision 1-3; 0 = every
        forward pass so far stayed in range) and the largest |w| of the live BN-folded weight blob."""
        n = ctypes.c_uint64(); w = ctypes.c_float()
        if self.ctx.lib.tg_net_range(self.ctx.h, ctypes.byref(n), ctypes.byref(w)) != 0:
            return {"fp16_overflows": 0, "weight_absmax": None}              # no network loaded in this context (yet)
        return {"fp16_overflows": int(n.value), "weight_absmax": float(w.value)}
