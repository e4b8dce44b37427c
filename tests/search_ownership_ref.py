"""Test helper: search ownership restated on top of oracle/wp_mcts.py's OracleSearch -- a mixin that keeps own_sum /
own_n with the engine's semantics in NumPy float32, the two stand-in ownership functions and the evaluator wrappers that return
(policy, value, own).  TEST INFRASTRUCTURE ONLY.

What contributes is exactly what OracleSearch.absorb backs up: a path whose leaf is not open yet when its turn comes.  The sign comes
from the leaf's own state (env.getPlayer), not from the root and the path's parity as the kernel computes it: two statements of one
rule."""
import numpy as np

from oracle import evaluators
from oracle.evaluators import _hash_planes
from oracle.wp_mcts import OracleSearch

BLACK = 1
F32 = np.float32


def own_exact(obs):
    """((h % 33) - 16) / 16: dyadic, so every partial sum of a few thousand of them is exact in float32 -- a mismatch is a wrong set
    of contributions or a wrong sign, never rounding."""
    h, _ = _hash_planes(np.asarray(obs))
    return ((h % 33) - 16).astype(F32) / F32(16)


def own_tenths(obs):
    """((h % 21) - 10) / 10: one float32 division; the partial sums round, which pins the order of the additions."""
    h, _ = _hash_planes(np.asarray(obs))
    return ((h % 21) - 10).astype(F32) / F32(10)


OWN_BY_NAME = {"exact": own_exact, "tenths": own_tenths}

R = 4
# The cases of tests/test_gpu_search_ownership.py: name -> (evaluator, board, games, simulations, moves, max_step, first seed).
# tests/test_search_ownership_host.py asserts on the CPU what each must contain (dropped duplicate leaves, terminal simulations,
# roots of both colours, moves that begin on a reused sub-tree, a search that completes only terminal simulations).
CASES = {
    "flat9": ("flat", 9, 6, 48, 5, 5, 900),            # max_step = 5: the fifth move's search meets nothing but the end of the game
    "flat19": ("flat", 19, 2, 32, 2, 450, 930),        # 361 points: six strides of 64 and a tail of 41
    "rule9": ("flat", 9, 6, 32, 5, 5, 900),            # the same games under the forced-playout and the Gumbel root rule
}


def with_own(name, own_fn):
    """The stand-in evaluator `name` (flat | sharp | spike) returning (policy, value, own)."""
    base = evaluators.BY_NAME[name]

    def evaluate(obs):
        p, v = base(obs)
        return p, v, own_fn(obs)
    return evaluate


def read_out(own_sum, own_n, komi):
    """tg_sp_root_ownership: one float32 division per point, the sequential float32 sum in point order, - komi."""
    if own_n == 0:
        mean = np.zeros_like(own_sum)
    else:
        mean = own_sum / F32(own_n)
    s = mean[0]
    for p in range(1, len(mean)):
        s = F32(s + mean[p])
    return mean, F32(s - F32(komi))


class OwnershipMixin:
    """Put in front of OracleSearch (or of a subclass with another root rule): the evaluator returns (policy, value, own)."""

    def __init__(self, *args, invert_sign=False, komi=7.5, **kw):
        self.invert_sign = bool(invert_sign)       # negative control: contributions from the leaf mover's own side
        self.komi = komi
        self.terminal_sims = self.dropped_paths = 0          # counted over the object's life
        self._last_own = None
        super().__init__(*args, **kw)              # (reset_root inside clears the accumulators)

    def clear_ownership(self):
        self.own_sum = np.zeros(self.S * self.S, F32)
        self.own_n = 0

    def _eval(self, states):
        obs = np.array([self.env.encode(s) for s in states], dtype="float32")
        policy, value, own = self.evaluate(obs)
        self.leaves_evaluated += len(states)
        self._last_own = np.asarray(own, F32).reshape(len(states), -1)
        return policy, value

    def reset_root(self):                          # tg_sp_reset; the root's own evaluation contributes nothing
        self.clear_ownership()
        super().reset_root()

    def search_move(self, selfplay=True):          # tg_sp_begin_move
        self.clear_ownership()
        if self.trace is not None:
            self.trace.append(("move", dict(root_player=int(self.env.getPlayer(self.root.state)), root_n=int(self.root.n))))
        return super().search_move(selfplay)

    def collect(self):
        before = self.sims_done
        paths, leaves = super().collect()
        self.terminal_sims += self.sims_done - before          # terminal leaves are backed up inside collect, without a network row
        if self.trace is not None and self.sims_done != before:
            self.trace.append(("terminal", self.sims_done - before))
        return paths, leaves

    def absorb(self, paths, leaves, probs, values):
        own = self._last_own
        root_black = self.env.getPlayer(self.root.state) == BLACK
        for i, (path, leaf_state, prob, value) in enumerate(zip(paths, leaves, probs, values)):
            dropped = path[-1].open                            # the duplicate leaf of a wave
            super().absorb([path], [leaf_state], [prob], [value])
            if dropped:
                self.dropped_paths += 1
                if self.trace is not None:
                    self.trace.append(("dropped", None))
                continue
            black = self.env.getPlayer(leaf_state) == BLACK
            assert black == (root_black == ((len(path) - 1) % 2 == 0))         # the kernel's form of the same rule
            s = F32(1) if black != self.invert_sign else F32(-1)
            self.own_sum = (self.own_sum + s * own[i]).astype(F32)             # float32 + float32, element by element
            self.own_n += 1
            if self.trace is not None:
                self.trace.append(("absorb", leaf_state))

    def root_ownership(self):
        mean, lead = read_out(self.own_sum, self.own_n, self.komi)
        return dict(mean=mean.copy(), n=int(self.own_n), score_lead=lead)


class OwnOracleSearch(OwnershipMixin, OracleSearch):
    pass


def search_class(rule="plain"):
    """The restatement search with the mixin for a root rule: plain | forced | gumbel."""
    if rule == "plain":
        return OwnOracleSearch
    if rule == "forced":
        from tests.forced_playouts_ref import ForcedOracleSearch
        return type("OwnForcedOracleSearch", (OwnershipMixin, ForcedOracleSearch), {})
    if rule == "gumbel":
        from tests.gumbel_ref import GumbelOracleSearch
        return type("OwnGumbelOracleSearch", (OwnershipMixin, GumbelOracleSearch), {})
    raise ValueError(rule)


def case_seeds(case):
    G, s0 = CASES[case][2], CASES[case][6]
    return np.arange(s0, s0 + G).astype(np.uint32)


def play_case(case, own="tenths", rule="plain", invert_sign=False, trace=False, **rule_kw):
    """Every game of a case: [(moves, search object, trace or None)] in seed order."""
    name, S, G, sims, moves, max_step, _ = CASES[case]
    out = []
    for s in case_seeds(case):
        tr = [] if trace else None
        mv, o = play_moves(with_own(name, OWN_BY_NAME[own]), int(s), moves, sims, board_size=S, max_step=max_step, readouts=R, rule=rule,
                           invert_sign=invert_sign, trace=tr, **rule_kw)
        out.append((mv, o, tr))
    return out


def play_moves(evaluate, seed, moves, sims, board_size=9, max_step=120, readouts=4, selfplay=True, rule="plain", trace=None,
               invert_sign=False, komi=7.5, **rule_kw):
    """`moves` searched moves of one game seeded `seed`.  Per move: the raw root visits, the action, the stream position, the
    ownership read-out (mean [P], n, score_lead) and what the case conditions ask about -- the root's side to move, root.n when the
    search began (> 0: a reused sub-tree), terminal simulations and dropped duplicate leaves of the move.  Plus the search object."""
    from oracle.go_oracle import OracleGoEnv
    rng = np.random.RandomState(int(seed))
    o = search_class(rule)(OracleGoEnv(board_size=board_size, max_step=max_step), evaluate, rng, num_simulation=sims,
                           parallel_readouts=readouts, board_size=board_size, trace=trace, invert_sign=invert_sign, komi=komi, **rule_kw)
    out = []
    for _ in range(moves):
        player, n0 = int(o.env.getPlayer(o.root.state)), int(o.root.n)
        t0, d0 = o.terminal_sims, o.dropped_paths
        a, pi, obs, info = o.search_move(selfplay)
        raw = np.array([o.root.kids[i].n if i in o.root.kids else 0 for i in range(o.A)])
        rec = dict(raw=raw, action=int(a), pi=pi, root_player=player, root_n0=n0, terminal=o.terminal_sims - t0,
                   dropped=o.dropped_paths - d0, **o.root_ownership())
        done = o.advance(a)
        rec["pos"] = int(rng.get_state()[2])
        out.append(rec)
        if trace is not None:
            trace.append(("played", int(a)))
        if done:
            break
    return out, o
