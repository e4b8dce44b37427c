"""Test helper: the oracle search with forced playouts and policy target pruning, written with the functions of
transgo_amd/forced_playouts.py (the definition) on top of oracle/wp_mcts.py's OracleSearch.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle.wp_mcts import OracleSearch, temperature
from transgo_amd import forced_playouts as fp


class ForcedOracleSearch(OracleSearch):
    def __init__(self, *args, forced_k=0.0, **kw):
        self.forced_k = float(forced_k)
        self.noised = False                       # the move in progress began with root noise
        self.root_selections = self.forced_selections = 0
        super().__init__(*args, **kw)

    # selection at the root of a noised move: the spec's score and forced rule (with k = 0 nothing is ever forced, and the scores
    # must be OracleSearch.score's bit for bit -- the k = 0 test holds the two together); every other level is the parent's
    def pick_child(self, node):
        if not (self.noised and node is self.root):
            return super().pick_child(node)
        total = node.n + node.pending

        def sc(c):
            if fp.is_forced(self.forced_k, c.prior, c.n, c.pending, total):
                return np.inf
            return fp.score(self.c1, self.c2, c.prior, c.n, c.pending, c.w, c.var, total)
        best = max(sc(c) for c in node.kids.values())
        tied = [a for a, c in node.kids.items() if sc(c) == best]
        if self.forced_k > 0:
            self.root_selections += 1
            self.forced_selections += int(best == np.inf)
        a = self.rng.choice(tied)
        return a, node.kids[a]

    def raw_counts(self):
        return np.array([self.root.kids[a].n if a in self.root.kids else 0 for a in range(self.A)])

    def pruned_counts(self):
        acts = list(self.root.kids.keys())
        kids = [(c.prior, c.n, c.w, c.var) for c in self.root.kids.values()]
        out = np.zeros(self.A, np.int64)
        out[acts] = fp.prune(self.forced_k, self.c1, self.c2, kids, self.root.n)
        return out

    def search_move(self, selfplay=True):
        self.noised = bool(selfplay)
        if selfplay:
            self.root.add_root_noise(self.rng)
        n0 = self.root.n
        while self.root.n < n0 + self.num_simulation:
            self.wave()
        raw = self.raw_counts()
        forced = self.noised and self.forced_k > 0
        pruned = self.pruned_counts() if forced else raw
        self.noised = False
        counts = np.where(pruned == 1, 0, pruned)
        pi = counts / np.sum(counts)
        tau = temperature(self.env.getStep(self.root.state)) if selfplay else 0.12
        powed = np.power(counts, 1.0 / tau)
        probs = np.array(powed) / np.sum(powed)
        action = self.rng.choice(np.arange(self.A), p=probs)
        obs = self.env.encode(self.root.state)
        return action, pi, obs, dict(n0=n0, counts=counts, raw=raw, pruned=pruned, forced=forced, tau=tau, root_n=self.root.n)


def play_moves(evaluate, seed, k, moves, sims, board_size=9, max_step=120, readouts=4, selfplay=True):
    """`moves` searched moves of one game seeded `seed`: per move raw / pruned counts, action, pi, the stream position and the
    chosen child's n; plus the search object."""
    from oracle.go_oracle import OracleGoEnv
    rng = np.random.RandomState(int(seed))
    o = ForcedOracleSearch(OracleGoEnv(board_size=board_size, max_step=max_step), evaluate, rng, num_simulation=sims,
                           parallel_readouts=readouts, board_size=board_size, forced_k=k)
    out = []
    for _ in range(moves):
        a, pi, obs, info = o.search_move(selfplay)
        child_n = o.root.kids[a].n
        done = o.advance(a)
        out.append(dict(raw=info["raw"], pruned=info["pruned"], action=int(a), pi=pi, pos=int(rng.get_state()[2]), child_n=child_n,
                        new_root_n=o.root.n, root_n=info["root_n"]))
        if done:
            break
    return out, o
