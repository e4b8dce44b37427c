"""Test helper: the oracle search with the Gumbel root rule, written with the functions of transgo_amd/gumbel.py (the definition)
on top of oracle/wp_mcts.py's OracleSearch.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle.wp_mcts import OracleSearch
from transgo_amd import gumbel as gb


class GumbelOracleSearch(OracleSearch):
    def __init__(self, *args, gumbel_m=0, c_visit=50.0, c_scale=1.0, **kw):
        self.gumbel_m, self.c_visit, self.c_scale = int(gumbel_m), float(c_visit), float(c_scale)
        self.in_gumbel = False                    # the move in progress is a Gumbel move
        self.root_selections = self.fallback_selections = 0
        self.gl = self.n0 = None
        self.base_n = self.budget = 0
        super().__init__(*args, **kw)

    def pick_child(self, node):
        if not (self.in_gumbel and node is self.root):
            return super().pick_child(node)
        acts = list(node.kids.keys())
        kids = [(c.n, c.pending, c.w) for c in node.kids.values()]
        scores, elig, fallback = gb.select(self.gl, kids, self.n0, node.n, node.pending, self.base_n, self.wu, self.gumbel_m, self.budget,
                                           self.c_visit, self.c_scale)
        self.root_selections += 1
        self.fallback_selections += int(fallback)
        best = max(scores[i] for i in elig)
        tied = [acts[i] for i in elig if scores[i] == best]
        a = self.rng.choice(tied)
        return a, node.kids[a]

    def raw_counts(self):
        return np.array([self.root.kids[a].n if a in self.root.kids else 0 for a in range(self.A)])

    def by_action(self, values, fill):
        out = np.full(self.A, fill, np.float64)
        out[list(self.root.kids.keys())] = values
        return out

    def search_move(self, selfplay=True):
        if not (selfplay and self.gumbel_m > 0):
            a, pi, obs, info = super().search_move(selfplay)
            info.update(raw=self.raw_counts(), gumbel=False, record=self.raw_counts())     # the record keeps raw visits
            return a, pi, obs, info
        root = self.root
        acts = list(root.kids.keys())
        g = gb.draw(self.rng, len(acts))
        self.gl = gb.table(g, [c.prior for c in root.kids.values()], self.gumbel_m)
        self.n0 = [c.n for c in root.kids.values()]
        self.base_n, self.budget = root.n, self.num_simulation
        self.in_gumbel = True
        while root.n < self.base_n + self.num_simulation:
            self.wave()
        self.in_gumbel = False
        kids = list(root.kids.values())
        i = gb.pick_move(self.gl, [(c.n, c.w) for c in kids], self.n0, self.c_visit, self.c_scale)
        action = acts[i]
        pi = self.by_action(gb.improved_policy_row([(c.prior, c.n, c.w) for c in kids], self.c_visit, self.c_scale), 0.0)
        obs = self.env.encode(root.state)
        info = dict(n0=self.base_n, raw=self.raw_counts(), gumbel=True, record=gb.fixed_point(pi), gl=self.by_action(self.gl, -np.inf),
                    effort=self.by_action([c.n - b for c, b in zip(kids, self.n0)], 0).astype(np.int64), root_n=root.n)
        return action, pi, obs, info


def play_moves(evaluate, seed, m, moves, sims, board_size=9, max_step=120, readouts=4, selfplay=True, c_visit=50.0, c_scale=1.0):
    """`moves` searched moves of one game seeded `seed`: per move the raw counts, gl table, action, pi, recorded counts, the stream
    position and the chosen child's n; plus the search object."""
    from oracle.go_oracle import OracleGoEnv
    rng = np.random.RandomState(int(seed))
    o = GumbelOracleSearch(OracleGoEnv(board_size=board_size, max_step=max_step), evaluate, rng, num_simulation=sims,
                           parallel_readouts=readouts, board_size=board_size, gumbel_m=m, c_visit=c_visit, c_scale=c_scale)
    out = []
    for _ in range(moves):
        nchild = len(o.root.kids)
        a, pi, obs, info = o.search_move(selfplay)
        child_n = o.root.kids[a].n
        done = o.advance(a)
        out.append(dict(raw=info["raw"], action=int(a), pi=pi, record=np.asarray(info["record"]), gumbel=info["gumbel"], gl=info.get("gl"),
                        effort=info.get("effort"), n0=info["n0"], pos=int(rng.get_state()[2]), child_n=child_n, new_root_n=o.root.n,
                        nchild=nchild))
        if done:
            break
    return out, o
