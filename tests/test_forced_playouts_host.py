"""Forced playouts and policy target pruning on the CPU: the definition (transgo_amd/forced_playouts.py) inside the oracle search
(tests/forced_playouts_ref.py).  The GPU tests (tests/test_gpu_forced_playouts.py) hold the kernels to the same helper.

The (evaluator, seed) pairs were picked with the oracle: with `sharp` and seed 500 the k = 2 search visits other root children
than the k = 0 search already in the first move (test_k2_changes_the_search names the pair)."""
import functools

import numpy as np
import pytest

from oracle import evaluators
from transgo_amd import forced_playouts as fp

SIMS, MOVES = 48, 4
PAIRS = [("sharp", 500), ("flat", 501)]
C1, C2 = 3, 0.05


@functools.lru_cache(maxsize=None)
def _forced_game(name, seed, k):
    from tests.forced_playouts_ref import play_moves
    return play_moves(evaluators.BY_NAME[name], seed, k, MOVES, SIMS)


@functools.lru_cache(maxsize=None)
def _plain_game(name, seed):
    from oracle.go_oracle import OracleGoEnv
    from oracle.wp_mcts import OracleSearch
    rng = np.random.RandomState(seed)
    o = OracleSearch(OracleGoEnv(), evaluators.BY_NAME[name], rng, num_simulation=SIMS)
    out = []
    for _ in range(MOVES):
        a, pi, obs, info = o.search_move()
        raw = np.array([o.root.kids[i].n if i in o.root.kids else 0 for i in range(82)])
        o.advance(a)
        out.append(dict(raw=raw, action=int(a), pi=pi, pos=int(rng.get_state()[2])))
    return out, rng.get_state()


@pytest.mark.parametrize("name,seed", PAIRS)
def test_k0_is_the_oracle_search_move_for_move(name, seed):
    """The overridden selection with k = 0 scores every root child with forced_playouts.score and forces nothing: raw visits,
    actions, pi and the position (and key) of the MT19937 stream are OracleSearch's."""
    want, st = _plain_game(name, seed)
    got, o = _forced_game(name, seed, 0.0)
    assert len(got) == len(want) == MOVES
    for m, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a["raw"], b["raw"]) and np.array_equal(a["pruned"], b["raw"]), m
        assert a["action"] == b["action"] and np.array_equal(a["pi"], b["pi"]) and a["pos"] == b["pos"], m
    assert np.array_equal(o.rng.get_state()[1], st[1]) and o.rng.get_state()[2] == st[2]
    assert o.forced_selections == 0


def test_k2_changes_the_search():
    """The condition on the inputs: for (sharp, 500) the raw root visits of the k = 2 search differ from the k = 0 search's."""
    a, o = _forced_game("sharp", 500, 2.0)
    b, _ = _forced_game("sharp", 500, 0.0)
    assert not np.array_equal(a[0]["raw"], b[0]["raw"])
    assert 0 < o.forced_selections < o.root_selections
    assert any((m["raw"] != m["pruned"]).any() for m in a)


@functools.lru_cache(maxsize=None)
def _roots(name, seed, k=2.0):
    """The root of every move of a k = 2 game as the search left it: (children tuples in action order, actions, root.n)."""
    from oracle.go_oracle import OracleGoEnv
    from tests.forced_playouts_ref import ForcedOracleSearch
    rng = np.random.RandomState(seed)
    o = ForcedOracleSearch(OracleGoEnv(), evaluators.BY_NAME[name], rng, num_simulation=SIMS, forced_k=k)
    out = []
    for _ in range(MOVES):
        a, _, _, info = o.search_move()
        kids = [(c.prior, c.n, c.w, c.var) for c in o.root.kids.values()]
        out.append((kids, list(o.root.kids.keys()), o.root.n, info))
        o.advance(a)
    return out


@pytest.mark.parametrize("name,seed", PAIRS)
def test_pruning_properties(name, seed):
    pruned_any = 0
    for kids, acts, root_n, info in _roots(name, seed):
        raw = [c[1] for c in kids]
        out = fp.prune(2.0, C1, C2, kids, root_n)
        assert np.array_equal(np.asarray(out), info["pruned"][acts]) and np.array_equal(np.asarray(raw), info["raw"][acts])
        star = fp.best_child(raw)
        assert raw[star] == max(raw) and raw.index(max(raw)) == star          # most visits, lowest action on a tie
        p, n, w, var = kids[star]
        s_star = fp.score(C1, C2, p, n, 0, w, var, root_n)
        assert out[star] == raw[star]                                          # c* is untouched
        assert sum(out) > 0
        for i, (p, n, w, var) in enumerate(kids):
            assert 0 <= out[i] <= raw[i]
            if raw[i] == 0:
                assert out[i] == 0                                             # an unvisited child stays 0
            if i == star or raw[i] == 0:
                continue
            lim = min(fp.forced_budget(2.0, p, root_n), raw[i])
            if out[i] < raw[i]:                                                # a pruned child
                pruned_any += 1
                assert fp.score(C1, C2, p, n, 0, w, var, root_n, denom_n=out[i]) < s_star or out[i] == raw[i] - lim
            if out[i] > raw[i] - lim:                                          # it stopped early: one visit fewer would not score below S*
                assert not fp.score(C1, C2, p, n, 0, w, var, root_n, denom_n=out[i] - 1) < s_star
    assert pruned_any > 0


def test_hand_built_root():
    """c1 = 3, c2 = 0.05, k = 2, root.n = 100, every variance 0, so s = float32(0.05) in every score.
    c* = A (60 visits, prior 0.5, q = +0.5): S* = 3 * 0.5 * 10 / 61 + s + 0.5 = 0.7459.. + s.
    B: prior 1/8, n = 6, w = +3 (q term -3/7): f = floor(sqrt(2 * 100 / 8)) = 5; score'(n') = 3.75 / (n' + 1) + s - 0.4286 is below
       S* for n' + 1 = 6, 5, 4 (0.9375 - 0.4286 = 0.5089) and not for n' + 1 = 3 (1.25 - 0.4286 = 0.8214): three visits go, 3 stay.
    C: prior 1/8, n = 2, w = -1 (q term +1/3): score'(1) = 1.875 + s + 0.3333 >= S*: nothing goes.
    D: prior 1/32, n = 8, w = +8 (q term -8/9): f = floor(sqrt(6.25)) = 2; every reduced count scores below S*: 8 - 2 = 6.
    E: never visited: 0."""
    f32 = np.float32
    kids = [(np.float64(0.5), 60, f32(-30.5), f32(0)), (np.float64(0.125), 6, f32(3), f32(0)), (np.float64(0.125), 2, f32(-1), f32(0)),
            (np.float64(0.03125), 8, f32(8), f32(0)), (np.float64(0.2), 0, f32(0), 0.)]
    assert fp.forced_budget(2.0, kids[1][0], 100) == 5 and fp.forced_budget(2.0, kids[3][0], 100) == 2
    assert fp.prune(2.0, C1, C2, kids, 100) == [60, 3, 2, 6, 0]
    assert fp.prune(0.0, C1, C2, kids, 100) == [60, 6, 2, 8, 0]
    # a tie for the most visits goes to the lowest action: with B at 60 visits as well, A is still c* and B is the one pruned
    tie = [kids[0], (np.float64(0.125), 60, f32(30), f32(0))]
    assert fp.best_child([60, 60]) == 0 and fp.prune(2.0, C1, C2, tie, 120)[0] == 60


def test_forced_rule_by_arithmetic():
    """n + pending < sqrt(k * prior * total): prior 1/8, k = 2, total 100 -> the bound is 5 exactly (strict); n = 0 is never forced."""
    p = np.float64(0.125)
    assert fp.is_forced(2.0, p, 4, 0, 100) and fp.is_forced(2.0, p, 2, 2, 100)
    assert not fp.is_forced(2.0, p, 5, 0, 100) and not fp.is_forced(2.0, p, 3, 2, 100)
    assert not fp.is_forced(2.0, p, 0, 0, 100) and not fp.is_forced(0.0, p, 1, 0, 100)


def test_score_is_the_oracle_score():
    """forced_playouts.score against OracleSearch.score on every root child of searched roots, pending counters included."""
    from oracle.go_oracle import OracleGoEnv
    from oracle.wp_mcts import OracleSearch
    rng = np.random.RandomState(7)
    o = OracleSearch(OracleGoEnv(), evaluators.flat, rng, num_simulation=24)
    o.root.add_root_noise(rng)
    seen = 0
    for _ in range(8):
        paths, leaves = o.collect()                                            # pending counters are up between collect and absorb
        for c in o.root.kids.values():
            a, b = o.score(o.root, c), fp.score(o.c1, o.c2, c.prior, c.n, c.pending, c.w, c.var, o.root.n + o.root.pending)
            assert type(a) is type(b) and a == b
            seen += c.pending > 0
        probs, values = o._eval(leaves)
        o.absorb(paths, leaves, probs, values)
    assert seen > 0


def test_prune_tables_equals_prune():
    """The array form (root_children() tables) gives what the per-child form gives on the oracle's roots."""
    for kids, acts, root_n, info in _roots("sharp", 500)[:2]:
        A = 82
        t = dict(n=np.zeros((1, A), np.int32), w=np.zeros((1, A), np.float32), var=np.zeros((1, A), np.float32),
                 prior=np.zeros((1, A), np.float64), flags=np.zeros((1, A), np.uint8), root_n=np.array([root_n], np.int32))
        for a, (p, n, w, var) in zip(acts, kids):
            t["n"][0, a], t["w"][0, a], t["var"][0, a], t["prior"][0, a], t["flags"][0, a] = n, w, var, p, 1
        assert np.array_equal(fp.prune_tables(2.0, C1, C2, t)[0], info["pruned"])
        assert np.array_equal(fp.prune_tables(2.0, C1, C2, t, forced_games=[False])[0], info["raw"])


def test_config_and_binding():
    from transgo_amd import _lib
    from transgo_amd.configure import Config
    assert Config().forced_playouts_k == 0.0 and Config(forced_playouts_k=2.0).forced_playouts_k == 2.0
    for bad in (-1.0, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="forced_playouts_k"):
            Config(forced_playouts_k=bad)
    for name, nargs in (("tg_sp_forced_playouts", 2), ("tg_sp_forced_playouts_get", 2), ("tg_sp_root_visits_pruned", 3)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
