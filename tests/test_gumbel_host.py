"""Gumbel root search on the CPU: the definition (transgo_amd/gumbel.py) inside the oracle search (tests/gumbel_ref.py).  The GPU
tests (tests/test_gpu_gumbel.py) hold the kernels to the same helper.

The (evaluator, seed) pair was picked with the oracle: with `sharp` and seed 500, m = 16 and 64 simulations, the searched root of
the first move differs from the PUCT search's (test_m16_changes_the_search names the pair)."""
import ctypes
import functools
import math

import numpy as np
import pytest

from oracle import evaluators
from transgo_amd import gumbel as gb

SIMS, MOVES, M = 64, 4, 16
PAIRS = [("sharp", 500), ("flat", 501)]


@functools.lru_cache(maxsize=None)
def _game(name, seed, m, sims=SIMS):
    from tests.gumbel_ref import play_moves
    return play_moves(evaluators.BY_NAME[name], seed, m, MOVES, sims)


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


def _table_by_loop(m, n):
    """The sequence of considered visits built by the plain list-extending loop (the paper's public implementation, restated)."""
    if m <= 1:
        return list(range(n))
    log2max = int(math.ceil(math.log2(m)))
    seq, visits, k = [], [0] * m, m
    while len(seq) < n:
        extra = max(1, int(n / (log2max * k)))
        for _ in range(extra):
            seq.extend(visits[:k])
            for i in range(k):
                visits[i] += 1
        k = max(2, k // 2)
    return seq[:n]


def test_schedule_against_the_list_built_table():
    for m in range(1, 33):
        for n in range(1, 129):
            want = _table_by_loop(m, n)
            got = [gb.considered_visit(m, n, t) for t in range(n)]
            assert got == want, (m, n)
            if m > 1:                                          # past the budget: the value of the last step
                assert gb.considered_visit(m, n, n + 3) == want[-1]
    assert gb.considered_visit(1, 8, 11) == 11


def test_host_draws_equal_the_definition_bit_for_bit():
    from transgo_amd import _lib
    lib = _lib.load()
    for seed in (0, 1, 500, 2 ** 32 - 1):
        rs = np.random.RandomState(seed)
        s = _lib.TgMt19937()
        lib.tg_host_mt_seed(ctypes.byref(s), ctypes.c_uint32(seed))
        for n in (1, 82, 362, 7, 311):                         # 311 + ... crosses the 624-word twist several times
            want = np.array(gb.draw(rs, n))
            got = np.zeros(n)
            lib.tg_host_mt_gumbel(ctypes.byref(s), n, got.ctypes.data_as(ctypes.c_void_p))
            assert want.tobytes() == got.tobytes(), (seed, n)
            key, pos = rs.get_state()[1], int(rs.get_state()[2])
            assert int(s.pos) == pos and np.array_equal(np.frombuffer(s.key, np.uint32), key), (seed, n)


def test_table_keeps_the_m_largest_ties_to_the_lower_action():
    g = [0.0, 1.0, 1.0, -1.0, 5.0]
    pri = [np.float32(1.0)] * 3 + [np.float32(0.0), np.float32(0.5)]
    assert gb.table(g, pri, 2) == [gb.NEG_INF, 1.0, gb.NEG_INF, gb.NEG_INF, 5.0 + math.log(0.5)]
    assert gb.table(g, pri, 9) == [0.0, 1.0, 1.0, gb.NEG_INF, 5.0 + math.log(0.5)]     # a prior of 0 is never considered
    assert gb.table(g, pri, 0) == [gb.NEG_INF] * 5


@pytest.mark.parametrize("name,seed", PAIRS)
def test_m0_is_the_oracle_search_move_for_move(name, seed):
    want, st = _plain_game(name, seed)
    got, o = _game(name, seed, 0)
    assert len(got) == len(want) == MOVES
    for m, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a["raw"], b["raw"]) and a["action"] == b["action"] and np.array_equal(a["pi"], b["pi"]) and a["pos"] == b["pos"], m
        assert not a["gumbel"]
    assert np.array_equal(o.rng.get_state()[1], st[1]) and o.rng.get_state()[2] == st[2]
    assert o.root_selections == 0


def test_m16_changes_the_search():
    """The condition on the inputs: for (sharp, 500) the searched root of the m = 16 search differs from the PUCT search's."""
    a, o = _game("sharp", 500, M)
    b, _ = _plain_game("sharp", 500)
    assert not np.array_equal(a[0]["raw"], b[0]["raw"])
    assert o.root_selections > 0


@pytest.mark.parametrize("name,seed", PAIRS)
def test_invariants_of_searched_roots(name, seed):
    got, o = _game(name, seed, M)
    for m, mv in enumerate(got):
        assert mv["gumbel"]
        cons = mv["gl"] > -np.inf
        m_eff = min(M, mv["nchild"])
        assert cons.sum() == m_eff
        assert (mv["effort"][~cons] == 0).all(), m            # only considered children gain visits in the move
        assert cons[mv["action"]] and mv["effort"][mv["action"]] == mv["effort"][cons].max(), m
        total = int(mv["effort"].sum())
        assert SIMS <= total < SIMS + 4
        assert abs(mv["pi"].sum() - 1.0) < 1e-12 and (mv["pi"] >= 0).all()


def test_effort_profile_is_the_schedules_without_drops():
    """One wave of one read-out never overshoots and never drops: the efforts after the budget replay the schedule exactly."""
    from oracle.go_oracle import OracleGoEnv
    from tests.gumbel_ref import GumbelOracleSearch
    rng = np.random.RandomState(7)
    o = GumbelOracleSearch(OracleGoEnv(), evaluators.sharp, rng, num_simulation=40, parallel_readouts=1, gumbel_m=8)
    _, _, _, info = o.search_move()
    assert o.fallback_selections == 0 and o.root_selections == 40
    eff = []
    for t in range(40):
        v = gb.considered_visit(8, 40, t)
        if v in eff:
            eff[eff.index(v)] += 1
        else:
            assert v == 0
            eff.append(1)
    assert sorted(eff) == sorted(int(x) for x in info["effort"] if x > 0)
    assert len(eff) == 8


def test_hand_built_root():
    """c_visit = 50, c_scale = 1, wu = 2, m = 2 over three children, budget 4: L = 1, x = max(1, 4 // 2) = 2, so the schedule is
    v = 0, 0, 1, 1.  gl = (0.5, -inf, 0.25); child 1 is not considered.  maxN = 3 (child 1's old visits count: maxN is absolute).
    t = 0: both considered children have e = 0 = v; score = gl + 53 * qhat: A: 0.5 + 53 * 0.0 = 0.5, C: 0.25 + 53 * 0.125 = 6.875
    -> C.  With C in flight (pending 2): e(C) = 1, t = 1, v = 0 -> A alone.  With both in flight t = 2, v = 1 -> both eligible again.
    A drop leaves e = (0, 0) at t = 3 (root pending 6 from another child's paths is impossible here, so build it by hand): v = 1,
    nobody has 1 -> fallback to the smallest effort."""
    f32 = np.float32
    gl = [0.5, gb.NEG_INF, 0.25]
    n0 = [0, 3, 0]
    kids = [(0, 0, f32(0.0)), (3, 0, f32(1.0)), (0, 0, f32(-0.125))]
    sc, el, fb = gb.select(gl, kids, n0, 3, 0, 3, 2, 2, 4, 50.0, 1.0)
    assert el == [0, 2] and not fb and sc[0] == 0.5 and sc[2] == 0.25 + 53.0 * 0.125 and sc[1] is None
    kids[2] = (0, 2, f32(-0.125))
    sc, el, fb = gb.select(gl, kids, n0, 3, 2, 3, 2, 2, 4, 50.0, 1.0)
    assert el == [0] and not fb
    kids[0] = (0, 2, f32(0.0))
    sc, el, fb = gb.select(gl, kids, n0, 3, 4, 3, 2, 2, 4, 50.0, 1.0)
    assert el == [0, 2] and not fb
    kids[0], kids[2] = (0, 0, f32(0.0)), (0, 0, f32(-0.125))
    sc, el, fb = gb.select(gl, kids, n0, 3, 6, 3, 2, 2, 4, 50.0, 1.0)
    assert el == [0, 2] and fb
    # the move: the considered children with the largest effort, then the score; ties to the lower action
    assert gb.pick_move(gl, [(2, f32(0.0)), (9, f32(9.0)), (2, f32(-0.3))], n0, 50.0, 1.0) == 2
    assert gb.pick_move(gl, [(3, f32(0.0)), (9, f32(9.0)), (2, f32(-3.0))], n0, 50.0, 1.0) == 0
    assert gb.pick_move([0.5, gb.NEG_INF, 0.5], [(2, f32(0.0)), (3, f32(0.0)), (2, f32(0.0))], n0, 50.0, 1.0) == 0
    assert gb.qhat(f32(1.0), 2) == float(f32(-1.0) / f32(3.0))


def test_fixed_point_target():
    """Each count / 2**24 is within 2**-25 of pi' (half a unit of the fixed point); the counts sum to within A of 2**24."""
    for name, seed in PAIRS:
        for mv in _game(name, seed, M)[0]:
            pi, cnt = mv["pi"], mv["record"]
            assert cnt.dtype == np.int32 and (cnt >= 0).all()
            assert np.abs(cnt / 2.0 ** 24 - pi).max() <= 2.0 ** -25
            assert abs(int(cnt.sum()) - 2 ** 24) <= 82
    assert gb.fixed_point(np.array([0.5 / 2 ** 24, 1.5 / 2 ** 24, 0.49 / 2 ** 24])).tolist() == [1, 2, 0]


def test_improved_policy_tables_equal_the_row_form():
    from oracle.go_oracle import OracleGoEnv
    from tests.gumbel_ref import GumbelOracleSearch
    rng = np.random.RandomState(500)
    o = GumbelOracleSearch(OracleGoEnv(), evaluators.sharp, rng, num_simulation=32, gumbel_m=8)
    _, pi, _, _ = o.search_move()
    A = 82
    t = dict(n=np.zeros((1, A), np.int32), w=np.zeros((1, A), np.float32), prior=np.zeros((1, A), np.float64), flags=np.zeros((1, A), np.uint8))
    for a, c in o.root.kids.items():
        t["n"][0, a], t["w"][0, a], t["prior"][0, a], t["flags"][0, a] = c.n, c.w, c.prior, 1
    assert np.array_equal(gb.improved_policy(t)[0], pi)
    assert not gb.improved_policy(t, games=[False]).any()


def test_config_and_binding():
    from transgo_amd import _lib
    from transgo_amd.configure import Config
    c = Config()
    assert (c.gumbel_m, c.gumbel_c_visit, c.gumbel_c_scale) == (0, 50.0, 1.0)
    assert Config(gumbel_m=16, gumbel_c_visit=40, gumbel_c_scale=0.5).gumbel_m == 16
    for bad in (-1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="gumbel_m"):
            Config(gumbel_m=bad)
    for bad in (float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="gumbel_c_visit"):
            Config(gumbel_c_visit=bad)
        with pytest.raises(ValueError, match="gumbel_c_scale"):
            Config(gumbel_c_scale=bad)
    with pytest.raises(ValueError, match="same root"):
        Config(gumbel_m=4, forced_playouts_k=2.0)
    for name, nargs in (("tg_sp_gumbel", 4), ("tg_sp_gumbel_get", 4), ("tg_sp_gumbel_move", 3), ("tg_sp_gumbel_target", 3),
                        ("tg_sp_gumbel_table", 2), ("tg_sp_gumbel_stats", 3), ("tg_host_mt_gumbel", 3)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
