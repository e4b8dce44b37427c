"""Policy surprise weighting, the host side: the restatement (transgo_amd.policy_surprise), its draw against tg_host_cap_draw, the
statistics of the copies, the margin condition on the fixtures of the GPU tests, and the Config refusals.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import policy_surprise_ref as ref
from transgo_amd import _lib, playout_cap
from transgo_amd import policy_surprise as psw
from transgo_amd.configure import Config


def test_weights_of_a_game_sum_to_its_length():
    rs = np.random.RandomState(3)
    for T in (1, 2, 5, 40, 120, 361):
        for lam in (0.25, 0.5, 1.0):
            s = rs.rand(T) * rs.choice([0.0, 1.0, 5.0], T)
            if not s.any():
                s[0] = 0.3
            w = psw.weights(s, lam)
            assert w.shape == (T,) and (w >= 1.0 - lam - 1e-15).all()
            assert abs(float(w.sum()) - T) <= 1e-12 * T, (T, lam, float(w.sum()) - T)


def test_weights_are_one_when_the_surprises_are_equal_or_all_zero():
    for T in (1, 3, 40):
        for lam in (0.5, 1.0):
            assert np.array_equal(psw.weights(np.zeros(T), lam), np.ones(T))
            w = psw.weights(np.full(T, 0.37), lam)
            assert np.abs(w - 1.0).max() <= 1e-12
    assert psw.weights(np.zeros(0), 0.5).shape == (0,)


def test_one_surprising_position_takes_the_whole_game_with_lambda_one():
    T = 12
    for eps in (1e-3, 1e-9, 0.0):
        s = np.full(T, eps); s[4] = 2.0
        w = psw.weights(s, 1.0)
        want = np.zeros(T); want[4] = T
        assert np.abs(w - want).max() <= T * T * eps / 2.0 + 1e-12, (eps, w)
    half = psw.weights(np.eye(1, T, 4)[0], 0.5)                        # KataGo's lambda: everybody keeps half
    assert half[4] == 0.5 + 0.5 * T and np.array_equal(np.delete(half, 4), np.full(T - 1, 0.5))


def test_surprise_is_the_kl_divergence_with_the_reference_rules():
    A = 82
    c = np.zeros(A, np.int32); c[[3, 10, 81]] = [6, 1, 2]              # the 1 is dropped: n = 8
    p = np.full(A, 1.0 / A, np.float32)
    want = 0.75 * (np.log(0.75) - np.log(float(p[3]))) + 0.25 * (np.log(0.25) - np.log(float(p[81])))
    assert abs(psw.surprise(c[None], p[None])[0] - want) <= 1e-15
    assert psw.surprise((c == 1).astype(np.int32)[None] * 1, p[None])[0] == 0.0       # n = 0
    q = p.copy(); q[3] = 0.0                                           # the floor: log(FLT_MIN), not -inf; no renormalisation
    got = psw.surprise(c[None], q[None])[0]
    assert np.isfinite(got) and abs(got - (0.75 * (np.log(0.75) - np.log(psw.FLT_MIN)) + 0.25 * (np.log(0.25) - np.log(float(p[81]))))) <= 1e-13
    same = np.zeros(A, np.float32); same[3], same[81] = 0.75, 0.25     # pi == p on the support: KL = 0, never below
    assert psw.surprise(c[None], same[None])[0] == 0.0
    big = np.zeros(A, np.float32); big[3], big[81] = 3.0, 1.0          # an unnormalised "prior" above pi: the sum is negative -> 0
    assert psw.surprise(c[None], big[None])[0] == 0.0


def test_the_draw_is_tg_host_cap_draw_with_the_domain_xored_seed():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.tg_host_cap_draw.restype = ctypes.c_uint32
    lib.tg_host_cap_draw.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32]
    assert psw.DOMAIN == 0x50535731
    rs = np.random.RandomState(5)
    for _ in range(200):
        gs, seed, T = int(rs.randint(0, 2 ** 32, dtype=np.uint64)), int(rs.randint(0, 2 ** 32, dtype=np.uint64)), int(rs.randint(1, 50))
        u = psw.uniforms(gs, T, seed)
        want = [lib.tg_host_cap_draw(gs, t, seed ^ 0x50535731) / 2.0 ** 24 for t in range(T)]
        assert u.dtype == np.float64 and list(u) == want and (u >= 0).all() and (u < 1).all()
    # another domain than the playout cap's own draws under the same seed
    assert not np.array_equal(psw.uniforms(11, 32, 0) * 2 ** 24, playout_cap.draw(11, np.arange(32), 0))


def test_mean_copies_over_seeds_is_the_weight():
    """4096 seeds: the copies of a position are floor(w) + Bernoulli(frac(w)), so their mean lies within 4 standard errors of w."""
    fx = ref.kernel_fixture(9, 0.5)
    s = psw.surprise(fx["counts"][1:41], fx["prior"][1:41])            # the game of 40
    w = psw.weights(s, 0.5)
    N = 4096
    k = np.stack([np.floor(w + psw.uniforms(gs, 40, 3)) for gs in range(N)])
    frac = w - np.floor(w)
    se = np.sqrt(frac * (1 - frac) / N)
    err = np.abs(k.mean(axis=0) - w)
    print("largest |mean - w| / standard error:", float((err / np.maximum(se, 1e-300)).max()))
    assert (err <= 4 * se + 1e-12).all(), (err / np.maximum(se, 1e-300)).max()
    assert abs(k.sum(axis=1).mean() - 40) <= 4 * np.sqrt((se ** 2).sum() * N) / np.sqrt(N)       # a game keeps its size on average


@pytest.mark.parametrize("S,lam", ref.KERNEL_CASES)
def test_margin_condition_and_coverage_of_the_kernel_fixtures(S, lam):
    """The condition on the inputs of the GPU kernel tests, checked with the reference alone: no w + u within 1e-9 of an integer
    (two f64 logs may differ by a few ulp, w then by about 1e-13), and the cases the fixtures are there for do occur."""
    fx = ref.kernel_fixture(S, lam)
    p = ref.reference_plan(fx)
    print(f"S {S} lambda {lam}: margin {ref.margin(p):.3e}, copies histogram {np.bincount(p['copies'])}")
    assert ref.margin(p) > ref.MARGIN
    nm = fx["n_moves"]
    assert {0, 1, 40} <= set(int(x) for x in nm)
    c = np.where(fx["counts"] == 1, 0, fx["counts"])
    assert (fx["counts"] == 1).any() and (c.sum(axis=1) == 0).any()    # rows with 1s; rows with n = 0
    assert ((fx["prior"] == 0.0) & (c > 0)).any()                      # the floor is met
    assert (p["copies"] == 0).any() and (p["copies"] >= 2).any()
    assert p["n_out"] == int(p["copies"].sum()) == len(p["src"]) and int(p["n_moves"].sum()) == p["n_out"]
    o = np.cumsum(nm) - nm
    for g, T in enumerate(nm):
        w = p["weight"][o[g]:o[g] + T]
        assert abs(float(w.sum()) - T) <= 1e-12 * max(int(T), 1)
    assert np.array_equal(p["weight"][o[5]:o[5] + 3], np.ones(3))      # the game without a twice-visited move


def test_resample_keeps_games_and_order_and_replaces_only_the_lengths():
    from transgo_amd import records
    fx = ref.kernel_fixture(9, 1.0)
    n, g = int(fx["n_moves"].sum()), len(fx["n_moves"])
    rs = np.random.RandomState(2)
    h = records.from_arrays(9, 10, fx["n_moves"], rs.randint(1, 3, g), rs.randint(-1, 2, (g, 81)), rs.randint(0, 2 ** 32, (n, 26), dtype=np.uint64),
                            fx["counts"], rs.choice([-1.0, 1.0], n), rs.randint(-1, 2, (n, 81)), rs.randint(1, 3, n),
                            slot=np.arange(g), seed=fx["seeds"], score=rs.randn(g))
    out, p = ref.resample(h, fx["prior"], 1.0, fx["seed"])
    assert out.n_games == g and out.n_positions == p["n_out"] and np.array_equal(out.view("n_moves"), p["n_moves"])
    for k in ("winner", "slot", "seed", "score", "terr"):
        assert np.array_equal(out.view(k), h.view(k)), k
    assert (np.diff(p["src"]) >= 0).all()
    for k in ("obs_bits", "counts", "z", "own", "player"):
        assert np.array_equal(out.view(k), h.view(k)[p["src"]]), k
    # lambda = 0 is the identity plan
    same, p0 = psw.resample(h, fx["prior"], 0.0, fx["seed"])
    assert np.array_equal(p0["copies"], np.ones(n, np.int32)) and np.array_equal(same.buf, h.buf)


def test_config_defaults_and_refusals():
    c = Config()
    assert (c.policy_surprise_weight, c.policy_surprise_seed) == (0.0, 0) and not psw.enabled(c)
    assert psw.enabled(Config(policy_surprise_weight=0.5, policy_surprise_seed=9))
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="policy_surprise_weight"):
            Config(policy_surprise_weight=bad)
    for bad in (-1, 2 ** 32, 0.5, "3"):
        with pytest.raises(ValueError, match="policy_surprise_seed"):
            Config(policy_surprise_weight=0.5, policy_surprise_seed=bad)
    late = Config()
    late.policy_surprise_weight = 2.0
    with pytest.raises(ValueError, match="policy_surprise_weight"):
        psw.check_config(late)
