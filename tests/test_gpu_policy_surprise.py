"""Policy surprise weighting on the device (csrc/policy_surprise.hip) against the restatement
(transgo_amd/policy_surprise.py through tests/policy_surprise_ref.py): the kernels on synthetic games with host priors, the gather
byte for byte, the network's prior rows, the untouched search, the refusals.  Small towers (2 blocks x 32 filters) or host priors
throughout; the engine runs and the plain harvests they are compared with are computed once and shared."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import evaluators
from tests import policy_surprise_ref as ref

EV = evaluators.sharp
LAM, PSW_SEED = 0.5, 21


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# ---- kernel level: synthetic counts, host priors, no network ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rules_context(S):
    from transgo_amd import _lib
    cfg = _lib.default_config()
    cfg.board_size, cfg.n_games = S, 0
    return _lib.Context(cfg)


def _device_plan(fx):
    ctx = _rules_context(fx["S"])
    nm, n = fx["n_moves"], int(fx["n_moves"].sum())
    r = dict(n_moves=np.full(len(nm), -1, np.int32), surprise=np.full(n, -1.0), weight=np.full(n, -1.0), copies=np.full(n, -1, np.int32),
             src=np.full(2 * n + 1, -1, np.int32))
    n_out = ctypes.c_int32(-1)
    ctx.call("tg_policy_surprise_plan_arrays", len(nm), _ptr(nm), _ptr(fx["seeds"]), _ptr(np.ascontiguousarray(fx["counts"], np.int32)),
             _ptr(np.ascontiguousarray(fx["prior"], np.float32)), ctypes.c_double(fx["lam"]), fx["seed"], ctypes.byref(n_out),
             _ptr(r["n_moves"]), _ptr(r["surprise"]), _ptr(r["weight"]), _ptr(r["copies"]), _ptr(r["src"]), len(r["src"]))
    r["n_out"] = n_out.value
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("S,lam", ref.KERNEL_CASES)
def test_kernels_against_the_restatement(S, lam):
    """k_psw_surprise and k_psw_plan at 9x9 and 19x19 (A = 82 / 362: a partial last stripe), T = 0, 1 and 40, rows with 1s, a row
    with n = 0, priors with exact zeros, lambda 0.5 and 1.0.  surprise to 1e-12 * sum|term| + 1e-300 per position (at most 362 terms,
    each a few f64 ulp off), weight to 1e-11 relative, copies / n_out / n_moves / the source rows exact."""
    fx = ref.kernel_fixture(S, lam)
    want, got = ref.reference_plan(fx), _device_plan(fx)
    assert ref.margin(want) > ref.MARGIN
    bound = 1e-12 * ref.abs_terms(fx["counts"], fx["prior"]) + 1e-300
    err = np.abs(got["surprise"] - want["surprise"])
    print(f"S {S} lambda {lam}: largest surprise error / bound {float((err / bound).max()):.3e}, "
          f"largest relative weight error {float((np.abs(got['weight'] - want['weight']) / np.maximum(want['weight'], 1e-300)).max()):.3e}")
    assert (err <= bound).all(), float((err / bound).max())
    assert (got["surprise"] >= 0).all() and (got["surprise"][want["surprise"] == 0.0] == 0.0).all()
    assert (np.abs(got["weight"] - want["weight"]) <= 1e-11 * np.abs(want["weight"])).all()
    assert np.array_equal(got["copies"], want["copies"])
    assert got["n_out"] == want["n_out"] and np.array_equal(got["n_moves"], want["n_moves"])
    assert np.array_equal(got["src"][:got["n_out"]], want["src"]) and (got["src"][got["n_out"]:] == -1).all()


@pytest.mark.gpu
def test_plan_over_more_games_than_one_block_of_threads():
    """The scan's carry from one block of 1024 games to the next: 2500 games of 0..3 positions."""
    rs = np.random.RandomState(8)
    g = 2500
    nm = rs.randint(0, 4, g).astype(np.int32)
    n, A = int(nm.sum()), 82
    counts = rs.randint(0, 30, (n, A)).astype(np.int32) * (rs.rand(n, A) < 0.1)
    prior = rs.rand(n, A).astype(np.float32); prior /= prior.sum(axis=1, keepdims=True)
    fx = dict(S=9, A=A, lam=0.5, seed=5, n_moves=nm, seeds=rs.randint(0, 2 ** 32, g, dtype=np.uint64).astype(np.uint32),
              counts=counts.astype(np.int32), prior=prior)
    want, got = ref.reference_plan(fx), _device_plan(fx)
    assert ref.margin(want) > ref.MARGIN
    assert np.array_equal(got["copies"], want["copies"]) and np.array_equal(got["n_moves"], want["n_moves"])
    assert got["n_out"] == want["n_out"] and np.array_equal(got["src"][:got["n_out"]], want["src"])


# ---- the gather: host evaluator, host priors ------------------------------------------------------------------------------------
G1, MAX1 = 6, 9
SEEDS1 = np.arange(40, 40 + G1).astype(np.uint32)


def _play_to_the_end(eng, seeds):
    eng.reset(seeds)
    while not eng.finished.all():
        eng.search()
        vis, st = eng.root_visits()
        acts, _ = eng.choose_moves(vis, st)
        done = eng.play(acts)
        if done.any():
            return done
    raise AssertionError("no game finished")


@functools.lru_cache(maxsize=None)
def _gather_run():
    """Six games with a host evaluator played until the first of them end: the plain harvest, then -- of the same finished games
    -- the resampled one to host arrays, to device memory, and the plan's read-outs with the caller's prior rows."""
    from transgo_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine(G1, num_simulation=40, max_step=MAX1, evaluator=EV)
    _play_to_the_end(eng, SEEDS1)
    plain = eng.harvest(device=False, seeds=SEEDS1)
    prior = np.ascontiguousarray(EV(plain.observations())[0], np.float32)
    eng.set_policy_surprise(LAM, PSW_SEED)
    host = eng.harvest(device=False, seeds=SEEDS1)
    dev = eng.harvest(device=True, seeds=SEEDS1)
    on_device, dev = dev.on_device, dev.to_host()
    read = eng.policy_surprise_plan(SEEDS1, prior, readout=True)
    stats = eng.policy_surprise_stats()
    eng.set_policy_surprise(0.0)
    again = eng.harvest(device=False, seeds=SEEDS1)
    eng.close()
    return dict(plain=plain, prior=prior, host=host, dev=dev, on_device=on_device, read=read, stats=stats, again=again)


@pytest.mark.gpu
def test_gather_is_byte_identical_to_the_restatement_host_and_device():
    r = _gather_run()
    plain = r["plain"]
    assert plain.n_games >= 2 and plain.n_positions > 8
    want, plan = ref.resample(plain, r["prior"], LAM, PSW_SEED)
    assert (plan["copies"] == 0).any() and (plan["copies"] >= 2).any()
    assert r["on_device"]
    for name, got in (("host", r["host"]), ("device", r["dev"])):
        assert (got.n_games, got.n_positions) == (want.n_games, want.n_positions), name
        for k in want.sec:
            assert np.array_equal(got.view(k), want.view(k)), (name, k)
        assert got.buf.tobytes() == want.buf.tobytes(), name           # the padding bytes too
    read = r["read"]
    assert read["n_out"] == plan["n_out"] and np.array_equal(read["copies"], plan["copies"])
    assert np.array_equal(read["prior"], r["prior"])
    assert (np.abs(read["weight"] - plan["weight"]) <= 1e-11 * plan["weight"]).all()
    assert r["stats"]["plans"] == 3 and r["stats"]["rows_forwarded"] == 0
    assert r["stats"]["positions_in"] == 3 * plain.n_positions and r["stats"]["positions_out"] == 3 * plan["n_out"]
    assert r["again"].buf.tobytes() == plain.buf.tobytes()              # weight 0 again: today's harvest


# ---- the network's prior ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights():
    from transgo_amd import model
    return model.random_weights(9, 10, 32, 2, seed=5)


@functools.lru_cache(maxsize=None)
def _reference_net():
    from transgo_amd import model
    h = model.HipNetwork(9, 10, 32, 2, rows_cap=64)
    h.set_weights(_weights())
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["position", "cache"])
def test_network_prior_is_the_plain_forward_chunked_past_symmetry_and_cache(mode):
    """rows_cap = 2 games x 4 readouts = 8 with more than 8 harvested positions: the forward runs in chunks; once under
    eval_symmetry "position", once with an evaluation cache.  prior_out is bit-identical to tg_net_predict (identity orientation) on
    the plain harvest's observations; neither the cache's counters nor tg_sp_stats' evals move."""
    from transgo_amd import model
    from transgo_amd.engine import SelfPlayEngine
    seeds = np.array([3, 4], np.uint32)
    kw = dict(eval_symmetry="position", symmetry_seed=77) if mode == "position" else dict(eval_cache_entries=4096)
    eng = SelfPlayEngine(2, num_simulation=24, max_step=8, net_blocks=2, net_filters=32, **kw)
    model.load_into(eng.ctx, _weights(), 9, 10, 32, 2)
    done = _play_to_the_end(eng, seeds)
    plain = eng.harvest(device=False, seeds=seeds)
    assert plain.n_positions > 8 and done.any()
    eng.set_policy_surprise(LAM, PSW_SEED)
    st0, c0 = eng.stats(), eng.eval_cache_stats()
    read = eng.policy_surprise_plan(seeds, None, readout=True)
    st1, c1 = eng.stats(), eng.eval_cache_stats()
    assert st1["evals"] == st0["evals"] and st1["sims"] == st0["sims"] and c1 == c0
    if mode == "cache":
        assert c0["lookups"] > 0
    want_prior = _reference_net().main_prediction(plain.observations())[0]
    assert read["prior"].tobytes() == want_prior.tobytes()
    ps = eng.policy_surprise_stats()
    assert ps["rows_forwarded"] == plain.n_positions and ps["games"] == plain.n_games
    want, plan = ref.resample(plain, want_prior, LAM, PSW_SEED)
    assert read["n_out"] == plan["n_out"] and np.array_equal(read["copies"], plan["copies"])
    got = eng.harvest(device=False, seeds=seeds)
    assert got.buf.tobytes() == want.buf.tobytes()
    eng.close()


# ---- the search is untouched -------------------------------------------------------------------------------------------------------
def _selfplay_run(weight, p_full):
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    cap = dict(playout_cap_p_full=p_full, playout_cap_fast=8, playout_cap_seed=2) if p_full < 1.0 else {}
    cfg = Config(num_simulation=24, max_step=12, num_features=32, num_blocks=2, policy_surprise_weight=weight,
                 policy_surprise_seed=PSW_SEED, **cap)
    sp = BatchedSelfPlay(cfg, 16, seed_fn=lambda g, k: 500 + 100 * k + g)
    sp.set_weights(_weights())
    trace, harvests = [], []
    for _ in range(15):                                                # past the end of the first generation
        h = sp.advance()
        eng = sp.engine
        trace.append((eng.root_visits()[0].tobytes(), eng.root_states().tobytes(), eng.rng_streams().tobytes(), sp.seeds.tobytes()))
        if h is not None:
            harvests.append(h)
    stats = sp.engine.stats()
    sp.engine.close()
    return trace, harvests, stats


@pytest.mark.gpu
@pytest.mark.parametrize("p_full", [1.0, 0.5])
def test_search_untouched_and_harvests_are_the_restatement_of_the_plain_ones(p_full):
    """Two BatchedSelfPlay runs with the same seeds, 16 games at 9x9, 24 simulations, max_step 12, weight 0.5 against 0: every root
    position, root visit table and RNG stream identical after every move through to the end (so every move is), and the on-run's
    harvests are the restatement applied to the off-run's.  Once more with playout_cap_p_full = 0.5: games with few or no recorded
    positions."""
    off_trace, off_h, off_st = _selfplay_run(0.0, p_full)
    on_trace, on_h, on_st = _selfplay_run(LAM, p_full)
    assert on_trace == off_trace
    assert on_st["sims"] == off_st["sims"] and on_st["evals"] == off_st["evals"]
    assert len(on_h) == len(off_h) >= 1 and sum(h.n_games for h in off_h) >= 16
    changed = 0
    for a, b in zip(on_h, off_h):
        prior = _reference_net().main_prediction(b.observations())[0] if b.n_positions else np.zeros((0, 82), np.float32)
        want, plan = ref.resample(b, prior, LAM, PSW_SEED)
        assert a.to_host().buf.tobytes() == want.buf.tobytes()
        changed += int((plan["copies"] != 1).sum())
    assert changed > 0
    if p_full < 1.0:
        nm = np.concatenate([h.view("n_moves") for h in off_h])
        assert (nm < 6).any()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_name_what_is_wrong():
    from transgo_amd import _lib
    from transgo_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine(2, num_simulation=12, max_step=3, evaluator=EV)
    for bad in (-0.25, 1.5, float("nan")):
        with pytest.raises(_lib.TransgoError, match=r"weight must lie in \[0, 1\]"):
            eng.ctx.call("tg_sp_policy_surprise", ctypes.c_double(bad), 0)
    with pytest.raises(ValueError, match="policy_surprise_weight"):
        eng.set_policy_surprise(2.0)
    assert eng.get_policy_surprise() == (0.0, 0)
    seeds = np.array([1, 2], np.uint32)
    with pytest.raises(_lib.TransgoError, match="weighting is off"):
        eng.policy_surprise_plan(seeds, np.zeros((0, 82), np.float32))
    eng.set_policy_surprise(0.5, 3)
    assert eng.get_policy_surprise() == (0.5, 3)
    _play_to_the_end(eng, seeds)
    ng, npos = ctypes.c_int32(), ctypes.c_int32()
    eng.ctx.call("tg_sp_finished", ctypes.byref(ng), ctypes.byref(npos))
    assert ng.value > 0
    buf = [np.zeros(4 * 2 * npos.value * 400 + 64, np.uint8) for _ in range(5)]
    harvest = lambda: eng.ctx.call("tg_sp_policy_surprise_harvest", *[_ptr(b) for b in buf], 0, None, None, None, None, None)
    with pytest.raises(_lib.TransgoError, match="no plan is current"):
        harvest()
    with pytest.raises(_lib.TransgoError, match="no network weights are loaded"):
        eng.policy_surprise_plan(seeds, None)                           # prior = NULL without a network
    with pytest.raises(ValueError, match="seeds"):
        eng.harvest(device=False)
    prior = np.full((npos.value, 82), 1.0 / 82, np.float32)
    assert eng.policy_surprise_plan(seeds, prior) >= 0
    harvest()                                                           # a current plan: accepted
    eng.reset(seeds, np.ones(2, np.uint8))                             # the finished games are gone, and the plan with them
    with pytest.raises(_lib.TransgoError, match="no plan is current"):
        harvest()
    eng.close()
