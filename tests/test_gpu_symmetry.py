"""Symmetry-aware evaluation on the device (tg_net_set_symmetry, csrc/symmetry.hip) against the existing forward plus NumPy
(transgo_amd.symmetry): every comparison is np.array_equal -- the reference path runs the plain forward on the same rows in the
same batch places with the same rows_cap, and the modes are defined so that nothing else differs."""
import ctypes

import numpy as np
import pytest

from transgo_amd import symmetry

pytestmark = pytest.mark.gpu

# (name, board, planes, filters, blocks, precision, rows_cap, row counts).  65 rows with rows_cap 32 cross two chunk boundaries of
# tg_net_predict; 13 planes of 9x9 are 1053 bits, so a row straddles word 32; 10 planes of 19x19 are 113 words with a 26-bit
# tail.  The 19x19 tower is 1x128: the library builds no narrower network at that size (32 filters are refused at the load).
CASES = {
    "9x9c10": (9, 10, 32, 2, "f32", 32, (1, 7, 65)),
    "9x9c13": (9, 13, 32, 1, "f32", 16, (9,)),
    "19x19c10": (19, 10, 128, 1, "f32", 8, (5,)),
    "9x9f16": (9, 10, 128, 2, "f16", 16, (9,)),
}
POSITION_SEED = 2024


def _positions(S, C, n):
    if C == 10:
        from tests.test_net_reference import parity_positions
        return parity_positions(S, n - 2, 5)[:n] if n > 2 else parity_positions(S, 4, 5)[:n]
    from tests.test_symmetry_host import encoded_positions
    return encoded_positions(S, C, 40, seed=3)[40 - n:]               # mid-game positions, not the first plies


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    """Two networks with the same weights: `net` is switched between modes, `plain` never hears of the option."""
    from transgo_amd import model
    S, C, F, NB, prec, cap, counts = CASES[request.param]
    sd = model.random_weights(S, C, F, NB, seed=17)
    net = model.HipNetwork(S, C, F, NB, rows_cap=cap, precision=prec)
    plain = model.HipNetwork(S, C, F, NB, rows_cap=cap, precision=prec)
    net.set_weights(sd); plain.set_weights(sd)
    x = _positions(S, C, max(counts))
    assert x.shape == (max(counts), C, S, S)
    yield dict(S=S, net=net, plain=plain, x=x, counts=counts, name=request.param)
    net.ctx.close(); plain.ctx.close()


def _under(plain, x, s_rows, S):
    """The definition: each row transformed, ONE plain forward over the batch in its own row order, outputs mapped back."""
    xt = np.stack([symmetry.transform_planes(x[r], int(s_rows[r])) for r in range(len(x))])
    p, v, o = plain.main_prediction(xt)
    return (np.stack([symmetry.untransform_policy(p[r], int(s_rows[r]), S) for r in range(len(x))]), v,
            np.stack([symmetry.untransform_board(o[r], int(s_rows[r]), S) for r in range(len(x))]))


def _equal(got, want, what):
    for g, w, k in zip(got, want, ("policy", "value", "own")):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k)
        assert np.array_equal(g, w), f"{what}: {k} differs in {int((g != w).sum())} entries, max |d| {np.abs(g - w).max():.3e}"


def test_fixed_symmetry_is_transform_forward_backmap(case):
    S, net, plain = case["S"], case["net"], case["plain"]
    differs = False
    for n in case["counts"]:
        x = case["x"][:n]
        none = plain.main_prediction(x)
        for s in range(8):
            net.set_symmetry(s)
            assert net.get_symmetry() == (1, s)
            got = net.main_prediction(x)
            _equal(got, _under(plain, x, np.full(n, s), S), f"{case['name']} rows {n} s {s}")
            assert np.abs(got[0].sum(1) - 1).max() < 1e-5
            if s == symmetry.IDENTITY:
                _equal(got, none, "identity")
            elif not np.array_equal(got[0], none[0]):
                differs = True
        net.set_symmetry("none")
        _equal(net.main_prediction(x), none, "back to none")
    assert differs, "no symmetry changed any output: the positions or the weights are symmetric and the test shows nothing"


def test_position_symmetry_per_row(case):
    S, net, plain = case["S"], case["net"], case["plain"]
    for n in case["counts"]:
        x = case["x"][:n]
        s_rows = symmetry.position_symmetry(POSITION_SEED, symmetry.pack_planes(x))
        if n == 65:
            assert len(set(s_rows.tolist())) >= 3, np.bincount(s_rows, minlength=8)
        net.set_symmetry("position", POSITION_SEED)
        assert net.get_symmetry() == (2, POSITION_SEED)
        got = net.main_prediction(x)
        _equal(got, _under(plain, x, s_rows, S), f"{case['name']} rows {n} position")
        _equal(got, symmetry.evaluate_with_symmetry(plain.main_prediction, x, "position", POSITION_SEED), "host restatement")
        # the same position in another place of another batch gets the same orientation: evaluated under ITS s there too
        if n >= 7:
            net.set_symmetry("position", POSITION_SEED)
            back = net.main_prediction(np.ascontiguousarray(x[::-1]))
            _equal(back, _under(plain, np.ascontiguousarray(x[::-1]), s_rows[::-1], S), "reversed batch")
    net.set_symmetry("none")


def test_mean8_is_the_fixed_order_float32_mean(case):
    S, net, plain = case["S"], case["net"], case["plain"]
    for n in case["counts"]:
        x = case["x"][:n]
        acc = None
        for s in range(8):
            cur = _under(plain, x, np.full(n, s), S)
            acc = cur if acc is None else tuple(a + c for a, c in zip(acc, cur))
        want = tuple(a * np.float32(0.125) for a in acc)
        net.set_symmetry("mean8")
        assert net.get_symmetry() == (3, 0)
        got = net.main_prediction(x)
        _equal(got, want, f"{case['name']} rows {n} mean8")
        assert np.abs(got[0].sum(1) - 1).max() < 1e-5
    net.set_symmetry("none")


def test_refusals_leave_the_setting_and_the_context_alone():
    from transgo_amd import _lib, model
    from transgo_amd.engine import SelfPlayEngine
    net = model.HipNetwork(9, 10, 32, 2, rows_cap=8)
    net.set_symmetry("position", 77)                                  # legal before weights are loaded
    for mode, arg in ((4, 0), (-1, 0), (1, 8)):
        with pytest.raises(_lib.TransgoError) as e:
            net.ctx.call("tg_net_set_symmetry", mode, arg)
        assert "tg_net_set_symmetry" in str(e.value)
        assert net.get_symmetry() == (2, 77)
    with pytest.raises(ValueError):
        net.set_symmetry(8)
    net.ctx.close()
    sd = model.random_weights(9, 10, 32, 2, seed=5)
    eng = SelfPlayEngine(4, num_simulation=16, net_blocks=2, net_filters=32, eval_symmetry=3)
    model.load_into(eng.ctx, sd, 9, 10, 32, 2)
    assert eng.get_symmetry() == (1, 3)
    seeds = np.arange(4, dtype=np.uint32)
    eng.ctx.call("tg_sp_reset", seeds.ctypes.data_as(ctypes.c_void_p), None)         # leaves a root batch pending
    with pytest.raises(_lib.TransgoError) as e:
        eng.set_symmetry("mean8")
    assert "pending" in str(e.value) and eng.get_symmetry() == (1, 3)
    eng.ctx.call("tg_sp_eval"); eng.ctx.call("tg_sp_expand_roots")
    eng.set_symmetry("mean8")                                          # at the move boundary it is taken
    assert eng.get_symmetry() == (3, 0)
    eng.search()
    assert (eng.root_visits()[0].sum(1) >= 15).all()
    eng.close()


def _play(eng, moves):
    """Per move: root visit table, chosen moves, and every game's MT19937 stream after the move."""
    out = []
    for _ in range(moves):
        eng.search()
        vis, st = eng.root_visits()
        acts, _ = eng.choose_moves(vis, st)
        eng.play(acts)
        out.append((vis.copy(), acts.copy(), eng.rng_streams().copy()))
    return out


@pytest.mark.parametrize("mode,sims", [("position", 32), ("mean8", 16)])
def test_engine_device_mode_equals_host_wrapper(mode, sims):
    """Engine A evaluates on the device under the mode; engine B has no device mode: its host evaluator hands tg_sp_batch_obs's rows
    to a HipNetwork of the same weights and rows_cap through symmetry.evaluate_with_symmetry; engine C lets SelfPlayEngine wrap a
    plain host evaluator itself.  Same visits, same moves, same random streams after each move."""
    from transgo_amd import model
    from transgo_amd.engine import SelfPlayEngine
    G, R, seed = 8, 4, 11
    sd = model.random_weights(9, 10, 32, 2, seed=23)
    kw = dict(num_simulation=sims, parallel_readouts=R, net_blocks=2, net_filters=32)
    a = SelfPlayEngine(G, eval_symmetry=mode, symmetry_seed=seed, **kw)
    model.load_into(a.ctx, sd, 9, 10, 32, 2)
    hn = model.HipNetwork(9, 10, 32, 2, rows_cap=G * R)
    hn.set_weights(sd)
    calls = []

    def wrapped(obs):
        calls.append(len(obs))
        return symmetry.evaluate_with_symmetry(lambda o: hn.main_prediction(o)[:2], obs, mode, seed)
    b = SelfPlayEngine(G, evaluator=wrapped, **kw)
    c = SelfPlayEngine(G, evaluator=lambda o: hn.main_prediction(o)[:2], eval_symmetry=mode, symmetry_seed=seed, **kw)
    assert b.get_symmetry() == (0, 0) and a.get_symmetry()[0] == c.get_symmetry()[0] == symmetry.MODES[mode]
    logs = []
    for eng in (a, b, c):
        eng.reset(np.arange(G) + 100)
        logs.append(_play(eng, 2))
    assert calls and hn.get_symmetry() == (0, 0) and hn.symmetry_staging_bytes() == 0
    for other, who in ((logs[1], "explicit host wrapper"), (logs[2], "engine-wrapped host evaluator")):
        for m, (x, y) in enumerate(zip(logs[0], other)):
            assert np.array_equal(x[0], y[0]), f"{who}: visit counts differ at move {m}"
            assert np.array_equal(x[1], y[1]), f"{who}: chosen moves differ at move {m}"
            assert np.array_equal(x[2], y[2]), f"{who}: random streams differ at move {m}"
    n = ctypes.c_uint64()
    a.ctx.call("tg_net_symmetry_staging", ctypes.byref(n))
    assert n.value > 0
    for eng in (a, b, c):
        eng.close()
    hn.ctx.close()


def test_mode_none_is_inert():
    """An engine created with eval_symmetry="none" and one that never heard of the option: the same stats(), visit counts and
    snapshot, and no staging buffer.  The snapshot is compared as tests/test_gpu_snapshot.py compares two runs of the same games --
    every section but the chunk ids, which depend on the order the games' workgroups reach the pool in any two runs."""
    from tests.test_gpu_snapshot import EXACT_SECTIONS, _exact_sections
    from transgo_amd import model
    from transgo_amd.engine import SelfPlayEngine
    sd = model.random_weights(9, 10, 32, 2, seed=23)
    kw = dict(num_simulation=32, parallel_readouts=4, net_blocks=2, net_filters=32)
    engines = [SelfPlayEngine(8, eval_symmetry="none", **kw), SelfPlayEngine(8, **kw)]
    res = []
    for eng in engines:
        model.load_into(eng.ctx, sd, 9, 10, 32, 2)
        eng.reset(np.arange(8) + 100)
        log = _play(eng, 2)
        n = ctypes.c_uint64()
        eng.ctx.call("tg_net_symmetry_staging", ctypes.byref(n))
        assert n.value == 0 and eng.get_symmetry() == (0, 0)
        res.append((log, eng.stats(), _exact_sections(eng)[0], eng.snapshot().size))
    for m, (x, y) in enumerate(zip(res[0][0], res[1][0])):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), m
    assert res[0][1] == res[1][1] and res[0][3] == res[1][3]
    for k in EXACT_SECTIONS:
        assert res[0][2][k] == res[1][2][k], k
    for eng in engines:
        eng.close()


def test_symmetry_spread():
    """The eight inputs of the empty board are one and the same, so its value spread is exactly 0 and its policy spread is the
    asymmetry of the one policy the network gives it (random weights are not equivariant, so that is not 0: the eight back-maps
    permute one asymmetric vector).  An asymmetric position spreads in both."""
    from transgo_amd import analysis, model
    from transgo_amd.environment import GoEnv
    env = GoEnv(board_size=9)
    empty = env.reset_batch(1)
    st = empty.copy()
    for a in (40, 20, 60, 3, 71):
        st, done, ok = env.step_batch(st, [a])
        assert ok.all() and not done.any()
    net = model.HipNetwork(9, 10, 32, 2, rows_cap=8)
    net.set_weights(model.random_weights(9, 10, 32, 2, seed=17))
    net.set_symmetry("position", 3)
    sp = analysis.symmetry_spread(net, np.concatenate([empty, st]))
    assert net.get_symmetry() == (2, 3)                                # the network's own mode is put back
    net.set_symmetry("none")
    obs = env.query_batch(np.concatenate([empty, st]), obs=True)["obs"]
    assert not obs[0].any()
    p = net.main_prediction(obs)[0]
    backs = np.stack([symmetry.untransform_policy(p[0], s, 9) for s in range(8)])
    assert sp[0]["value"] == 0.0
    assert sp[0]["policy"] == float((backs.max(0) - backs.min(0)).max())
    assert sp[1]["policy"] > 0 and sp[1]["value"] > 0
    assert analysis.symmetry_spread(net, empty[:0]) == []
    net.ctx.close(); env.ctx.close()
