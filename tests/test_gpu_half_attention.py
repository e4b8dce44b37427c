"""fp16-storage network ("f16", net_precision 1) with Self_Attention at 9x9, F = 128: the fused k_attention_h and its plumbing
(weight image staged at the synchronous load and at the background refresh, act16 hand-off to the next residual block and to the
head conv, the PRO variant of the policy head, the range guard, the refusals), against the float64 emulation of the chain's
rounding points (tests/half_attention_ref.py; tests/test_half_attention_reference.py pins it and the tolerances on the CPU).

Short archs are the smallest shapes at which each code path can be wrong: "A" (attention after the stem; its act16 carries the tail
BN for k_head_h), "AR" (act16 with the next block's bn1), "AA" (no act16 between the two), "RA+P" (PRO, which needs the last
block's f32 stream).  Batches of 1, 7 and 2179 boards (more than 256 workgroups x 4 waves: every wave walks several boards), after
a prefill forward on other positions; rows 0-6 of the big batch bit-identical to the 7-row batch.

Measured on an MI355X, max logit-space error against the float64 emulation over the three batch sizes (tolerance in brackets; the
emulation itself moves by the sensitivities listed in the CPU file under another summation order):
    A 8.8e-5, AR 7.9e-4, AA 2.8e-4, RA+P 1.7e-4 (2e-3); MainNetwork 2.05e-3 at n = 300 and at n = 2179 (6e-3).
    MainNetwork with random_transgo_weights against the torch f32 module: 5.3e-5 absolute (1e-3).
    Negative control (one value_conv channel zeroed in the HIP network only): 3.2e-1."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BIG = 2179


def _tol(code):
    from tests.test_half_attention_reference import tolerance
    return tolerance(code)


def _net(code, sd, rows_cap, precision="f16", S=9, F=128):
    from tests.half_attention_ref import arch_of
    from transgo_amd.model import HipNetwork
    h = HipNetwork(S, 10, F, rows_cap=rows_cap, arch=arch_of(code), precision=precision)
    h.set_weights(sd)
    return h


def _batch(s, n, seed):
    """n rows: the K + 2 checked positions first (rows 0 .. K+1), then a seeded draw of them; the last row the all-edges board."""
    k = s["x"].shape[0]
    ids = np.concatenate([np.arange(k), np.random.RandomState(seed).randint(0, k, max(0, n - k))])[:n]
    ids[n - 1] = k - 1 if n > k else ids[n - 1]
    return ids


def _check(h, s, n, label, tol, expect_fail=False):
    """Prefill on other positions, the checked forward of n rows; copies of a position identical, the distinct positions within tol
    of the float64 emulation.  Returns (error, outputs)."""
    from oracle.net import parity_error
    x, alt = s["x"], s["alt"]
    k = x.shape[0]
    ids = _batch(s, n, n)
    before = h.main_prediction(alt[np.random.RandomState(n + 1).randint(0, alt.shape[0], n)])
    got = h.main_prediction(x[ids])
    first = np.array([int(np.flatnonzero(ids == i)[0]) if (ids == i).any() else -1 for i in range(k)])
    have = first >= 0
    for a, b in zip(got, before):
        assert np.array_equal(a, a[first[ids]]), f"{label}: copies of one position differ"
        assert not np.array_equal(a, b)
    err, per = parity_error([a[first[have]] for a in got], [r[have] for r in s["ref"]])
    print(f"\n{label}: max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} own {per[2]:.1e}), tolerance {tol:.0e}")
    if expect_fail:
        assert err > tol, f"{label}: the comparator did not flag the mutated weights"
    else:
        assert err < tol, label
    return err, got


@pytest.mark.parametrize("code", ["A", "AR", "AA", "RA+P"])
def test_short_archs_against_the_float64_emulation(code):
    from tests.half_attention_ref import setup, state_dict_np
    s = setup(code)
    tol = _tol(code)
    h = _net(code, state_dict_np(s["net"]), BIG)
    try:
        _, one = _check(h, s, 1, f"{code} n=1", tol)
        _, seven = _check(h, s, 7, f"{code} n=7", tol)
        _, big = _check(h, s, BIG, f"{code} n={BIG}", tol)
        for a, b, c in zip(one, seven, big):
            assert np.array_equal(a, b[:1]) and np.array_equal(b, c[:7]), f"{code}: a board's result depends on its batch"
        assert h.net_range()["fp16_overflows"] == 0
    finally:
        h.ctx.close()


def test_mainnetwork_against_the_float64_emulation():
    """The shipped arch with parity_transgo weights, n = 300 and n = 2179, under FULL_TOL = 6e-3 (CPU file: 2.3 x the emulation's own
    sensitivity 2.35e-3).  Measured on an MI355X: 2.05e-3 at both sizes (9.9e-4 on the first seven rows)."""
    from tests.half_attention_ref import FULL, setup, state_dict_np
    from tests.test_half_attention_reference import FULL_TOL
    s = setup(FULL)
    h = _net(FULL, state_dict_np(s["net"]), BIG)
    try:
        _, seven = _check(h, s, 7, "MainNetwork f16 n=7", FULL_TOL)
        _, mid = _check(h, s, 300, "MainNetwork f16 n=300", FULL_TOL)
        _, big = _check(h, s, BIG, f"MainNetwork f16 n={BIG}", FULL_TOL)
        for a, b, c in zip(seven, mid, big):
            assert np.array_equal(a, b[:7]) and np.array_equal(a, c[:7])
        assert h.net_range()["fp16_overflows"] == 0
    finally:
        h.ctx.close()


def test_mainnetwork_within_1e3_of_torch_f32():
    """The project's stated bound for fp16 (tests/test_gpu_baseline_sizes.py): probabilities, value and ownership within 1e-3
    absolute of the torch f32 module, model.random_transgo_weights.  Measured on an MI355X: policy 1.5e-6, value 2.5e-5, ownership 5.3e-5."""
    import torch
    from oracle.net import TransGoMain
    from tests.half_attention_ref import FULL, setup
    from transgo_amd.model import random_transgo_weights
    torch.set_num_threads(8)
    sd = random_transgo_weights(9, 10, 128, seed=21)
    net = TransGoMain(9, 10, 128).eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    x = setup("A")["x"]
    with torch.no_grad():
        want = [t.numpy() for t in net.main_prediction(torch.from_numpy(x))]
    h = _net(FULL, sd, x.shape[0])
    try:
        got = h.main_prediction(x)
        e = [float(np.abs(a - b).max()) for a, b in zip(got, want)]
        print(f"\nMainNetwork f16 vs torch f32: max abs error policy {e[0]:.2e} value {e[1]:.2e} own {e[2]:.2e}")
        assert max(e) < 1e-3
        assert h.net_range()["fp16_overflows"] == 0
    finally:
        h.ctx.close()


def test_negative_control_mutated_value_channel_is_flagged():
    """The comparator can fail on the GPU: the HIP network runs with one value_conv output channel zeroed, the reference does not."""
    from tests.half_attention_ref import case_mutations, setup, state_dict_np
    code = "AR"
    s = setup(code)
    m = [m for m in case_mutations(code, _tol(code)) if "value_conv" in m.name][0]
    h = _net(code, state_dict_np(m.apply(s["net"])), 64)
    try:
        _check(h, s, 50, f"negative control {code}: HIP network with '{m.name}'", _tol(code), expect_fail=True)
    finally:
        h.ctx.close()


def test_background_refresh_equals_a_fresh_load():
    """tg_net_load_async restages the fp16 attention images (trunk and +P) into the retired set; after adoption the outputs are
    bit-identical to a fresh context loaded with the same weights."""
    from tests.half_attention_ref import arch_of, parity_arch, setup, state_dict_np
    from transgo_amd import model
    code = "RA+P"
    s = setup(code)
    x = s["x"]
    sd_a = state_dict_np(s["net"])
    sd_b = state_dict_np(parity_arch(code, 9, 10, 128, 777, x))
    fresh = _net(code, sd_b, 64)
    try:
        want = fresh.main_prediction(x)
    finally:
        fresh.ctx.close()
    h = _net(code, sd_a, 64)
    try:
        old = h.main_prediction(x)
        blob = model.pack_weights(sd_b, 9, 10, 128, arch=arch_of(code))
        h.ctx.call("tg_net_load_async", code.encode(), blob.ctypes.data_as(ctypes.c_void_p), blob.size)
        pend = ctypes.c_int(-1)
        h.ctx.call("tg_net_load_poll", 1, ctypes.byref(pend))
        assert pend.value == 0
        got = h.main_prediction(x)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert not any(np.array_equal(a, b) for a, b in zip(got, old))
    finally:
        h.ctx.close()


def test_range_guard_counts_an_attention_input_beyond_fp16():
    """Arch "A" with the stem's BatchNorm gain x 8e4: the BN-folded stem weights still fit fp16 (|w| < 65504) but the stem's output
    does not, and the stem writes only its f32 stream, so the attention block's projection input is the one fp16 rounding that sees
    the values beyond 65504.  A counted condition, not an error path."""
    import copy
    import torch
    from tests.half_attention_ref import setup, state_dict_np
    s = setup("A")
    good = state_dict_np(s["net"])
    big = copy.deepcopy(s["net"])
    with torch.no_grad():
        big.main_network.conv1.conv[1].weight.mul_(8e4)
        assert float(big.main_network.conv1(torch.from_numpy(s["x"])).max()) > 2 * 65504
    bad = state_dict_np(big)
    h = _net("A", good, 64)
    try:
        h.main_prediction(s["x"])
        assert h.net_range()["fp16_overflows"] == 0
        assert h.set_weights(bad)["weight_absmax"] < 65504
        h.main_prediction(s["x"])
        assert h.net_range()["fp16_overflows"] > 0
        msg = h.ctx.lib.tg_last_error(h.ctx.h).decode()
        assert "fp16 overflow" in msg and "65504" in msg
    finally:
        h.ctx.close()


@pytest.mark.parametrize("prec,S,F", [("f16r", 9, 128), ("f16", 9, 256), ("f16", 19, 128)])
def test_refusals_name_what_is_built_and_the_f32_modes_keep_working(prec, S, F):
    """fp16 attention is built for "f16" at 9x9 with 128 filters only: "f16r", F = 256 and 19x19 are TransgoErrors that say so.  The
    same arch and shape keep working in "f32" and "f32x3" (one forward each, within 1e-3 of each other and of the built f16 case)
    -- at 9x9: no precision has an attention kernel for 19x19 (f32 loads and fails at the forward, f32x3 is refused at the load, as
    before this mode existed), so there only the refusal is checked."""
    from tests.half_attention_ref import seeded_arch, state_dict_np
    from tests.test_net_reference import parity_positions
    from transgo_amd._lib import TransgoError
    code = "RA"
    x = parity_positions(S, 6, 31)
    # random-init weights: the class the 1e-3 absolute bound of the fp16 modes is stated for (the parity weight sets are made to
    # amplify every layer: logit spreads up to 14, where half an fp16 ulp of an activation is already 1e-3 of a probability)
    sd = state_dict_np(seeded_arch(code, S, 10, F, 55))
    with pytest.raises(TransgoError, match="9x9 with 128 filters"):
        _net(code, sd, 8, precision=prec, S=S, F=F)
    if S != 9:
        return
    outs = {}
    for p in ("f32", "f32x3") + (("f16",) if (S, F) == (9, 128) else ()):
        h = _net(code, sd, 8, precision=p, S=S, F=F)
        try:
            outs[p] = h.main_prediction(x)
        finally:
            h.ctx.close()
    for p in outs:
        e = max(float(np.abs(a - b).max()) for a, b in zip(outs[p], outs["f32"]))
        print(f"\n{code} {S}x{S} F={F} {p} vs f32: {e:.2e}")
        assert e < 1e-3


def test_self_play_end_to_end_on_the_fp16_mainnetwork():
    """Config(network="transgo", inference_dtype="f16") through BatchedSelfPlay: games finish, no engine error, no fp16 overflow,
    the harvested records have the reference's shapes."""
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    cfg = Config(network="transgo", inference_dtype="f16", num_simulation=24, max_step=12)
    sp = BatchedSelfPlay(cfg, 16)
    sp.set_weights(model.random_transgo_weights(9, 10, 128, seed=3))
    try:
        sp.start()
        finished = []
        for _ in range(14):
            finished += sp.step()
            if len(finished) >= 16:
                break
        st = sp.engine.stats()
        assert len(finished) >= 16 and st["errors"] == 0 and st["fp16_overflows"] == 0
        obs, pi, z, own = sp.targets(finished[0])[0]
        assert obs.shape == (10, 9, 9) and abs(pi.sum() - 1.0) < 1e-9 and z in (-1.0, 1.0) and own.shape == (81,)
    finally:
        sp.engine.close()
