"""Self_Attention at 19x19 in f32 on the GPU: the tiled k_attention_t (net.hip) and its plumbing -- both f32 chains, the out2
hand-off to a residual block of the DMA-fed chain, the pre-activated policy-head variant, the channel split at 256 filters, the
load-time refusals -- against oracle.net.float64_forward under the tolerances of tests/test_attention19_reference.py (fixture: 8
positions, one parity weight set per arch code; every tolerance is max(PARITY_TOL["f32"], 4 x e_cpu) = 5e-5 there).

Short archs are the smallest shapes at which each hand-off can be wrong: "A" (attention after the stem, tail BN behind it), "AR"
(out2 for the next block), "AA" (no out2 between the two), "RA+P" (the policy head's pre-activated input).  Batches of 1, 5 and
300 boards (more boards than CUs: a second round of workgroups), built from copies of the 8 positions, after a prefill forward on
other positions.

Measured on an MI355X, max logit-space error against float64 over the batch sizes (tolerance 5e-5):
    F = 128: A 3.8e-6, AR 2.9e-6, AA 3.0e-6, RA+P 4.9e-6; F = 256: AR 2.8e-6, RA+P 2.3e-6;
    AR with TG_DMA_CONV=0: 2.0e-6, and 3.1e-6 from the DMA chain's result; MainNetwork (parity_transgo) 7.3e-6.
    MainNetwork with random_transgo_weights against the torch f32 module: policy 4.4e-9, value 9.7e-8, ownership 2.5e-7 absolute (1e-3).
    Negative control (one value_conv channel zeroed in the HIP network only): 4.5e-2.
Per launch at 1024 boards, F = 128 (profiles/att19_transgo_launch_times.json): k_attention_t 0.728 ms, its q|k|v projection 0.186 ms,
one k_conv3x3_sg<19,128,.> 0.770 / 0.798 ms -- an attention block is 0.58x a residual block."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, C = 19, 10


def _ref():
    import tests.test_attention19_reference as r
    return r


def _net(code, sd, rows_cap, precision="f32", F=128):
    from tests.half_attention_ref import arch_of
    from transgo_amd.model import HipNetwork
    h = HipNetwork(S, C, F, rows_cap=rows_cap, arch=arch_of(code), precision=precision)
    h.set_weights(sd)
    return h


def _ids(n):
    """n rows of the 8 positions: rows 0-4 are positions 0-4 for every n >= 5 (so the batches can be compared row by row), then the
    rest in order, then a seeded draw of copies."""
    return np.concatenate([np.arange(8), np.random.RandomState(n).randint(0, 8, max(0, n - 8))])[:n]


def _check(h, s, n, label, tol, expect_fail=False):
    """Prefill on other positions, then the checked forward of n rows: copies of a position bit-identical, the distinct positions
    within tol of the float64 reference (or, expect_fail, beyond it).  Returns (error, outputs)."""
    from oracle.net import parity_error
    x, alt = s["x"], s["alt"]
    ids = _ids(n)
    before = h.main_prediction(alt[np.random.RandomState(n + 1).randint(0, alt.shape[0], n)])
    got = h.main_prediction(x[ids])
    first = np.array([int(np.flatnonzero(ids == i)[0]) if (ids == i).any() else -1 for i in range(x.shape[0])])
    have = first >= 0
    for a, b in zip(got, before):
        assert np.array_equal(a, a[first[ids]]), f"{label}: copies of one position differ"
        assert not np.array_equal(a, b)
    err, per = parity_error([a[first[have]] for a in got], [r[have] for r in s["ref"]])
    print(f"\n{label}: max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} own {per[2]:.1e}), tolerance {tol:.1e}")
    if expect_fail:
        assert err > tol, f"{label}: the comparator did not flag the mutated weights"
    else:
        assert err < tol, label
    return err, got


@pytest.mark.parametrize("code", ["A", "AR", "AA", "RA+P"])
def test_short_archs_against_float64(code):
    from tests.half_attention_ref import state_dict_np
    s = _ref().setup(code)
    tol = _ref().tolerance(code)
    h = _net(code, state_dict_np(s["net"]), 300)
    try:
        _, one = _check(h, s, 1, f"{code} n=1", tol)
        _, five = _check(h, s, 5, f"{code} n=5", tol)
        _, big = _check(h, s, 300, f"{code} n=300", tol)
        same = all(np.array_equal(a, b[:1]) and np.array_equal(b, c[:5]) for a, b, c in zip(one, five, big))
    finally:
        h.ctx.close()
    assert same, f"{code}: a board's result depends on its batch"


@pytest.mark.parametrize("code", ["AR", "RA+P"])
def test_256_filters_split_the_channels_over_two_sweeps(code):
    from tests.half_attention_ref import state_dict_np
    s = _ref().setup(code, 256)
    tol = _ref().tolerance(code, 256)
    h = _net(code, state_dict_np(s["net"]), 8, F=256)
    try:
        _, one = _check(h, s, 1, f"{code} F=256 n=1", tol)
        _, five = _check(h, s, 5, f"{code} F=256 n=5", tol)
        same = all(np.array_equal(a, b[:1]) for a, b in zip(one, five))
    finally:
        h.ctx.close()
    assert same


_CHILD = """
import sys
import numpy as np
from tests.half_attention_ref import arch_of
from transgo_amd.model import HipNetwork
d = np.load(sys.argv[1], allow_pickle=True)
sd = {k[3:]: d[k] for k in d.files if k.startswith("sd:")}
h = HipNetwork(19, 10, 128, rows_cap=8, arch=arch_of("AR"), precision="f32")
try:
    h.set_weights(sd)
    h.main_prediction(d["alt"][:5])
    p, v, o = h.main_prediction(d["x"][:5])
finally:
    h.ctx.close()
np.savez(sys.argv[2], p=p, v=v, o=o)
"""


def test_general_f32_chain_without_out2(tmp_path):
    """TG_DMA_CONV=0 (read at the load, so in a fresh process): the residual block runs on k_conv3x3 and activates its own input,
    the attention kernel gets out2 = nullptr.  Within tolerance of float64 and within PARITY_TOL["f32"] of the DMA chain's result."""
    from oracle.net import PARITY_TOL, parity_error
    from tests.half_attention_ref import state_dict_np
    code = "AR"
    s = _ref().setup(code)
    tol = _ref().tolerance(code)
    sd = state_dict_np(s["net"])
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, x=s["x"], alt=s["alt"], **{"sd:" + k: v for k, v in sd.items()})
    env = dict(os.environ, TG_DMA_CONV="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, src, dst], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(dst)
    f32 = [d["p"], d["v"], d["o"]]
    h = _net(code, sd, 8)
    try:
        _, dma = _check(h, s, 5, f"{code} DMA chain n=5", tol)
    finally:
        h.ctx.close()
    err = parity_error(f32, [r_[:5] for r_ in s["ref"]])[0]
    gap = parity_error(f32, dma)[0]
    print(f"\n{code} TG_DMA_CONV=0 n=5: error against float64 {err:.2e} (tolerance {tol:.1e}), against the DMA chain {gap:.2e}")
    assert err < tol
    assert gap < PARITY_TOL["f32"]


def test_mainnetwork_against_float64():
    from tests.half_attention_ref import FULL, state_dict_np
    s = _ref().setup(FULL)
    h = _net(FULL, state_dict_np(s["net"]), 8)
    try:
        _check(h, s, 5, "MainNetwork 19x19 n=5", _ref().tolerance(FULL))
    finally:
        h.ctx.close()


def test_mainnetwork_within_1e3_of_torch_f32():
    """The project's stated bound: probabilities, value and ownership within 1e-3 absolute of the torch f32 module
    (oracle.net.TransGoMain) with model.random_transgo_weights."""
    import torch
    from oracle.net import TransGoMain
    from tests.half_attention_ref import FULL
    from transgo_amd.model import random_transgo_weights
    torch.set_num_threads(8)
    sd = random_transgo_weights(S, C, 128, seed=23)
    net = TransGoMain(S, C, 128).eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    x = _ref().positions()[0]
    with torch.no_grad():
        want = [t.numpy() for t in net.main_prediction(torch.from_numpy(x))]
    h = _net(FULL, sd, 8)
    try:
        got = h.main_prediction(x)
    finally:
        h.ctx.close()
    e = [float(np.abs(a - b).max()) for a, b in zip(got, want)]
    print(f"\nMainNetwork 19x19 f32 vs torch f32: max abs error policy {e[0]:.2e} value {e[1]:.2e} own {e[2]:.2e}")
    assert max(e) < 1e-3


def test_negative_control_mutated_value_channel_is_flagged():
    """The comparator sees this kernel's output: the HIP network runs with one value_conv output channel zeroed, the reference
    does not."""
    from tests.half_attention_ref import state_dict_np
    code = "A"
    s = _ref().setup(code)
    mutated, eff = _ref().value_channel_mutation(code)
    h = _net(code, state_dict_np(mutated), 8)
    try:
        _check(h, s, 5, f"negative control {code} (float64 effect {eff:.2e})", _ref().tolerance(code), expect_fail=True)
    finally:
        h.ctx.close()


@pytest.mark.parametrize("prec,F", [("f16", 128), ("f32x3", 128), ("f32", 64)])
def test_refusals_at_the_load_name_what_is_built(prec, F):
    """fp16 and split precision with attention at 19x19, and f32 attention at 19x19 with other than 128 / 256 filters, are refused
    when the weights are loaded -- not at the first forward -- with a message that names what is built."""
    from tests.half_attention_ref import seeded_arch, state_dict_np
    from transgo_amd._lib import TransgoError
    from transgo_amd.model import HipNetwork
    from tests.half_attention_ref import arch_of
    code = "RA"
    sd = state_dict_np(seeded_arch(code, S, C, F, 55))
    h = HipNetwork(S, C, F, rows_cap=8, arch=arch_of(code), precision=prec)
    try:
        with pytest.raises(TransgoError, match="128 filters|128 or 256 filters"):
            h.set_weights(sd)
    finally:
        h.ctx.close()


def test_self_play_end_to_end_on_the_19x19_mainnetwork():
    from transgo_amd import model
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    cfg = Config(board_size=19, network="transgo", num_simulation=16, max_step=8, concurrent_games=8)
    sp = BatchedSelfPlay(cfg, cfg.concurrent_games)
    try:
        sp.set_weights(model.random_transgo_weights(19, 10, 128, seed=3))
        sp.start()
        finished = []
        for _ in range(10):
            finished += sp.step()
            if len(finished) >= 8:
                break
        st = sp.engine.stats()
        obs, pi, z, own = sp.targets(finished[0])[0] if finished else (None,) * 4
    finally:
        sp.engine.close()
    assert len(finished) >= 8 and st["errors"] == 0
    assert obs.shape == (10, 19, 19) and own.shape == (361,) and abs(pi.sum() - 1.0) < 1e-9
