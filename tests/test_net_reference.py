"""The float64 parity reference of the network tests (oracle/net.py), on the CPU: the parity weight sets make every layer matter,
torch f32 passes the logit-space comparator against float64, and every mutation -- a bug of the kind a kernel could have -- fails
it by a wide margin.  tests/test_gpu_net_parity.py holds the HIP kernels to the same comparator."""
import numpy as np
import pytest
import torch

from oracle.net import (PARITY_TOL, check_weight_properties, half_storage_forward, mutations, parity_error, parity_tower,
                        parity_transgo, reference)


def parity_positions(S, k, seed):
    """k distinct positions from random play, then the empty board and a board with a stone on every edge point (black on the
    first and last row, white on the first and last column in between)."""
    from oracle.go_oracle import OracleGoEnv
    env = OracleGoEnv(board_size=S, max_step=S * S)
    rng = np.random.RandomState(seed)
    obs, seen = [], set()
    while len(obs) < k:
        s, done = env.reset()
        while not done and len(obs) < k:
            la = env.getLegalAction(s)
            s, done = env.step(s, int(la[rng.randint(len(la))]))
            e = env.encode(s)
            if rng.rand() < 0.3 and e.tobytes() not in seen:
                seen.add(e.tobytes())
                obs.append(e)
    s, _ = env.reset()
    obs.append(env.encode(s))
    black = [r * S + c for r in (0, S - 1) for c in range(S)]
    white = [r * S + c for c in (0, S - 1) for r in range(1, S - 1)]
    white += [S * S] * (len(black) - len(white))                   # white passes once its edge points are taken
    for b, w in zip(black, white):
        s, _ = env.step(s, b)
        s, _ = env.step(s, w)
    obs.append(env.encode(s))
    return np.stack(obs)


def mutation_margin(net, x, mode, cls, ref):
    """Smallest logit-space effect over the class's mutations on positions x, with the name of that mutation."""
    effects = [(parity_error(reference(net, x, mode, mutation=m), ref)[0], m.name) for m in mutations(cls, net, x)]
    return min(effects)


CASES = [("tower", 9, 128, 6), ("tower", 9, 256, 2), ("tower", 19, 128, 2), ("transgo", 9, 64, 0), ("transgo", 9, 128, 0)]


def _net(kind, S, F, NB, x, seed=11):
    return parity_tower(S, 10, F, NB, seed, x) if kind == "tower" else parity_transgo(S, 10, F, seed, x)


@pytest.mark.parametrize("kind,S,F,NB", CASES)
def test_torch_f32_passes_and_every_mutation_fails(kind, S, F, NB):
    torch.set_num_threads(4)
    x = parity_positions(S, 24, 5)
    net = _net(kind, S, F, NB, x)
    ref = reference(net, x)
    props = check_weight_properties(ref)
    with torch.no_grad():
        got = [t.numpy() for t in net.main_prediction(torch.from_numpy(x))]
    err, per = parity_error(got, ref)
    tol = PARITY_TOL["f32"]
    eff, name = mutation_margin(net, x, "f64", "f32", ref)
    print(f"{kind} {NB}x{F}@{S}: torch f32 vs float64 {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} own {per[2]:.1e}), "
          f"tolerance {tol:.0e}, smallest mutation effect {eff:.2e} ({name}); {props}")
    assert err < tol / 2
    assert eff >= 4 * tol


@pytest.mark.parametrize("S,F,NB,half_res", [(9, 128, 4, False), (9, 256, 2, True), (19, 256, 1, False)])
def test_half_storage_reference_and_mutations(S, F, NB, half_res):
    """The fp16 class: the f32-accumulating emulation sits within the tolerance of its float64 version (the rest is the order of
    summation), the float64 version itself is the same rounding points (it matches the f32 one far more closely than the f32
    network), and every fp16-class mutation is at least 4x the tolerance away."""
    torch.set_num_threads(4)
    x = parity_positions(S, 16, 9)
    net = _net("tower", S, F, NB, x)
    mode = "half_res" if half_res else "half"
    ref = reference(net, x, mode)
    check_weight_properties(ref)
    emu32 = [t.numpy() for t in half_storage_forward(net, torch.from_numpy(x), half_residual=half_res)]
    err = parity_error(emu32, ref)[0]
    tol = PARITY_TOL["f16"]
    eff, name = mutation_margin(net, x, mode, "f16", ref)
    f64_gap = parity_error(reference(net, x), ref)[0]
    print(f"fp16 {'f16r' if half_res else 'f16'} {NB}x{F}@{S}: f32 emulation vs float64 emulation {err:.2e}, exact float64 network "
          f"{f64_gap:.2e}, tolerance {tol:.0e}, smallest mutation effect {eff:.2e} ({name})")
    assert err < tol
    assert f64_gap > 2 * err                     # the reference really carries the fp16 rounding points
    assert eff >= 4 * tol


def test_reference_is_per_position():
    """The reference may run on a subset of a batch: every position's outputs depend on that position alone."""
    torch.set_num_threads(4)
    x = parity_positions(9, 10, 2)
    net = _net("tower", 9, 64, 2, x)
    full = reference(net, x)
    part = reference(net, x[3:6])
    assert all(np.array_equal(a[3:6], b) or np.abs(a[3:6] - b).max() < 1e-14 for a, b in zip(full, part))
    h_full = reference(net, x, "half")
    h_part = reference(net, x[[7, 1]], "half")
    assert all(np.abs(a[[7, 1]] - b).max() < 1e-14 for a, b in zip(h_full, h_part))


def test_weight_properties_guard():
    """The property check rejects the weight sets it exists to rule out: torch's default init (nearly constant outputs) and
    a tower whose heads saturate tanh."""
    from oracle.net import parity_weights, seeded_tower, TowerNetwork
    x = parity_positions(9, 8, 4)
    with pytest.raises(AssertionError):
        check_weight_properties(reference(seeded_tower(9, 10, 64, 2, seed=3), x))
    hot = parity_weights(TowerNetwork(9, 10, 64, 2).eval(), 3, vo_gain=40.0)
    with pytest.raises(AssertionError), np.errstate(divide="ignore"):
        check_weight_properties(reference(hot, x))


def test_edge_and_empty_positions():
    x = parity_positions(9, 4, 1)
    assert x.shape == (6, 10, 9, 9)
    occ = x[-1].sum(0)
    ring = np.ones((9, 9), bool); ring[1:-1, 1:-1] = False
    assert (occ[ring] == 1).all() and (occ[~ring] == 0).all()
    assert x[-2][[0, 1, 2, 3, 4, 5]].sum() == 0
