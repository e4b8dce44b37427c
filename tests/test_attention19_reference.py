"""Self_Attention at 19x19 in f32 (k_attention_t, net.hip), the CPU side: the two-pass form the tiled kernel computes is the oracle's
Self_Attention, and the fixture and tolerances that tests/test_gpu_attention19.py holds the kernel to.

Orientation.  energy[i][j] = q_i . k_j, softmax over j, out[:, j] = sum_i v[:, i] attention[i][j]: the sum runs over the softmaxed
ROW index, so the normaliser belongs to the index being summed and a tiled kernel needs the row statistics (m_i, l_i) of every row
before it forms the first output column -- pass 1: m_i = max_j e_ij, l_i = sum_j exp(e_ij - m_i); pass 2, per column tile:
out[:, j] = sum_i (v[:, i] / l_i) exp(e_ij - m_i).  two_pass() below is that, tile by tile (16 wide, P = 361 = 22 tiles + 9), in
float64; a kernel that took the softmax over i, or summed over j, fails the non-symmetric case.

Fixture.  One parity weight set per (arch code, filters) at S = 19, C = 10 (oracle.net.parity_weights; the MainNetwork through
parity_transgo), on 8 positions of one draw of parity_positions(19, 64, .): six from play (the last one around move 200: a dense
board), the empty board and the all-edges board.  The reference is oracle.net.float64_forward.

Tolerance.  tolerance(code, F) = max(PARITY_TOL["f32"], 4 x e_cpu), e_cpu the logit-space parity_error of the torch f32 forward of
the same module against the float64 forward on these positions: the reference's own f32 sensitivity is the yardstick, the factor 4
covers another summation order over 361 terms.  Measured e_cpu (torch 2.x CPU, 8 threads):
    F = 128: A 3.6e-6, AR 2.6e-6, AA 2.6e-6, RA+P 8.5e-6; MainNetwork 1.9e-6
    F = 256: AR 2.2e-6, RA+P 2.0e-6
4 x e_cpu stays below PARITY_TOL["f32"] = 5e-5 for every code (the largest, RA+P at F = 128, is 3.4e-5): all tolerances are 5e-5."""
import numpy as np
import pytest
import torch

from oracle.net import PARITY_TOL, SelfAttention, check_weight_properties, float64_forward, parity_error, parity_transgo
from tests.half_attention_ref import FULL, parity_arch

S, C = 19, 10
SHORT = ("A", "AR", "AA", "RA+P")
SEEDS = {"A": 1901, "AR": 1902, "AA": 1903, "RA+P": 1904, FULL: 1905}
PICK = (2, 12, 24, 36, 48, 63, 64, 65)       # of the draw below: six from play (63: dense), the empty board, the all-edges board
ALT = (5, 15, 30, 40, 55, 60, 8, 20)         # the prefill positions of the GPU tests
_draw = []
_setups = {}


def positions():
    """(x, alt): the 8 checked positions and 8 others, all from one draw."""
    if not _draw:
        from tests.test_net_reference import parity_positions
        _draw.append(parity_positions(S, 64, 719))
    d = _draw[0]
    return d[list(PICK)], d[list(ALT)]


def setup(code, F=128):
    """dict(net, x, alt, ref, e_cpu, props) of the weight set of arch `code` with F filters; computed once per process."""
    if (code, F) not in _setups:
        torch.set_num_threads(8)
        x, alt = positions()
        net = parity_transgo(S, C, F, SEEDS[code], x) if code == FULL else parity_arch(code, S, C, F, SEEDS[code], x)
        ref = float64_forward(net, x)
        with torch.no_grad():
            f32 = [t.numpy() for t in net.main_prediction(torch.from_numpy(x))]
        _setups[(code, F)] = dict(net=net, x=x, alt=alt, ref=ref, e_cpu=parity_error(f32, ref)[0], props=check_weight_properties(ref))
    return _setups[(code, F)]


def tolerance(code, F=128):
    return max(PARITY_TOL["f32"], 4.0 * setup(code, F)["e_cpu"])


def value_channel_mutation(code, F=128):
    """(net with one value_conv output channel of the first attention block zeroed, its float64 effect): the channel, of the four
    with the largest weight norm, that moves the float64 reference the most."""
    import copy
    s = setup(code, F)
    name = [n for k, n in zip(s["net"].main_network.arch.kinds, s["net"].main_network.arch.names) if k == "A"][0]
    w = getattr(s["net"].main_network, name).value_conv.weight.detach().flatten(1).norm(dim=1)
    best = None
    for c in [int(c) for c in torch.argsort(w, descending=True)[:4]]:
        m = copy.deepcopy(s["net"])
        with torch.no_grad():
            cv = getattr(m.main_network, name).value_conv
            cv.weight[c] = 0.0
            cv.bias[c] = 0.0
        eff = parity_error(float64_forward(m, s["x"]), s["ref"])[0]
        if best is None or eff > best[1]:
            best = (m, eff)
    return best


def two_pass(q, k, v, tile=16):
    """out[c][j] of one board from q [P][d], k [P][d], v [P][F] (float64), the way the tiled kernel walks it."""
    P = q.shape[0]
    m = np.full(P, -np.inf)
    l = np.zeros(P)
    for i0 in range(0, P, tile):                       # pass 1: row statistics, a tile row at a time, padded columns excluded
        e = q[i0:i0 + tile] @ k.T
        m[i0:i0 + tile] = e.max(1)
        l[i0:i0 + tile] = np.exp(e - e.max(1, keepdims=True)).sum(1)
    out = np.zeros((v.shape[1], P))
    for j0 in range(0, P, tile):                       # pass 2: one output column tile at a time, summed over every row tile
        for i0 in range(0, P, tile):
            e = q[i0:i0 + tile] @ k[j0:j0 + tile].T
            p = np.exp(e - m[i0:i0 + tile, None]) / l[i0:i0 + tile, None]
            out[:, j0:j0 + tile] += v[i0:i0 + tile].T @ p
    return out


@pytest.mark.parametrize("F", [128, 256])
def test_two_pass_formula_is_the_oracles_self_attention(F):
    """Random 19x19 input, random (non-symmetric) q / k weights: the two-pass form equals oracle.net.SelfAttention in float64 to
    1e-12; the transposed softmax and the transposed sum do not."""
    g = torch.Generator().manual_seed(40 + F)
    att = SelfAttention(F).double().eval()
    with torch.no_grad():
        for p in att.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.3 if p.dim() > 1 else 0.1))
        att.gamma.fill_(0.8)
        att.bn.running_mean.copy_(torch.randn(F, generator=g, dtype=torch.float64) * 0.1)
        att.bn.running_var.copy_(torch.rand(F, generator=g, dtype=torch.float64) + 0.5)
    x = torch.randn(2, F, S, S, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = att(x).numpy()
        proj = lambda conv: conv(x).view(2, -1, S * S).permute(0, 2, 1).numpy()           # [board][P][channels]
        q, k, v = proj(att.query_conv), proj(att.key_conv), proj(att.value_conv)
        sc = (att.bn.weight / torch.sqrt(att.bn.running_var + att.bn.eps)).numpy()
        sh = att.bn.bias.numpy() - att.bn.running_mean.numpy() * sc
    xn = x.numpy().reshape(2, F, S * S)

    def block(o, b):
        return np.maximum((0.8 * o + xn[b]) * sc[:, None] + sh[:, None], 0.0).reshape(F, S, S)

    for b in range(2):
        e = q[b] @ k[b].T
        assert np.abs(e - e.T).max() > 0.1                                                # the case is not symmetric
        assert np.abs(block(two_pass(q[b], k[b], v[b]), b) - want[b]).max() < 1e-12
        soft_i = np.exp(e - e.max(0)) / np.exp(e - e.max(0)).sum(0)                       # softmax over i instead of j
        soft_j = np.exp(e - e.max(1, keepdims=True)) / np.exp(e - e.max(1, keepdims=True)).sum(1, keepdims=True)
        assert np.abs(block(v[b].T @ soft_i, b) - want[b]).max() > 1e-3
        assert np.abs(block(v[b].T @ soft_j.T, b) - want[b]).max() > 1e-3                 # summed over j instead of i


def test_positions_hold_an_empty_and_a_dense_board():
    x, alt = positions()
    assert x.shape == (8, C, S, S) and len({p.tobytes() for p in x}) == 8
    assert not {p.tobytes() for p in x} & {p.tobytes() for p in alt}
    stones = x[:, [2, 5]].sum((1, 2, 3))          # planes 2 and 5: the current stones of the two colours
    print("stones per checked position:", stones.astype(int).tolist())
    assert stones.min() == 0 and stones.max() >= 120


@pytest.mark.parametrize("code,F", [(c, 128) for c in SHORT] + [("AR", 256), ("RA+P", 256), (FULL, 128)])
def test_fixture_and_tolerance(code, F):
    """The weight set has the properties the comparator relies on (check_weight_properties in setup()), the tolerance follows the
    rule of the docstring, and -- for the arch of the GPU negative control -- a zeroed value_conv channel is far above it."""
    s = setup(code, F)
    tol = tolerance(code, F)
    print(f"{code} F={F}: e_cpu {s['e_cpu']:.2e}, 4 x e_cpu {4 * s['e_cpu']:.2e}, tolerance {tol:.2e}; {s['props']}")
    assert tol == max(PARITY_TOL["f32"], 4.0 * s["e_cpu"])
    assert s["e_cpu"] < 1e-3                       # the f32 forward itself is well conditioned on this weight set
    if (code, F) == ("A", 128):
        _, eff = value_channel_mutation(code, F)
        print(f"    value_conv channel zeroed: {eff:.2e}")
        assert eff >= 4 * tol
