"""HIP network forward against a float64 reference at production batch sizes, on the dispatch paths the small-batch tests never
reach: the persistent tile walk of k_conv3x3_sg at F=256, both sides of every 2-GiB switch (DMA chain / general k_conv3x3, fp16 and
f32x3 refusals), the k_head_gemm tile walk, both F=128 tile shapes at 19x19, k_conv3x3_h2 (f16, f16r, f32x3) at 19x19 F=256 and
the MainNetwork at 4096 boards.

Weights: oracle.net.parity_tower / parity_transgo (every layer moves the outputs; the properties are asserted per case).  Batch:
K distinct positions from play plus the empty board and the all-edges board, repeated over the whole batch in a seeded
permutation (the last row, the final partial tile and the rows around the 2^30-byte offsets hold reference positions, so every
row is checked).  Order: one forward of the same size on OTHER positions first, so a skipped tile cannot leave correct values
behind; then the checked forward.  Asserted: all copies of a position are bit-identical, and the K + 2 distinct rows are within
the class tolerance of the float64 reference in logit space (oracle.net.parity_error).  Per case the smallest effect of the
class's mutations (oracle.net.mutations) on the reference must be at least 4x the tolerance; the negative controls load a
mutated weight set into the HIP network and require the comparator to flag it.

Tolerances (oracle.net.PARITY_TOL) and what an MI355X measured on these cases (max over policy, value, ownership in logit space):
    f32 class 5e-5: exact f32 towers <= 5.0e-6 (every path above, the general k_conv3x3 included), MainNetwork f32 1.2e-5, f32x3
        towers 3.5e-6, MainNetwork f32x3 1.1e-5;
    f16 class 2e-3: f16 6.4e-4, f16r 6.6e-4 (19x19, F=256; what is left is fp16 rounding-boundary flips under another summation
        order: the float64 emulation itself moves by up to 8.6e-4 when it accumulates in f32).
Smallest mutation effect per case 1.2e-2 .. 3.8e-2, i.e. >= 5.9x the f16 and >= 290x the f32 tolerance.  No kernel bug was found."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K = 40
GIB2 = 1 << 31
_refs = {}


def _setup(kind, S, F, NB, mode):
    """(net, x, ref, smallest mutation effect, its name, prefill positions) of a weight set, cached per (net, reference mode)."""
    key = (kind, S, F, NB, mode)
    if key not in _refs:
        import torch
        from oracle.net import check_weight_properties, mutations, parity_error, parity_tower, parity_transgo, reference
        from tests.test_net_reference import parity_positions
        torch.set_num_threads(16)
        x = parity_positions(S, K, 100 + S)
        net = parity_tower(S, 10, F, NB, 200 + F, x) if kind == "tower" else parity_transgo(S, 10, F, 300 + F, x)
        ref = reference(net, x, mode)
        props = check_weight_properties(ref)
        cls = "f32" if mode == "f64" else "f16"
        muts = mutations(cls, net, x)
        eff = min((parity_error(reference(net, x, mode, mutation=m), ref)[0], m.name) for m in muts)
        _refs[key] = dict(net=net, x=x, ref=ref, eff=eff, muts=muts, props=props, alt=parity_positions(S, K + 2, 900 + S))
    return _refs[key]


def _layout(n, k, S, F, seed):
    """Row -> position id: every id about n/k times in a seeded permutation; the last row holds the all-edges board (id k-1) and the
    rows holding byte offset 2^30 of the row-major f32 stream and of the slice-major conv input the empty board (id k-2)."""
    P = S * S
    ids = np.random.RandomState(seed).permutation(np.arange(n) % k)
    M = n * P
    for off_row in ((1 << 30) // (4 * F), (((1 << 24) % M) if M * F * 4 > (1 << 30) else -1)):
        if 0 <= off_row < M:
            ids[off_row // P] = k - 2
    ids[n - 1] = k - 1
    return ids


def _sd(net):
    return {k: v.detach().numpy() for k, v in net.state_dict().items()}


def _arch(kind):
    from transgo_amd.model import transgo_arch
    return transgo_arch() if kind == "mainnet" else None


def _check(h, setup, n, label, tol, expect_fail=False):
    """Prefill with other positions, run the checked forward of n rows, assert copies identical and parity; returns the error."""
    from oracle.net import parity_error
    x, alt = setup["x"], setup["alt"]
    k = x.shape[0]
    S, F = x.shape[-1], h.F
    ids = _layout(n, k, S, F, n)
    before = h.main_prediction(alt[np.random.RandomState(n + 1).randint(0, alt.shape[0], n)])
    got = h.main_prediction(x[ids])
    first = np.full(k, -1)
    for r in range(n - 1, -1, -1):
        first[ids[r]] = r
    assert (first >= 0).all()
    for a, b in zip(got, before):
        assert np.array_equal(a, a[first[ids]]), f"{label}: copies of one position differ"
        assert not np.array_equal(a, b)
    err, per = parity_error([a[first] for a in got], setup["ref"])
    eff, name = setup["eff"]
    print(f"\n{label}: max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} own {per[2]:.1e}), tolerance "
          f"{tol:.0e}, smallest mutation effect {eff:.2e} ({name})")
    assert eff >= 4 * tol
    if expect_fail:
        assert err > tol, f"{label}: the comparator did not flag the mutated weights"
    else:
        assert err < tol, label
    return err


def _net(kind, S, F, NB, prec, rows_cap, sd):
    from transgo_amd.model import HipNetwork
    h = HipNetwork(S, 10, F, NB, rows_cap=rows_cap, precision=prec, arch=_arch(kind))
    h.set_weights(sd)
    return h


def _f32_path(S, F, n, prec):
    M = n * S * S
    if prec == "f32":
        if M * F * 4 >= GIB2:
            return "k_conv3x3 (general, M*F*4 >= 2 GiB)"
        if F == 256:
            nt = (M + 127) // 128
            return f"k_conv3x3_sg F=256, {nt} tiles on {min(nt, 512)} workgroups"
        small = ((M + 131071) // 131072) * 131072 < ((M + 147455) // 147456) * 147456
        return f"k_conv3x3_sg F=128, {'128' if small else '192'}-row tiles"
    return f"k_conv3x3_h2 ({prec}), {(M + 255) // 256} row tiles"


def _head_path(S, n):
    tmh = 64 * (3 if S == 9 else 4) - 2 * (S + 1)
    nt = (n * S * S + tmh - 1) // tmh
    return f"k_head_gemm {nt} tiles{' (walk)' if nt > 512 else ''}"


MODE = {"f32": "f64", "f32x3": "f64", "f16": "half", "f16r": "half_res"}
CLS = {"f32": "f32", "f32x3": "f32", "f16": "f16", "f16r": "f16"}

# (case, kind, S, F, NB, precision, batch sizes): every size is checked in one context, in order
CASES = [
    ("dma-walk+head-walk-9x9-F256", "tower", 9, 256, 2, "f32", (2000,)),
    ("dma-walk+head-walk-19x19-F256", "tower", 19, 256, 2, "f32", (4096,)),
    ("dma-switch-19x19-F256", "tower", 19, 256, 2, "f32", (5809, 5810)),
    ("dma-switch-9x9-F256", "tower", 9, 256, 2, "f32", (25890, 25891)),
    ("dma-switch-9x9-F128", "tower", 9, 128, 2, "f32", (51781, 51782)),
    ("tile-shapes+head-walk-19x19-F128", "tower", 19, 128, 2, "f32", (400, 700)),
    ("h2-f16-19x19-F256", "tower", 19, 256, 2, "f16", (333,)),
    ("h2-f16r-19x19-F256", "tower", 19, 256, 2, "f16r", (333,)),
    ("h2-f32x3-19x19-F256", "tower", 19, 256, 2, "f32x3", (333,)),
    ("mainnet-f32-4096", "mainnet", 9, 128, 0, "f32", (4096,)),
    ("mainnet-f32x3-4096", "mainnet", 9, 128, 0, "f32x3", (4096,)),
]


@pytest.mark.parametrize("case,kind,S,F,NB,prec,sizes", CASES, ids=[c[0] for c in CASES])
def test_parity_at_production_sizes(case, kind, S, F, NB, prec, sizes):
    from oracle.net import PARITY_TOL
    setup = _setup("transgo" if kind == "mainnet" else "tower", S, F, NB, MODE[prec])
    h = _net(kind, S, F, NB, prec, max(sizes), _sd(setup["net"]))
    try:
        for n in sizes:
            path = _f32_path(S, F, n, prec) if kind == "tower" else f"MainNetwork {prec} (k_attention_mfma / k_attention_x3)"
            if prec == "f32" and kind == "tower":
                path += "; " + _head_path(S, n)
            _check(h, setup, n, f"{case} n={n} [{path}]", PARITY_TOL[CLS[prec]])
    finally:
        h.ctx.close()


@pytest.mark.parametrize("prec,n", [("f16", 11618), ("f32x3", 5809)])
def test_size_limit_accepted_below_refused_above(prec, n):
    """fp16 / f16r refuse M*F*2 >= 2^31 and f32x3 M*F*4 >= 2^31 (19x19, F=256): the last accepted batch is checked like every
    case, one row more is a clean TransgoError naming the limit (not the rows_cap error: the context has room for it)."""
    from oracle.net import PARITY_TOL
    from transgo_amd._lib import TransgoError
    S, F = 19, 256
    per = 2 if prec == "f16" else 4
    assert n * S * S * F * per < GIB2 <= (n + 1) * S * S * F * per
    setup = _setup("tower", S, F, 2, MODE[prec])
    h = _net("tower", S, F, 2, prec, n + 1, _sd(setup["net"]))
    try:
        _check(h, setup, n, f"{prec} limit n={n} [{_f32_path(S, F, n, prec)}]", PARITY_TOL[CLS[prec]])
        with pytest.raises(TransgoError, match="2 GiB"):
            h.main_prediction(np.repeat(setup["x"][:1], n + 1, 0))
        print(f"{prec} n={n + 1}: refused")
    finally:
        h.ctx.close()


@pytest.mark.parametrize("prec,S,F,n,mut", [("f32", 9, 256, 2000, 1), ("f16", 19, 256, 333, 0)])
def test_negative_control_mutated_weights_are_flagged(prec, S, F, n, mut):
    """The comparator can fail on the GPU: the HIP network runs a mutated weight set (f32: one weight of the last block's second
    conv zeroed; f16: one 3x3 slice of it), the reference stays unmutated."""
    from oracle.net import PARITY_TOL
    setup = _setup("tower", S, F, 2, MODE[prec])
    m = setup["muts"][mut]
    assert m.edit is not None
    h = _net("tower", S, F, 2, prec, n, _sd(m.apply(setup["net"])))
    try:
        _check(h, setup, n, f"negative control {prec} {S}x{S} F={F} n={n}: HIP network with '{m.name}'", PARITY_TOL[CLS[prec]],
               expect_fail=True)
    finally:
        h.ctx.close()
