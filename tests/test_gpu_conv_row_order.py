"""f32 tower on the board-grouped slice-major row order (transgo_amd/csrc/conv_rows.h) and the tap-skipping k_conv3x3_sg, against
the float64 reference of oracle.net, for board counts around every boundary the order introduces: 1, one short of / exactly / one
past a group of 16 boards (15, 16, 17), and one short of / one past a workgroup's board range at both tile shapes (64*2 and 64*3
boards: 127, 129, 191, 193).  Then a batch with a partial last group (37 = 2 groups + 5 boards) right after a LARGER forward (200
boards) on other positions, so the never-written rows of its 11 absent boards hold stale activations of that forward: they feed
only MFMA columns that are never stored, and the 37 results must not notice.

Every row of every batch is compared with the reference row of its position at the f32 class tolerance oracle.net.PARITY_TOL (5e-5
in logit space; the exact-f32 towers measure <= 5e-6 against float64, tests/test_gpu_net_parity.py), and rows that hold the same
position must be bit-identical whichever board group, MFMA column and workgroup they fall in.  Each checked forward follows one
of the same size on other positions, so a skipped tile cannot leave correct values behind."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K = 40
SIZES = (1, 15, 16, 17, 127, 129, 191, 193)
_refs = {}


def _setup(S, F):
    if (S, F) not in _refs:
        import torch
        from oracle.net import parity_tower, reference
        from tests.test_net_reference import parity_positions
        torch.set_num_threads(16)
        x = parity_positions(S, K, 100 + S)
        net = parity_tower(S, 10, F, 2, 200 + F, x)
        _refs[(S, F)] = dict(net=net, x=x, ref=reference(net, x, "f64"), alt=parity_positions(S, K + 2, 900 + S))
    return _refs[(S, F)]


def _check(h, setup, n, label, prefill):
    from oracle.net import PARITY_TOL, parity_error
    x, alt, ref = setup["x"], setup["alt"], setup["ref"]
    k = x.shape[0]
    ids = np.random.RandomState(n).permutation(np.arange(max(n, k)) % k)[:n]
    before = h.main_prediction(alt[np.random.RandomState(n + 1).randint(0, alt.shape[0], prefill)])
    got = h.main_prediction(x[ids])
    first = {}
    for r in range(n):
        first.setdefault(ids[r], r)
    same = np.array([first[i] for i in ids])
    for a, b in zip(got, before):
        assert a.shape[0] == n
        assert np.array_equal(a, a[same]), f"{label}: copies of one position differ"
        assert not np.array_equal(a, b[:n])
    err, per = parity_error(got, [r[ids] for r in ref])
    print(f"\n{label}: max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} own {per[2]:.1e}), tolerance "
          f"{PARITY_TOL['f32']:.0e}")
    assert err < PARITY_TOL["f32"], label


@pytest.mark.parametrize("S,F", [(9, 128), (9, 256), (19, 128)], ids=["9x9-F128", "9x9-F256", "19x19-F128"])
def test_f32_tower_parity_around_group_and_range_boundaries(S, F):
    from transgo_amd.model import HipNetwork
    setup = _setup(S, F)
    h = HipNetwork(S, 10, F, 2, rows_cap=200, precision="f32")
    h.set_weights({k: v.detach().numpy() for k, v in setup["net"].state_dict().items()})
    try:
        for n in SIZES:
            _check(h, setup, n, f"{S}x{S} F={F} n={n}", prefill=n)
        _check(h, setup, 37, f"{S}x{S} F={F} n=37 after a forward of 200 (stale padded rows)", prefill=200)
    finally:
        h.ctx.close()
