"""The launch order of k_conv3x3_sg (conv_launch_wg, transgo_amd/csrc/conv_rows.h) on the device: every (board range, position)
workgroup of a launch must run exactly once, whichever branch of the map its blockIdx takes.

Network: a 2-block x 128-filter f32 tower at 9x9 with random weights (oracle.net.parity_tower: every layer moves the outputs).
Batches 1, 130, 1024 (8 ranges of 128 boards: one per XCD, no leftover), 1100 (9: one leftover range dealt over the XCDs) and 2200
(18 = 2 * 8 + 2: whole ranges per XCD, all of them in the drain part, and two leftover ranges) -- the smallest counts that reach
every branch; one 19x19 / 128-filter case with 130 boards and one 9x9 / 256-filter case with 1100.

  * Batch-split invariance: the outputs of one tg_net_predict over all boards equal, bit for bit, those of the same boards
    evaluated in chunks of 100.  An MFMA column depends on its own board only, so any difference is a workgroup that was mapped to
    the wrong (range, p), mapped twice, or not mapped at all.
  * Reference: every row of the full-batch outputs is within oracle.net.PARITY_TOL["f32"] (5e-5 in logit space, the tolerance of
    tests/test_gpu_net_parity.py) of the float64 torch reference of its position.
A forward of the same size on other positions runs first, so a workgroup that never ran cannot leave correct values behind."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K = 40
_setups = {}


def _setup(S, F):
    if (S, F) not in _setups:
        import torch
        from oracle.net import parity_tower, reference
        from tests.test_net_reference import parity_positions
        torch.set_num_threads(16)
        x = parity_positions(S, K, 100 + S)
        net = parity_tower(S, 10, F, 2, 200 + F, x)
        _setups[(S, F)] = dict(net=net, x=x, ref=reference(net, x, "f64"), alt=parity_positions(S, K + 2, 900 + S))
    return _setups[(S, F)]


@pytest.mark.parametrize("S,F,n", [(9, 128, 1), (9, 128, 130), (9, 128, 1024), (9, 128, 1100), (9, 128, 2200), (19, 128, 130), (9, 256, 1100)])
def test_full_batch_equals_chunks_of_100_and_the_float64_reference(S, F, n):
    from oracle.net import PARITY_TOL, parity_error
    from transgo_amd.model import HipNetwork
    st = _setup(S, F)
    x, alt = st["x"], st["alt"]
    ids = np.random.RandomState(n).permutation(np.arange(n) % x.shape[0])
    h = HipNetwork(S, 10, F, 2, rows_cap=n, precision="f32")
    try:
        h.set_weights({k: v.detach().numpy() for k, v in st["net"].state_dict().items()})
        h.main_prediction(alt[np.random.RandomState(n + 1).randint(0, alt.shape[0], n)])
        full = [np.array(a) for a in h.main_prediction(x[ids])]
        parts = [h.main_prediction(x[ids[i:i + 100]]) for i in range(0, n, 100)]
        for k, a in enumerate(full):
            b = np.concatenate([np.asarray(p[k]) for p in parts])
            assert a.shape == b.shape
            diff = np.flatnonzero((a != b).reshape(n, -1).any(1))
            assert diff.size == 0, f"S={S} F={F} n={n}: output {k} differs from the chunked evaluation on {diff.size} boards, first {diff[:8]}"
        err, per = parity_error(full, [r[ids] for r in st["ref"]])
        print(f"\nS={S} F={F} n={n}: max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} own {per[2]:.1e}), "
              f"tolerance {PARITY_TOL['f32']:.0e}")
        assert err < PARITY_TOL["f32"]
    finally:
        h.ctx.close()
