"""k_conv3x3_sg's last stage (transgo_amd/csrc/net.hip) issues every cout tile's bias / ReLU and stores between the MFMAs of the next
tile, as bounds-checked buffer stores whose offset drops the boards past the batch, and no barrier closes the walk.
tests/test_gpu_conv_arms_pinned.py holds the bits of 9x9 (F = 128, 256) and of 19x19 / F = 128; this file covers what no digest pins:

  1. 19x19 / F = 256 / 1 block at 1 and 17 boards against the float64 reference network, within oracle.net.PARITY_TOL["f32"] in
     logit space (the tolerance of tests/test_gpu_net_parity.py);
  2. row independence under the interleaved stores: the same positions evaluated in one forward and again in smaller forwards
     (9x9 / F = 128 / 2 blocks: 129 boards against 16 + 17 + 1; F = 256 / 1 block: 17 against 16 + 1) give the same BYTES of policy,
     value and ownership per board.  A board's outputs depend on its own rows only, and every element accumulates the same terms in
     the same order whatever tile, wave, workgroup or range its board falls into; a store that lands in a neighbour's row, is
     dropped for a present board or is not dropped for an absent one shows as a difference.

The library runs in a fresh child process without torch; every checked forward follows one of the same size on other positions, so
a skipped store cannot leave correct values behind.  Weights are oracle.net.parity_tower's, planes tests.test_net_reference's
parity_positions, as in the pinned test."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("policy", "value", "own")


def _worker(inp, outp):
    """Child process: load the tower and evaluate x[lo:hi] for every span, each behind a forward of as many other positions."""
    sys.path.insert(0, ROOT)
    from transgo_amd.model import HipNetwork
    d = np.load(inp)
    S, F, NB = int(d["S"]), int(d["F"]), int(d["NB"])
    x, alt = d["x"], d["alt"]
    spans = [(int(lo), int(hi)) for lo, hi in d["spans"]]
    sd = {k[2:]: d[k] for k in d.files if k.startswith("w:")}
    h = HipNetwork(S, 10, F, NB, rows_cap=max(hi - lo for lo, hi in spans), precision="f32")
    h.set_weights(sd)
    out = {}
    try:
        for lo, hi in spans:
            h.main_prediction(alt[np.random.RandomState(hi).randint(0, alt.shape[0], hi - lo)])
            for name, a in zip(OUTPUTS, h.main_prediction(x[lo:hi])):
                out[f"{name}:{lo}:{hi}"] = np.asarray(a)
    finally:
        h.ctx.close()
    np.savez(outp, **out)


def run_child(tmp, S, F, NB, spans, x, alt, net):
    inp, outp = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
    np.savez(inp, S=S, F=F, NB=NB, spans=np.array(spans), x=x, alt=alt,
             **{"w:" + k: v.detach().numpy() for k, v in net.state_dict().items()})
    e = {k: v for k, v in os.environ.items() if k not in ("TG_DMA_CONV", "TG_ONE_STREAM")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), inp, outp], env=e, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, f"child failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    got = np.load(outp)
    return {(lo, hi): [got[f"{name}:{lo}:{hi}"] for name in OUTPUTS] for lo, hi in spans}


def inputs(S, F, NB, k):
    """k + 2 positions, as many other ones, and the tower with its head scales calibrated on (at most 40 of) the positions."""
    import torch
    from oracle.net import parity_tower
    from tests.test_net_reference import parity_positions
    torch.set_num_threads(16)
    x = parity_positions(S, k, 100 + S)
    return x, parity_positions(S, k, 900 + S), parity_tower(S, 10, F, NB, 200 + F, x[:40])


@pytest.mark.gpu
def test_19x19_f256_within_f32_parity_of_float64(tmp_path):
    from oracle.net import PARITY_TOL, parity_error, reference
    S, F, NB = 19, 256, 1
    x, alt, net = inputs(S, F, NB, 15)
    assert x.shape[0] == 17
    ref = reference(net, x, "f64")
    spans = [(0, 1), (0, 17)]
    got = run_child(str(tmp_path), S, F, NB, spans, x, alt, net)
    for lo, hi in spans:
        for a in got[(lo, hi)]:
            assert a.dtype == np.float32 and a.shape[0] == hi - lo
        err, per = parity_error(got[(lo, hi)], [r[lo:hi] for r in ref])
        print(f"\n19x19 F=256 boards {hi - lo}: max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} own {per[2]:.1e}), "
              f"tolerance {PARITY_TOL['f32']:.0e}")
        assert err < PARITY_TOL["f32"], (lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("F,NB,whole,parts", [(128, 2, (0, 129), [(0, 16), (16, 33), (128, 129)]), (256, 1, (0, 17), [(0, 16), (16, 17)])],
                         ids=["9x9-F128-129-vs-16+17+1", "9x9-F256-17-vs-16+1"])
def test_rows_do_not_depend_on_the_batch_they_sit_in(F, NB, whole, parts, tmp_path):
    S = 9
    x, alt, net = inputs(S, F, NB, whole[1] - 2)
    assert x.shape[0] == whole[1] and alt.shape[0] == whole[1]
    got = run_child(str(tmp_path), S, F, NB, [whole] + parts, x, alt, net)
    big = got[whole]
    assert all(np.isfinite(a).all() for a in big)
    # the checked forwards are not degenerate: the boards' outputs differ from one another
    assert len({a.tobytes() for a in big[0]}) == whole[1]
    for lo, hi in parts:
        for name, a, b in zip(OUTPUTS, big, got[(lo, hi)]):
            assert b.dtype == np.float32 and b.shape[0] == hi - lo
            differ = [lo + i for i in range(hi - lo) if a[lo + i].tobytes() != b[i].tobytes()]
            assert not differ, f"F={F}: {name} of boards {differ} differs between the forward of {whole[1]} and the one of {hi - lo}"


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
