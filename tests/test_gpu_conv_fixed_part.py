"""k_conv3x3_sg with the shortened fixed part of a workgroup (transgo_amd/csrc/net.hip, template parameter FP): bias | s2 | t2 fetched
beside the weight DMAs, the first barrier waiting for the weight stages 0 and 1 only, stages 2 and 3 issued behind the first consumer
of the B fragments and the residual, and conv2's fragment hand-over at the end of the stage.  TG_CONV_FIXED_PART=0 (read when the
network is loaded, like TG_ONE_STREAM) selects the prologue this replaced, which is the reference here.

Per case, through tg_net_predict (transgo_amd.model.HipNetwork) with oracle.net's parity weights and real 0/1 planes:
  1. policy, value and ownership are BITWISE equal to the same library run with TG_CONV_FIXED_PART=0 -- no accumulation changes
     its order, only when its operands are fetched;
  2. they are within oracle.net.PARITY_TOL["f32"] of the float64 reference network in logit space, the tolerance of
     tests/test_gpu_conv_row_order.py.
Each arm runs in a fresh child process; every checked forward follows one of the same size on other positions, so a skipped tile
cannot leave correct values behind.

Shapes: 9x9 / F = 128 / 2 blocks with 130 boards (two ranges, the second with 2 boards: one wave partly present, three absent) and
with 16 and 17 boards (the tile boundary); F = 256, 1 block, 17 boards; 19x19 / F = 128, 1 block, 5 boards."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 40
# (id, S, F, blocks, board counts)
CASES = [
    ("9x9-F128", 9, 128, 2, (130, 16, 17)),
    ("9x9-F256", 9, 256, 1, (17,)),
    ("19x19-F128", 19, 128, 1, (5,)),
]


def _ids(n, k):
    return np.random.RandomState(n).permutation(np.arange(max(n, k)) % k)[:n]


def _worker(inp, outp):
    """Child process: load the network (TG_CONV_FIXED_PART is read here) and run every board count; no torch, no oracle."""
    sys.path.insert(0, ROOT)
    from transgo_amd.model import HipNetwork
    d = np.load(inp)
    S, F, NB = int(d["S"]), int(d["F"]), int(d["NB"])
    counts = [int(n) for n in d["counts"]]
    x, alt = d["x"], d["alt"]
    sd = {k[2:]: d[k] for k in d.files if k.startswith("w:")}
    h = HipNetwork(S, 10, F, NB, rows_cap=max(counts), precision="f32")
    h.set_weights(sd)
    fn = h.ctx.lib.tg_net_conv_fixed_part
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    fp = ctypes.c_int(-1)
    h.ctx.call("tg_net_conv_fixed_part", ctypes.byref(fp))
    out = {"fixed_part": np.array(fp.value)}
    try:
        for n in counts:
            h.main_prediction(alt[np.random.RandomState(n + 1).randint(0, alt.shape[0], n)])
            for name, a in zip(("policy", "value", "own"), h.main_prediction(x[_ids(n, x.shape[0])])):
                out[f"{name}:{n}"] = np.asarray(a)
    finally:
        h.ctx.close()
    np.savez(outp, **out)


def _arm(inp, outp, fixed_part):
    env = dict(os.environ)
    for v in ("TG_CONV_FIXED_PART", "TG_ONE_STREAM", "TG_DMA_CONV"):
        env.pop(v, None)
    if fixed_part is not None:
        env["TG_CONV_FIXED_PART"] = fixed_part
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(inp), str(outp)], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, f"TG_CONV_FIXED_PART={fixed_part}: child failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(outp)


@pytest.mark.parametrize("case,S,F,NB,counts", CASES, ids=[c[0] for c in CASES])
def test_fixed_part_bit_equal_to_earlier_prologue_and_within_f32_parity(case, S, F, NB, counts, tmp_path):
    import torch
    from oracle.net import PARITY_TOL, parity_error, parity_tower, reference
    from tests.test_net_reference import parity_positions
    torch.set_num_threads(16)
    x = parity_positions(S, K, 100 + S)
    net = parity_tower(S, 10, F, NB, 200 + F, x)
    ref = reference(net, x, "f64")
    inp = tmp_path / "in.npz"
    np.savez(inp, S=S, F=F, NB=NB, counts=np.array(counts), x=x, alt=parity_positions(S, K + 2, 900 + S),
             **{"w:" + k: v.detach().numpy() for k, v in net.state_dict().items()})
    new = _arm(inp, tmp_path / "new.npz", None)
    old = _arm(inp, tmp_path / "old.npz", "0")
    assert int(new["fixed_part"]) == 1 and int(old["fixed_part"]) == 0      # the arms really ran different kernels
    for n in counts:
        ids = _ids(n, x.shape[0])
        got = [new[f"{name}:{n}"] for name in ("policy", "value", "own")]
        for name, a in zip(("policy", "value", "own"), got):
            b = old[f"{name}:{n}"]
            assert a.shape == b.shape and a.shape[0] == n
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                f"{case} n={n}: {name} differs from TG_CONV_FIXED_PART=0 in {int((a.view(np.uint32) != b.view(np.uint32)).sum())} elements, max |d| {np.abs(a - b).max():.2e}"
        err, per = parity_error(got, [r[ids] for r in ref])
        print(f"\n{case} n={n}: bit-equal to the earlier prologue; max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} "
              f"own {per[2]:.1e}), tolerance {PARITY_TOL['f32']:.0e}")
        assert err < PARITY_TOL["f32"], f"{case} n={n}"


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
