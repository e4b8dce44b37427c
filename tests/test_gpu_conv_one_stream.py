"""f32 DMA chain with ONE residual stream in the conv's row order (transgo_amd/csrc/net.hip, CHAIN_DMA): between two conv layers the
stem / k_conv3x3_sg's second conv write only the slice-major board-grouped stream, the next block's first conv applies
relu(bn1(.)) to its B fragments as they land and its second conv starts its accumulators from the stream.  TG_ONE_STREAM=0
selects the chain this replaced (row-major f32 stream plus a pre-activated slice-major copy), which is the reference here.

Per case, through tg_net_predict (transgo_amd.model.HipNetwork) with oracle.net's parity weights and real 0/1 planes:
  1. policy, value and ownership are BITWISE equal to the same library run with TG_ONE_STREAM=0 -- the activation on load is the
     multiply, add and maximum the producer's epilogue applied, on the same f32 values, and every output element accumulates the
     same terms in the same order;
  2. they are within oracle.net.PARITY_TOL["f32"] of the float64 reference network in logit space, as tests/test_gpu_net_parity.py
     checks it.
Each arm runs in a fresh child process (the variable is read when the network is loaded); every checked forward follows one of the
same size on other positions, so a skipped tile cannot leave correct values behind.

Board counts straddle the layout's seams: the group of 16 boards (15, 16, 17), the workgroup's range of 128 (127, 128, 129), two
ranges plus one board (257), and 1.  Absent boards of a partial group sit next to present ones in every count that is no multiple
of 16.  The 3-block tower has a middle block whose neighbours on both sides share the single stream; the MainNetwork case runs the
layers around Self_Attention, which keep two tensors, next to residual runs that do not."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 40
ALL = (1, 15, 16, 17, 127, 128, 129, 257)
# (id, kind, S, F, blocks, board counts)
CASES = [
    ("9x9-F128", "tower", 9, 128, 2, ALL),
    ("9x9-F256", "tower", 9, 256, 2, ALL),
    ("19x19-F128", "tower", 19, 128, 2, (1, 17, 129)),
    ("9x9-F128-3blocks", "tower", 9, 128, 3, (17, 129)),
    ("9x9-mainnetwork", "mainnet", 9, 128, 0, (17,)),
]


def _ids(n, k):
    return np.random.RandomState(n).permutation(np.arange(max(n, k)) % k)[:n]


def _worker(inp, outp):
    """Child process: load the network (TG_ONE_STREAM is read here) and run every board count; no torch, no oracle."""
    sys.path.insert(0, ROOT)
    from transgo_amd.model import HipNetwork, transgo_arch
    d = np.load(inp)
    kind, S, F, NB = str(d["kind"]), int(d["S"]), int(d["F"]), int(d["NB"])
    counts = [int(n) for n in d["counts"]]
    x, alt = d["x"], d["alt"]
    sd = {k[2:]: d[k] for k in d.files if k.startswith("w:")}
    h = HipNetwork(S, 10, F, NB, rows_cap=max(counts), precision="f32", arch=transgo_arch() if kind == "mainnet" else None)
    h.set_weights(sd)
    one, act = ctypes.c_int(-1), ctypes.c_int(-1)
    h.ctx.call("tg_net_stream_layout", ctypes.byref(one), ctypes.byref(act))
    out = {"layout": np.array([one.value, act.value])}
    try:
        for n in counts:
            h.main_prediction(alt[np.random.RandomState(n + 1).randint(0, alt.shape[0], n)])
            for name, a in zip(("policy", "value", "own"), h.main_prediction(x[_ids(n, x.shape[0])])):
                out[f"{name}:{n}"] = np.asarray(a)
    finally:
        h.ctx.close()
    np.savez(outp, **out)


def _arm(inp, outp, one_stream):
    env = dict(os.environ)
    env.pop("TG_ONE_STREAM", None)
    env.pop("TG_DMA_CONV", None)
    if one_stream is not None:
        env["TG_ONE_STREAM"] = one_stream
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(inp), str(outp)], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, f"TG_ONE_STREAM={one_stream}: child failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(outp)


@pytest.mark.parametrize("case,kind,S,F,NB,counts", CASES, ids=[c[0] for c in CASES])
def test_one_stream_bit_equal_to_two_tensors_and_within_f32_parity(case, kind, S, F, NB, counts, tmp_path):
    import torch
    from oracle.net import PARITY_TOL, parity_error, parity_tower, parity_transgo, reference
    from tests.test_net_reference import parity_positions
    torch.set_num_threads(16)
    x = parity_positions(S, K, 100 + S)
    net = parity_tower(S, 10, F, NB, 200 + F, x) if kind == "tower" else parity_transgo(S, 10, F, 300 + F, x)
    ref = reference(net, x, "f64")
    inp = tmp_path / "in.npz"
    np.savez(inp, kind=kind, S=S, F=F, NB=NB, counts=np.array(counts), x=x, alt=parity_positions(S, K + 2, 900 + S),
             **{"w:" + k: v.detach().numpy() for k, v in net.state_dict().items()})
    one = _arm(inp, tmp_path / "one.npz", None)
    two = _arm(inp, tmp_path / "two.npz", "0")
    # the arms really differ (tg_net_stream_layout: one_stream mode, pre-activated copy allocated): the default keeps one stream and,
    # in a pure tower, no copy; the MainNetwork keeps the copy for the residual blocks behind its attention layers
    assert list(one["layout"]) == [1, 1 if kind == "mainnet" else 0], list(one["layout"])
    assert list(two["layout"]) == [0, 1], list(two["layout"])
    for n in counts:
        ids = _ids(n, x.shape[0])
        got = [one[f"{name}:{n}"] for name in ("policy", "value", "own")]
        for name, a in zip(("policy", "value", "own"), got):
            b = two[f"{name}:{n}"]
            assert a.shape == b.shape and a.shape[0] == n
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                f"{case} n={n}: {name} differs from TG_ONE_STREAM=0 in {int((a.view(np.uint32) != b.view(np.uint32)).sum())} elements, max |d| {np.abs(a - b).max():.2e}"
        err, per = parity_error(got, [r[ids] for r in ref])
        print(f"\n{case} n={n}: bit-equal to the two-tensor chain; max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} "
              f"own {per[2]:.1e}), tolerance {PARITY_TOL['f32']:.0e}")
        assert err < PARITY_TOL["f32"], f"{case} n={n}"


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
