"""The f32 DMA chain (transgo_amd/csrc/net.hip, CHAIN_DMA), pinned to the two run-time arms it once had.  Both were environment
variables that kept a second copy of the hot path compiling; both computed the same bits as the default, and
tests/golden/conv_arms.json (tests/golden/gen_conv_arms.py) holds the SHA-256 of what both arms gave, each recorded on the last
commit that had its arm:
  fixed-part/...   k_conv3x3_sg's earlier prologue (TG_CONV_FIXED_PART=0, commit be131a0).  The
                   kernel fetches its per-channel parameters beside its weight DMAs, waits at its first barrier for weight stages 0
                   and 1 only, issues stages 2 and 3 behind the first consumer of the B fragments and the residual, and hands
                   conv2's fragments over at the end of the stage.
  one-stream/...   the two-tensor chain (TG_ONE_STREAM=0, commit bf253ad): a row-major f32
                   stream plus a pre-activated slice-major copy behind every producer, written by a second output of both f32 conv
                   kernels.  Today, between two conv layers, the stem / k_conv3x3_sg's second conv write only the slice-major
                   board-grouped stream, the next block's first conv applies relu(bn1(.)) to its B fragments as they land and its
                   second conv starts its accumulators from the stream -- the multiply, add and maximum the producer's epilogue
                   applied, on the same f32 values, every output element accumulating the same terms in the same order.

Per case, through tg_net_predict (transgo_amd.model.HipNetwork) with oracle.net's parity weights and real 0/1 planes:
  1. the raw bytes of policy, value and ownership have the recorded digest: BITWISE what the retired arm computed;
  2. they are within oracle.net.PARITY_TOL["f32"] of the float64 reference network in logit space, the tolerance of
     tests/test_gpu_conv_row_order.py and tests/test_gpu_net_parity.py;
  3. tg_net_stream_layout reports one stream, and the pre-activated copy only in the MainNetwork (for the residual blocks behind
     its attention layers), never in a tower.
The library runs in a fresh child process; every checked forward follows one of the same size on other positions, so a skipped
tile cannot leave correct values behind.  The two head scales that oracle.net.parity_weights calibrates with an f32 forward (not
the same bits on every machine) are the recorded ones; everything else is generated here.  test_recorded_inputs_are_reproduced
(no GPU) holds the weights and positions to the recording, so that a drift in their generators reads "inputs differ" and not
"kernel regression", and the recorded scales to what the calibration gives here.

Shapes, fixed-part: 9x9 / F = 128 / 2 blocks with 130 boards (two ranges, the second with 2 boards: one wave partly present, three
absent) and with 16 and 17 boards (the tile boundary); F = 256, 1 block, 17 boards; 19x19 / F = 128, 1 block, 5 boards.
Shapes, one-stream: board counts straddle the layout's seams: the group of 16 boards (15, 16, 17), the workgroup's range of 128
(127, 128, 129), two ranges plus one board (257), and 1.  Absent boards of a partial group sit next to present ones in every count
that is no multiple of 16.  The 3-block tower has a middle block whose neighbours on both sides share the single stream; the
MainNetwork case runs the layers around Self_Attention, which keep two tensors, next to residual runs that do not."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_arms.json")
K = 40
OUTPUTS = ("policy", "value", "own")
ALL = (1, 15, 16, 17, 127, 128, 129, 257)
# (id, network, S, F, blocks, board counts)
CASES = [
    ("fixed-part/9x9-F128", "tower", 9, 128, 2, (130, 16, 17)),
    ("fixed-part/9x9-F256", "tower", 9, 256, 1, (17,)),
    ("fixed-part/19x19-F128", "tower", 19, 128, 1, (5,)),
    ("one-stream/9x9-F128", "tower", 9, 128, 2, ALL),
    ("one-stream/9x9-F256", "tower", 9, 256, 2, ALL),
    ("one-stream/19x19-F128", "tower", 19, 128, 2, (1, 17, 129)),
    ("one-stream/9x9-F128-3blocks", "tower", 9, 128, 3, (17, 129)),
    ("one-stream/9x9-mainnetwork", "mainnet", 9, 128, 0, (17,)),
]
case_params = pytest.mark.parametrize("case,kind,S,F,NB,counts", CASES, ids=[c[0] for c in CASES])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _ids(n, k):
    return np.random.RandomState(n).permutation(np.arange(max(n, k)) % k)[:n]


def layout(kind):
    """What tg_net_stream_layout reports: one stream; the pre-activated copy only behind the MainNetwork's attention layers."""
    return [1, 1 if kind == "mainnet" else 0]


def inputs(kind, S, F, NB, head_scales=None):
    """The case's positions, the other positions run in front of every checked forward, and its network (head scales calibrated on
    the positions, or the given pair)."""
    from oracle.net import parity_tower, parity_transgo
    from tests.test_net_reference import parity_positions
    x = parity_positions(S, K, 100 + S)
    net = parity_tower(S, 10, F, NB, 200 + F, x, head_scales) if kind == "tower" else parity_transgo(S, 10, F, 300 + F, x, head_scales)
    return x, parity_positions(S, K + 2, 900 + S), net


def input_digests(kind, S, F, NB, x, alt, net):
    from transgo_amd.model import pack_weights, transgo_arch
    blob = pack_weights(net.state_dict(), S, 10, F, NB, arch=transgo_arch() if kind == "mainnet" else None)
    return {"weights": sha(blob), "x": sha(x), "alt": sha(alt)}


def _worker(inp, outp):
    """Child process: load the network and run every board count; no torch, no oracle."""
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
            for name, a in zip(OUTPUTS, h.main_prediction(x[_ids(n, x.shape[0])])):
                out[f"{name}:{n}"] = np.asarray(a)
    finally:
        h.ctx.close()
    np.savez(outp, **out)


def run_child(tmp, kind, S, F, NB, counts, x, alt, net, env=()):
    """The worker in a fresh process, on the library's default path (but for `env`: the recording scripts select their arms there)."""
    inp, outp = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
    np.savez(inp, kind=kind, S=S, F=F, NB=NB, counts=np.array(counts), x=x, alt=alt,
             **{"w:" + k: v.detach().numpy() for k, v in net.state_dict().items()})
    e = {k: v for k, v in os.environ.items() if k not in ("TG_DMA_CONV", "TG_ONE_STREAM")}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), inp, outp], env=e, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, f"{dict(env)}: child failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(outp)


@case_params
def test_recorded_inputs_are_reproduced(case, kind, S, F, NB, counts):
    rec = json.load(open(FIXTURE))["cases"][case]
    got = input_digests(kind, S, F, NB, *inputs(kind, S, F, NB, rec["inputs"]["head_scales"]))
    assert sorted(int(n) for n in rec["outputs"]) == sorted(counts), f"{case}: board counts differ from the recording"
    for name in ("weights", "x", "alt"):
        assert got[name] == rec["inputs"][name], f"{case}: {name} differ from the recording (generator drift, not a kernel regression)"
    # the recorded scales are what the calibration measures: an f32 forward is within PARITY_TOL["f32"] = 5e-5 of float64 on logits
    # whose calibrated spread is at least 2, so two machines' scales agree to a few 1e-5; 1e-3 leaves room and still catches a
    # calibration on other positions or weights
    here = inputs(kind, S, F, NB)[2].head_scales
    assert np.allclose(here, rec["inputs"]["head_scales"], rtol=1e-3, atol=0), (case, here, rec["inputs"]["head_scales"])


@pytest.mark.gpu
@case_params
def test_bit_equal_to_recorded_arms_and_within_f32_parity(case, kind, S, F, NB, counts, tmp_path):
    import torch
    from oracle.net import PARITY_TOL, parity_error, reference
    torch.set_num_threads(16)
    rec = json.load(open(FIXTURE))["cases"][case]
    x, alt, net = inputs(kind, S, F, NB, rec["inputs"]["head_scales"])
    assert input_digests(kind, S, F, NB, x, alt, net) == {k: rec["inputs"][k] for k in ("weights", "x", "alt")}, \
        f"{case}: inputs differ from the recording"
    ref = reference(net, x, "f64")
    got_all = run_child(str(tmp_path), kind, S, F, NB, counts, x, alt, net)
    assert list(got_all["layout"]) == layout(kind), list(got_all["layout"])
    for n in counts:
        ids = _ids(n, x.shape[0])
        got = [got_all[f"{name}:{n}"] for name in OUTPUTS]
        for name, a in zip(OUTPUTS, got):
            assert a.dtype == np.float32 and a.shape[0] == n
            assert sha(a) == rec["outputs"][str(n)][name], f"{case} n={n}: {name} is not bitwise what the retired arms computed"
        err, per = parity_error(got, [r[ids] for r in ref])
        print(f"\n{case} n={n}: bit-equal to the recorded arms; max logit-space error {err:.2e} (policy {per[0]:.1e} value {per[1]:.1e} "
              f"own {per[2]:.1e}), tolerance {PARITY_TOL['f32']:.0e}")
        assert err < PARITY_TOL["f32"], f"{case} n={n}"


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
