"""Recording of what the retired prologue of k_conv3x3_sg computed (tests/golden/conv_arms.json, read by
tests/test_gpu_conv_arms_pinned.py).  Run by hand, ONCE, on the GPU, on the LIBRARY of commit be131a0 -- the last one that has the
arm TG_CONV_FIXED_PART=0 (k_conv3x3_sg's earlier prologue) -- under the Python of the commit that added this script: it imports the
pinned test's cases, inputs and worker, and oracle.net's head_scales, which be131a0 does not have.  To repeat it: build
transgo_amd/libtransgo_hip.so at be131a0 (make -C transgo_amd/csrc), check out this script's commit without rebuilding, run it.  On
a later library it refuses to run: tg_net_conv_fixed_part is gone.

    python tests/golden/gen_conv_arms.py [OUTPUT, default tests/golden/conv_arms.json]

For every case and board count of the test, with the test's own weights, positions and worker: the default arm and the old arm
each run in a fresh child process, each must report the layout / prologue it was asked for and both must be bitwise equal, or
nothing is written.  The file holds digests only (SHA-256 of the packed weight blob, of the x and alt planes, and of the
raw bytes of policy, value and own per board count); the arrays and weights are too large to commit.  Beside them it holds the two
head scales that oracle.net.parity_weights calibrated on this machine: with them the test rebuilds the same weights bit for bit on
any other."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import test_gpu_conv_arms_pinned as T  # noqa: E402

COMMIT = "be131a0"
# arm -> (environment, tg_net_conv_fixed_part)
ARMS = {
    "default": ({}, 1),
    "TG_CONV_FIXED_PART=0": ({"TG_CONV_FIXED_PART": "0"}, 0),
}


def fixed_part_worker(outp):
    """Child process: which prologue a loaded f32 network runs (read from the environment at the load)."""
    from transgo_amd.model import HipNetwork, random_weights
    h = HipNetwork(9, 10, 128, 1, rows_cap=16, precision="f32")
    h.set_weights(random_weights(9, 10, 128, 1, seed=1))
    fn = h.ctx.lib.tg_net_conv_fixed_part
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    fp = ctypes.c_int(-1)
    h.ctx.call("tg_net_conv_fixed_part", ctypes.byref(fp))
    h.ctx.close()
    json.dump(fp.value, open(outp, "w"))


def fixed_part(tmp, env):
    e = dict(os.environ, **env)
    outp = os.path.join(tmp, "fp.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--fixed-part", outp], env=e, cwd=ROOT, check=True)
    return json.load(open(outp))


def main():
    from transgo_amd import _lib
    for v in ("TG_DMA_CONV", "TG_ONE_STREAM", "TG_CONV_FIXED_PART"):    # every arm starts from the default path
        os.environ.pop(v, None)
    if not hasattr(_lib.load(), "tg_net_conv_fixed_part"):
        sys.exit(f"gen_conv_arms.py: this library has no tg_net_conv_fixed_part, so the arm it records is gone; "
                 f"build the library of {COMMIT} to record again (see the header)")
    rec = {"recorded_at": COMMIT,
           "note": f"SHA-256 digests; recorded on the library of {COMMIT} under the Python of the commit that added "
                   "tests/golden/gen_conv_arms.py; every output was bitwise equal in the arms " + ", ".join(ARMS),
           "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for arm, (env, want) in ARMS.items():
            got = fixed_part(tmp, env)
            assert got == want, f"{arm}: tg_net_conv_fixed_part says {got}, expected {want}"
    for case, S, F, NB, counts in T.CASES:
        x, alt, net = T.inputs(S, F, NB)
        arms = list(ARMS)
        with tempfile.TemporaryDirectory() as tmp:
            got = {}
            for arm in arms:
                os.makedirs(os.path.join(tmp, arm))
                got[arm] = T.run_child(os.path.join(tmp, arm), S, F, NB, counts, x, alt, net, env=ARMS[arm][0])
                assert list(got[arm]["layout"]) == [1, 0], f"{case} {arm}: layout {list(got[arm]['layout'])}"
            outputs = {}
            for n in counts:
                outputs[str(n)] = {}
                for name in T.OUTPUTS:
                    a = got["default"][f"{name}:{n}"]
                    assert a.dtype == np.float32 and a.shape[0] == n
                    for arm in arms[1:]:
                        b = got[arm][f"{name}:{n}"]
                        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                            f"{case} n={n}: {name} of {arm} differs from the default arm; nothing written"
                    outputs[str(n)][name] = T.sha(a)
        rec["cases"][case] = {"arms": arms, "outputs": outputs,
                              "inputs": dict(T.input_digests(S, F, NB, x, alt, net), head_scales=list(net.head_scales))}
        print(case, "arms", arms, "bitwise equal at", list(counts), flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", f.name, os.path.getsize(f.name), "bytes")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--fixed-part"]:
        fixed_part_worker(sys.argv[2])
    else:
        main()
