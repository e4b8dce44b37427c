"""Recordings of what the retired run-time arms of the f32 DMA chain computed (tests/golden/conv_arms.json, read by
tests/test_gpu_conv_arms_pinned.py).  Each is run by hand, ONCE, on the GPU, on the LIBRARY of the last commit that has its arm,
under the Python of the commit that added the recording to this script: it imports the pinned test's cases, inputs and worker.

    python tests/golden/gen_conv_arms.py RECORDING [OUTPUT, default tests/golden/conv_arms.json]

  fixed-part   library of be131a0, the last with TG_CONV_FIXED_PART=0 (k_conv3x3_sg's earlier prologue).  On a later library it
               refuses to run: tg_net_conv_fixed_part is gone.
  one-stream   library of bf253ad, the last with TG_ONE_STREAM=0 (the two-tensor chain: row-major stream, pre-activated copy behind
               every producer).  A later library ignores the variable, so it refuses to run where tg_net_stream_layout does not
               report [0, 1] under it.
To repeat one: build transgo_amd/libtransgo_hip.so at its commit (make -C transgo_amd/csrc), check out this script's commit without
rebuilding, run it.  The cases of the other recordings are left in OUTPUT as they are.

For every case and board count of the test, with the test's own weights, positions and worker: the default arm and the old arm
each run in a fresh child process, each must report the layout / prologue it was asked for and both must be bitwise equal, or
nothing is written.  The file holds digests only (SHA-256 of the packed weight blob, of the x and alt planes, and of the
raw bytes of policy, value and own per board count); the arrays and weights are too large to commit.  Beside them it holds the two
head scales that oracle.net.parity_weights calibrated on the recording machine: with them the test rebuilds the same weights bit
for bit on any other.  A case listed in SAME_NETWORK takes the scales of an earlier recording's case with the same network and
positions instead, and its digests at the board counts both have must then be the ones already in the file: two recordings of one
computation."""
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

VARIABLES = ("TG_DMA_CONV", "TG_ONE_STREAM", "TG_CONV_FIXED_PART")
# recording (the prefix of its case ids) -> (commit, arm -> (environment, what probe() must report under it))
RECORDINGS = {
    "fixed-part": ("be131a0", {"default": ({}, {"fixed_part": 1, "one_stream": 1}),
                               "TG_CONV_FIXED_PART=0": ({"TG_CONV_FIXED_PART": "0"}, {"fixed_part": 0, "one_stream": 1})}),
    "one-stream": ("bf253ad", {"default": ({}, {"one_stream": 1, "act_copy": 0}),
                               "TG_ONE_STREAM=0": ({"TG_ONE_STREAM": "0"}, {"one_stream": 0, "act_copy": 1})}),
}
SAME_NETWORK = {"one-stream/9x9-F128": "fixed-part/9x9-F128"}
NOTE = ("SHA-256 digests, written by tests/golden/gen_conv_arms.py, each recording under the Python of the commit that added it to that "
        "script; every output was bitwise equal in the arms of its recording.  " +
        "  ".join(f"Cases {r}/...: library of {c}, arms {', '.join(a)}." for r, (c, a) in RECORDINGS.items()) +
        "  A case without a recorded_at of its own was recorded at the file's.")


def probe_worker(outp):
    """Child process: which prologue and which stream layout a loaded f32 tower runs (read from the environment at the load)."""
    from transgo_amd.model import HipNetwork, random_weights
    h = HipNetwork(9, 10, 128, 1, rows_cap=16, precision="f32")
    h.set_weights(random_weights(9, 10, 128, 1, seed=1))
    fp, one, act = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    if hasattr(h.ctx.lib, "tg_net_conv_fixed_part"):
        fn = h.ctx.lib.tg_net_conv_fixed_part
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        h.ctx.call("tg_net_conv_fixed_part", ctypes.byref(fp))
    h.ctx.call("tg_net_stream_layout", ctypes.byref(one), ctypes.byref(act))
    h.ctx.close()
    json.dump({"fixed_part": fp.value, "one_stream": one.value, "act_copy": act.value}, open(outp, "w"))


def probe(tmp, env):
    e = dict(os.environ, **env)
    outp = os.path.join(tmp, "probe.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--probe", outp], env=e, cwd=ROOT, check=True)
    return json.load(open(outp))


def main(recording, path):
    for v in VARIABLES:                                                  # every arm starts from the default path
        os.environ.pop(v, None)
    commit, arms = RECORDINGS[recording]
    with tempfile.TemporaryDirectory() as tmp:
        for arm, (env, want) in arms.items():
            got = probe(tmp, env)
            if any(got[k] != v for k, v in want.items()):
                sys.exit(f"gen_conv_arms.py {recording}: under the arm {arm} this library reports {got}, not {want}, so the arm it "
                         f"records is gone; build the library of {commit} to record again (see the header)")
    rec = json.load(open(path)) if os.path.exists(path) else {"recorded_at": commit, "cases": {}}
    have = [c for c in rec["cases"] if c.startswith(recording + "/")]
    if have:                                                             # a recording whose arm is gone cannot be made again
        sys.exit(f"gen_conv_arms.py {recording}: {path} already holds {have}; take them out by hand to record them again")
    names = list(arms)
    for case, kind, S, F, NB, counts in T.CASES:
        if not case.startswith(recording + "/"):
            continue
        same = rec["cases"][SAME_NETWORK[case]] if case in SAME_NETWORK else None
        x, alt, net = T.inputs(kind, S, F, NB, same and same["inputs"]["head_scales"])
        with tempfile.TemporaryDirectory() as tmp:
            got = {}
            for arm in names:
                os.makedirs(os.path.join(tmp, arm))
                got[arm] = T.run_child(os.path.join(tmp, arm), kind, S, F, NB, counts, x, alt, net, env=arms[arm][0])
                want = T.layout(kind) if arms[arm][1]["one_stream"] else [0, 1]    # two tensors: the copy behind every producer
                assert list(got[arm]["layout"]) == want, f"{case} {arm}: layout {list(got[arm]['layout'])}, expected {want}"
            outputs = {}
            for n in counts:
                outputs[str(n)] = {}
                for name in T.OUTPUTS:
                    a = got["default"][f"{name}:{n}"]
                    assert a.dtype == np.float32 and a.shape[0] == n
                    for arm in names[1:]:
                        b = got[arm][f"{name}:{n}"]
                        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                            f"{case} n={n}: {name} of {arm} differs from the default arm; nothing written"
                    outputs[str(n)][name] = T.sha(a)
        inputs = dict(T.input_digests(kind, S, F, NB, x, alt, net), head_scales=list(net.head_scales))
        if same:
            assert inputs == same["inputs"], f"{case}: inputs differ from {SAME_NETWORK[case]}"
            both = sorted(set(outputs) & set(same["outputs"]))
            assert both and all(outputs[n] == same["outputs"][n] for n in both), \
                f"{case}: digests at {both} boards differ from {SAME_NETWORK[case]}; nothing written"
            print(case, "equals", SAME_NETWORK[case], "at", both, flush=True)
        rec["cases"][case] = {"arms": names, "outputs": outputs, "inputs": inputs}
        if commit != rec["recorded_at"]:                                 # the file's own stamp is the first recording's
            rec["cases"][case]["recorded_at"] = commit
        print(case, "arms", names, "bitwise equal at", list(counts), flush=True)
    rec["note"] = NOTE
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", f.name, os.path.getsize(f.name), "bytes")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--probe"]:
        probe_worker(sys.argv[2])
    elif sys.argv[1:2] and sys.argv[1] in RECORDINGS:
        main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE)
    else:
        sys.exit(f"usage: gen_conv_arms.py {{{' | '.join(RECORDINGS)}}} [OUTPUT]")
