"""Where a workgroup of k_conv3x3_sg<9,128> spends its time outside the walk, from in-kernel cycle-counter stamps (diagnostic build:
net.hip with -DTG_CONV_STAMP, `scripts/build_variant.sh cstamp net.hip -DTG_CONV_STAMP`, copied over transgo_amd/libtransgo_hip.so on
the GPU box; the shipped library has no stamp).  `python scripts/stamp_conv.py [rows blocks]`: forwards of a 9x9 / F = 128 tower as
scripts/time_net.py runs them; the stamps are those of lane 0 of wave 0 of six workgroups of XCD 0 in the last conv1 launch and the
last stream-to-stream conv2 launch: the first interior, edge and corner position of board range 0 (first round) and of range 7 (the
middle of the XCD's run).  Read the SHARES: the stamps fence the scheduler, the build is slower than the product."""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transgo_amd import _lib
from transgo_amd.model import HipNetwork, random_weights

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
NB = int(sys.argv[2]) if len(sys.argv) > 2 else 6
h = HipNetwork(9, 10, 128, NB, rows_cap=B, precision="f32")
h.set_weights(random_weights(9, 10, 128, NB))
x = (np.random.RandomState(0).rand(B, 10, 9, 9) < 0.2).astype(np.float32)
h.main_prediction(x[:256])
h.ctx.call("tg_prof_enable", 1, 4096)
for _ in range(3):
    h.main_prediction(x)
ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
h.ctx.call("tg_prof_read", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
fn = _lib.load().tg_debug_conv_stamps
fn.restype = ctypes.c_int; fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
out = (ctypes.c_ulonglong * 96)()
assert fn(out, 96) == 0
s = np.array([int(v) for v in out], dtype=np.int64).reshape(2, 2, 3, 8)           # [EPI][round][class][phase]
# The unit is the tick of __builtin_readcyclecounter.  It is NOT the 10 ns of s_memrealtime: an interior workgroup's walk of 72 stages
# reads ~480 k ticks while a launch of 9936 workgroups on 1024 slots takes ~2.4 ms (~250 us per workgroup), about 0.5 ns per tick.
print(f"rows {B}, blocks {NB}; stamped build: "
      f"{n.value} conv launches, {ms.value / n.value:.3f} ms on average (not the product's time)")
names = ["entry -> bias (|s2|t2) issued", "-> weight DMAs of the prologue issued", "-> first counted wait + barrier passed",
         "-> first MFMAs issued (B fragments, residual landed)", "-> last MFMA issued (all stores but the last tile's are out)",
         "-> the last cout tile's stores issued", "-> stores written"]
for e, kern in enumerate(("conv1 <9,128,0,SIN>", "conv2 <9,128,1,SIN,SOUT>")):
    for r, rnd in enumerate(("first round (range 0)", "middle round (range 7)")):
        print(f"{kern}, {rnd}: ticks per phase (share of the workgroup) for interior | edge | corner")
        d = np.diff(s[e, r], axis=1).astype(float)                                       # [class][7 phases]
        for i, nm in enumerate(names):
            print(f"  {nm:62s} " + " | ".join(f"{d[c, i]:8.0f} ({100 * d[c, i] / d[c].sum():4.1f} %)" for c in range(3)))
        fixed = d[:, :4].sum(1) + d[:, 5:].sum(1)
        print(f"  {'fixed part = everything but the walk':62s} " + " | ".join(f"{fixed[c]:8.0f} ({100 * fixed[c] / d[c].sum():4.1f} %)" for c in range(3)))
