// sym_dev.h -- the eight dihedral symmetries of the board, shared by the replay sampler (replay.hip) and the evaluator's
// symmetry wrapper (symmetry.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace tg {

// symmetry s = 2*(i-1) + f for the reference's loop "for i in 1..4: rot90(x, i); then fliplr of that" (self_play.py:944-965).
// Returns the SOURCE point of destination (r, c).  np.rot90(m, k)[r][c]: k=1: m[c][S-1-r]; k=2: m[S-1-r][S-1-c];
// k=3: m[S-1-c][r]; k=4: m[r][c].  fliplr(y)[r][c] = y[r][S-1-c].
__device__ __forceinline__ int sym_src(int s, int r, int c, int S) {
    const int k = (s >> 1) + 1, f = s & 1;
    if (f) c = S - 1 - c;
    int rr, cc;
    switch (k & 3) {
        case 1: rr = c; cc = S - 1 - r; break;
        case 2: rr = S - 1 - r; cc = S - 1 - c; break;
        case 3: rr = S - 1 - c; cc = r; break;
        default: rr = r; cc = c; break;
    }
    return rr * S + cc;
}

}  // namespace tg
