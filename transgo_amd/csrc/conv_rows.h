// conv_rows.h -- row order of the slice-major f32 activation tensors and the tap walk of k_conv3x3_sg (net.hip).
// Plain constexpr C++ without HIP dependencies: the device code includes it, and tests/test_conv_row_order.py compiles it with g++.
//
// A slice-major tensor is [F/16 slices][rows][16 channels].  Its rows are BOARD-GROUPED: inside a group of 16 boards they run
// position-major, row = ((b >> 4) * P + p) * 16 + (b & 15) for board b, position p.  The 16 columns of one MFMA are then the same
// position on 16 boards, so whether a 3x3 tap falls on the board is the same for all of them (a scalar), and a tap (dy, dx) is a
// shift of (dy * S + dx) * 16 rows that never leaves the group.  The tensor holds ceil(boards / 16) * 16 * P rows; the rows of the
// absent boards of the last group are never written.
#pragma once

namespace tg {

constexpr int conv_sg_rows(int boards, int P) { return ((boards + 15) >> 4) * 16 * P; }
constexpr int conv_sg_row(int b, int p, int P) { return ((b >> 4) * P + p) * 16 + (b & 15); }

// bit tap = (dy + 1) * 3 + (dx + 1) is set where the neighbour (y + dy, x + dx) of position p lies on the SxS board
constexpr unsigned conv_tap_mask(int p, int S) {
    const int x = p % S, y = p / S;
    unsigned mk = 0;
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy >= 0 && yy < S && xx >= 0 && xx < S) mk |= 1u << tap;
    }
    return mk;
}
constexpr int conv_tap_count(unsigned mask) {
    int n = 0;
    for (int tap = 0; tap < 9; ++tap) n += (mask >> tap) & 1;
    return n;
}
// the on-board taps of a mask in ascending order, 4 bits each (the kernel walks them with a scalar shift)
constexpr unsigned long long conv_tap_list(unsigned mask) {
    unsigned long long l = 0;
    int k = 0;
    for (int tap = 0; tap < 9; ++tap)
        if ((mask >> tap) & 1) { l |= (unsigned long long)tap << (4 * k); ++k; }
    return l;
}

// Order in which the workgroups of one board range take the positions: longest walk first -- the (S-2)^2 interior positions
// (9 taps), then the 4(S-2) edge positions (6), then the corners (4).  A bijection of [0, S*S).
constexpr int conv_pos_of(int idx, int S) {
    const int I = S - 2;
    if (idx < I * I) return (1 + idx / I) * S + 1 + idx % I;
    const int e = idx - I * I;
    if (e < 4 * I) {
        const int side = e / I, k = 1 + e % I;
        return side == 0 ? k : side == 1 ? (S - 1) * S + k : side == 2 ? k * S : k * S + S - 1;
    }
    const int c = e - 4 * I;
    return (c >> 1) * (S - 1) * S + (c & 1) * (S - 1);
}

}  // namespace tg
