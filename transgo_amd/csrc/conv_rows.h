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

// ---- launch order of k_conv3x3_sg: which (board range, position) workgroup blockIdx.x is -----------------------
// Workgroup b runs on XCD b & 7 and is the (b >> 3)-th of that XCD's list.  With q = nrange / 8 whole ranges per XCD, m = nrange % 8
// leftover ranges and kd = min(K, q), the list of XCD x is
//   bulk:  its ranges x*q .. x*q + q - kd - 1, range-major, inside a range in conv_pos_of order -- the workgroups that read one
//          range's input are neighbours on one L2;
//   drain: its last kd ranges and its share of the m leftover ranges 8q .. nrange - 1, CLASS-major -- every interior position (the
//          longest walk), then every edge, then every corner; inside a class range by range, the XCD's own ranges first.  The
//          leftover workgroups, numbered class-major and inside a class range by range, are dealt out by that number mod 8.
// So every XCD's list ends on its short walks, the lists differ by at most one workgroup in every class and in total, and XCD 0
// holds the longest: the grid is 8 x its length (the count of workgroups rounded up to a multiple of 8, as it always was).
// Class c = 0 interior, 1 edge, 2 corner: a contiguous piece of conv_pos_of's index space.
constexpr int conv_class_count(int c, int S) { return c == 0 ? (S - 2) * (S - 2) : c == 1 ? 4 * (S - 2) : 4; }
constexpr int conv_class_first(int c, int S) { return c == 0 ? 0 : c == 1 ? (S - 2) * (S - 2) : (S - 2) * (S - 2) + 4 * (S - 2); }
// K, the ranges per XCD that are spent class-major, is the kernel's choice per shape: conv_drain_k in net.hip.
constexpr int conv_launch_grid(int nrange, int S) { return 8 * ((nrange >> 3) * S * S + ((nrange & 7) * S * S + 7) / 8); }
constexpr int conv_launch_bulk(int nrange, int S, int K) { return ((nrange >> 3) - (K < (nrange >> 3) ? K : (nrange >> 3))) * S * S; }
constexpr int conv_xcd_share(int x, int v) { return (v - x + 7) >> 3; }   // how many of x, x + 8, x + 16, ... lie below v (0 <= x < 8, v >= 0)
struct conv_wg { int range, p; };                                        // range < 0: no workgroup (the end of a shorter list)
constexpr conv_wg conv_launch_wg(int x, int i, int nrange, int S, int K) {
    const int P = S * S, q = nrange >> 3, m = nrange & 7, kd = K < q ? K : q;
    const int bulk = (q - kd) * P;
    if (i < bulk) {
        const int r = i / P;
        return {x * q + r, conv_pos_of(i - r * P, S)};
    }
    int d = i - bulk;
    for (int c = 0; c < 3; ++c) {
        const int n = conv_class_count(c, S), f = conv_class_first(c, S);
        if (d < kd * n) {                                                // the XCD's own last ranges
            const int r = d / n;
            return {x * q + q - kd + r, conv_pos_of(f + d - r * n, S)};
        }
        d -= kd * n;
        const int j0 = conv_xcd_share(x, m * f), left = conv_xcd_share(x, m * (f + n)) - j0;
        if (d < left) {                                                  // its share of the leftover ranges
            const int t = x + 8 * (j0 + d) - m * f, r = t / n;
            return {8 * q + r, conv_pos_of(f + t - r * n, S)};
        }
        d -= left;
    }
    return {-1, 0};
}

}  // namespace tg
