"""The launch order of k_conv3x3_sg (conv_launch_wg / conv_launch_grid in transgo_amd/csrc/conv_rows.h), compiled with plain g++ and
checked without a GPU, for S = 9 and 19, every nrange in 1..40 plus 123 and 128, and K = 1, 2, 4 (the kernel's own K, conv_drain_k in net.hip, is held to that set by a static_assert there):
  * over all (xcd, i) of the grid the map is a bijection onto nrange x P, and "none" exactly for the rest of the grid;
  * the grid is 8 x the longest XCD list and the count of workgroups rounded up to a multiple of 8;
  * the bulk part of every XCD is whole ranges, the XCD's own (x*q ...), in conv_pos_of order;
  * inside every XCD's drain part the walk never gets longer, and its own ranges come before the leftover ones inside a class;
  * per class, and in total, the XCDs' counts differ by at most one workgroup.
nrange < 8 (everything is leftover), nrange = 8q (no leftover), q <= K and q = K + 1 are all inside 1..40 for K = 1, 2, 4."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <vector>
#include <algorithm>
#include "conv_rows.h"
using namespace tg;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (S %d nrange %d K %d)\n", __LINE__, #c, S, nrange, K); return 1; } } while (0)
static int cls_of(int p, int S) { const int nt = conv_tap_count(conv_tap_mask(p, S)); return nt == 9 ? 0 : nt == 6 ? 1 : 2; }
static int check(int S, int nrange, int K) {
    const int P = S * S, q = nrange / 8, m = nrange % 8, kd = std::min(K, q);
    const int grid = conv_launch_grid(nrange, S), len = grid / 8, bulk = conv_launch_bulk(nrange, S, K);
    CHECK(grid % 8 == 0 && grid == (nrange * P + 7) / 8 * 8);
    CHECK(bulk == (q - kd) * P && bulk <= len);
    std::vector<int> seen(nrange * P, 0);
    int cnt[8][3] = {}, tot[8] = {}, longest = 0;
    for (int x = 0; x < 8; ++x) {
        bool ended = false;
        int prev_nt = 9, prev_cls = -1, prev_range = -1;
        for (int i = 0; i < len + 3; ++i) {                              // a little past the grid: still "none"
            const conv_wg w = conv_launch_wg(x, i, nrange, S, K);
            if (w.range < 0) { ended = true; continue; }
            CHECK(!ended);                                               // a list has no holes
            CHECK(i < len);
            CHECK(w.range < nrange && w.p >= 0 && w.p < P);
            CHECK(seen[w.range * P + w.p]++ == 0);
            const int c = cls_of(w.p, S), nt = conv_tap_count(conv_tap_mask(w.p, S));
            ++cnt[x][c]; ++tot[x];
            if (i < bulk) {                                              // whole own ranges, range-major, conv_pos_of inside
                CHECK(w.range == x * q + i / P && w.range < x * q + q - kd);
                CHECK(w.p == conv_pos_of(i % P, S));
            } else {                                                     // the last kd own ranges or a leftover range, class-major
                const bool own = w.range >= x * q + q - kd && w.range < x * q + q, left = w.range >= 8 * q;
                CHECK(own || left);
                CHECK(nt <= prev_nt);
                if (c == prev_cls) CHECK(w.range >= prev_range);         // range by range inside a class, own ranges first
                prev_nt = nt; prev_cls = c; prev_range = w.range;
            }
        }
        longest = std::max(longest, tot[x]);
    }
    for (int v : seen) CHECK(v == 1);
    CHECK(longest == len);
    for (int c = 0; c < 3; ++c) {
        int lo = cnt[0][c], hi = cnt[0][c];
        for (int x = 1; x < 8; ++x) { lo = std::min(lo, cnt[x][c]); hi = std::max(hi, cnt[x][c]); }
        CHECK(hi - lo <= 1);
        if (m == 0) CHECK(hi == lo);
    }
    CHECK(*std::max_element(tot, tot + 8) - *std::min_element(tot, tot + 8) <= 1);
    return 0;
}
int main() {
    int cases = 0;
    for (int S : {9, 19})
        for (int K : {1, 2, 4}) {
            for (int nrange = 1; nrange <= 40; ++nrange, ++cases) if (check(S, nrange, K)) return 1;
            for (int nrange : {123, 128}) { ++cases; if (check(S, nrange, K)) return 1; }
        }
    std::printf("launch order ok: %d cases\n", cases);
    return 0;
}
"""


def test_launch_order_is_a_bijection_that_ends_every_xcd_on_its_short_walks(tmp_path):
    src = tmp_path / "conv_launch_check.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "conv_launch_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "transgo_amd", "csrc"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "launch order ok: 252 cases" in out.stdout, out.stdout
