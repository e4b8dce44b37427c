"""Index arithmetic of the board-grouped slice-major row order and of k_conv3x3_sg's tap walk (transgo_amd/csrc/conv_rows.h), compiled
with plain g++ -- the header has no HIP dependency -- and checked without a GPU:
  * conv_sg_row is a bijection of the (board, position) pairs of whole groups of 16 boards onto [0, conv_sg_rows), and the rows of
    the boards that exist stay below conv_sg_rows of the batch;
  * a tap that conv_tap_mask keeps shifts a row by (dy*S + dx)*16 and lands on the row of the neighbour position of the SAME board;
  * conv_pos_of is a bijection of the positions, longest walk first;
  * the (position, tap) stages walked number (3S-2)^2 for S = 9 and 19, and conv_tap_list / the kernel's k / nt multiplication
    enumerate exactly the taps of the mask, in ascending order, for every stage index the kernel can ask for."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv_rows.h"
using namespace tg;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
static int check(int S) {
    const int P = S * S;
    // row map: bijection onto the padded range for board counts around the group and workgroup boundaries
    const int counts[] = {1, 15, 16, 17, 127, 128, 129, 191, 192, 193, 1000};
    for (int boards : counts) {
        const int padded = (boards + 15) / 16 * 16, rows = conv_sg_rows(boards, P);
        CHECK(rows == padded * P);
        std::vector<int> seen(rows, 0);
        for (int b = 0; b < padded; ++b)
            for (int p = 0; p < P; ++p) {
                const int r = conv_sg_row(b, p, P);
                CHECK(r >= 0 && r < rows);
                CHECK(seen[r]++ == 0);
                CHECK((r & 15) == (b & 15));                        // a board keeps its MFMA column
            }
    }
    // taps: count, neighbour rows, list
    long stages = 0;
    for (int p = 0; p < P; ++p) {
        const unsigned mask = conv_tap_mask(p, S);
        const int nt = conv_tap_count(mask);
        CHECK(nt == 4 || nt == 6 || nt == 9);
        stages += nt;
        const unsigned long long list = conv_tap_list(mask);
        int k = 0;
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1, y = p / S + dy, x = p % S + dx;
            const bool on = y >= 0 && y < S && x >= 0 && x < S;
            CHECK(on == (((mask >> tap) & 1) != 0));
            if (!on) continue;
            CHECK((int)((list >> (4 * k)) & 15) == tap);
            ++k;
            for (int b : {0, 5, 16, 37})
                CHECK(conv_sg_row(b, p, P) + (dy * S + dx) * 16 == conv_sg_row(b, y * S + x, P));
        }
        CHECK(k == nt && (list >> (4 * k)) == 0);
        // the kernel's stage -> (slice, tap): k / nt as (k * inv) >> 16, for every stage of the widest tower (16 slices)
        const int inv = nt == 9 ? 7282 : nt == 6 ? 10923 : 16384;
        for (int st = 0; st < 16 * nt; ++st) {
            const int sl = (st * inv) >> 16;
            CHECK(sl == st / nt);
            CHECK((int)((list >> (4 * (st - sl * nt))) & 15) < 9);
        }
        for (int t = 0; t < 9; ++t) CHECK(((t * 11) >> 5) == t / 3);   // tap / 3 as the kernel forms it on a scalar
    }
    CHECK(stages == (long)(3 * S - 2) * (3 * S - 2));
    // workgroup order: a bijection, walks never longer than the one before
    std::vector<int> seen(P, 0);
    int prev = 9;
    for (int i = 0; i < P; ++i) {
        const int p = conv_pos_of(i, S);
        CHECK(p >= 0 && p < P && seen[p]++ == 0);
        const int nt = conv_tap_count(conv_tap_mask(p, S));
        CHECK(nt <= prev);
        prev = nt;
    }
    std::printf("S=%d stages=%ld of %d\n", S, stages, 9 * P);
    return 0;
}
int main() { return check(9) || check(19); }
"""


def test_row_map_is_a_bijection_and_the_walk_has_3s_minus_2_squared_stages(tmp_path):
    src = tmp_path / "conv_rows_check.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "conv_rows_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "transgo_amd", "csrc"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "S=9 stages=625 of 729" in out.stdout and "S=19 stages=3025 of 3249" in out.stdout, out.stdout
