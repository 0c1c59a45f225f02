// Host check of the range guard of the multi-step kernels' 32-bit output offsets (csrc/state_layout.h: many_steps_in_range /
// many_steps_max), at the boundary and without any buffer.  Prints one line per case: name, expected, got.  Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../drl_uav_cellularnet_amd/csrc/state_layout.h"

static int g_bad = 0;
static void row(const char *name, long long want, long long got) {
    std::printf("%s %lld %lld\n", name, want, got);
    if (want != got) ++g_bad;
}

int main() {
    using uavk::many_steps_in_range;
    using uavk::many_steps_max;
    // T x N x U x 4 at 2^32 - 4, at 2^32 and one element past it (the *_bytes rows check the products themselves).
    // N = 2^20, U = 1: a block is 4 MiB; T = 1023 -> 2^32 - 2^22, T = 1024 -> 2^32
    row("pow2_below", 1, many_steps_in_range(1023, 1 << 20, 1, 0));
    row("pow2_at", 0, many_steps_in_range(1024, 1 << 20, 1, 0));
    row("pow2_max", 1023, many_steps_max(1 << 20, 1, 0));
    // exactly 2^32 - 4: T x N x U = 2^30 - 1 = 9 x 119304647
    row("minus4", 1, many_steps_in_range(9, 119304647LL, 1, 0));
    row("minus4_bytes", (long long)((1ull << 32) - 4), 9LL * 119304647LL * 1 * 4);
    // exactly 2^32: T x N x U = 2^30: T = 16, N = 2^20, U = 64
    row("exact", 0, many_steps_in_range(16, 1 << 20, 64, 0));
    row("exact_one_less_step", 1, many_steps_in_range(15, 1 << 20, 64, 0));
    // one element past 2^32: T x N x U = 2^30 + 1 = 5 x 214748365
    row("plus4", 0, many_steps_in_range(5, 214748365LL, 1, 0));
    row("plus4_bytes", (long long)((1ull << 32) + 4), 5LL * 214748365LL * 1 * 4);
    row("plus4_max", 4, many_steps_max(214748365LL, 1, 0));
    // the cell blocks (T x N x B x 8) decide where 8 B > 4 U: N = 2^20, U = 4, B = 8: a block is 64 MiB; T = 63 fits, T = 64 is 2^32
    row("cells_below", 1, many_steps_in_range(63, 1 << 20, 4, 8));
    row("cells_at", 0, many_steps_in_range(64, 1 << 20, 4, 8));
    row("cells_max", 63, many_steps_max(1 << 20, 4, 8));
    // the benchmark's shapes are far inside: 4096 x 20 x 4 bytes x 100 steps = 32 MiB
    row("bench", 1, many_steps_in_range(100, 4096, 20, 4));
    row("bench_max", ((1ll << 32) - 1) / (4096ll * 80), many_steps_max(4096, 20, 4));
    // every launch of a cut call is in range, and the cut is the largest that is: T = max fits, max + 1 does not
    for (long long n : {7LL, 129LL, 4096LL, 65536LL, 1LL << 22}) {
        for (long long u : {4LL, 10LL, 20LL, 64LL}) {
            const long long m = many_steps_max(n, u, 8);
            if (!many_steps_in_range(m, n, u, 8) || (m < 0x7FFFFFFFLL && many_steps_in_range(m + 1, n, u, 8))) { std::printf("max_consistent %lld %lld FAIL\n", n, u); ++g_bad; }
        }
    }
    row("degenerate_steps", 1, many_steps_in_range(0, 1 << 30, 64, 8));

    // ---- a lowered bound (trailing parameter `lim`, the handle's UAVENV_DEBUG_MANY_OFFSET_LIMIT) --------------------------------------
    using uavk::many_steps_per_piece;
    const unsigned long long top = 1ull << 32;
    struct Shape { long long n, u, b; unsigned long long block; };
    const Shape shapes[] = {{7, 20, 4, 560}, {129, 20, 4, 10320}, {129, 10, 8, 8256}};      // the last one: 8 B > 4 U, the cell blocks govern
    row("block_7x20", 560, (long long)uavk::many_block_bytes(7, 20, 4));
    row("block_129x20", 10320, (long long)uavk::many_block_bytes(129, 20, 4));
    row("block_129x10_8uav", 8256, (long long)uavk::many_block_bytes(129, 10, 8));
    // the bounds the device test sets: per * block + 1 gives exactly per; half a block more gives no step more; one block gives one step
    row("lim_per6", 6, many_steps_max(129, 20, 4, 6 * 10320ull + 1));
    row("lim_per6_in", 1, many_steps_in_range(6, 129, 20, 4, 6 * 10320ull + 1));
    row("lim_per6_out", 0, many_steps_in_range(7, 129, 20, 4, 6 * 10320ull + 1));
    row("lim_per23", 23, many_steps_max(129, 20, 4, 23 * 10320ull + 1));
    row("lim_half_block_more", 6, many_steps_max(129, 20, 4, 6 * 10320ull + 10320ull / 2));
    row("lim_one_block", 1, many_steps_max(129, 20, 4, 10320ull));
    row("lim_one_block_in", 0, many_steps_in_range(1, 129, 20, 4, 10320ull));        // "one step per launch" although that step fails the predicate
    row("lim_cells_per6", 6, many_steps_max(129, 10, 8, 6 * 8256ull + 1));
    // the bound can only be tightened: above 2^32 it is 2^32, and 0 is 1
    row("lim_above_max", many_steps_max(4096, 20, 4), many_steps_max(4096, 20, 4, 1ull << 33));
    row("lim_above_in", 0, many_steps_in_range(1024, 1 << 20, 1, 0, ~0ull));
    row("lim_zero_max", 1, many_steps_max(129, 20, 4, 0));
    row("lim_zero_in", 0, many_steps_in_range(1, 129, 20, 4, 0));
    long long bound_cases = 0, piece_cases = 0;
    for (const Shape &s : shapes) {
        const unsigned long long B = s.block;
        for (unsigned long long lim : {B, B + 1, 2 * B - 1, 2 * B, 6 * B + 1, 6 * B + B / 2, top}) {
            // bound consistency: the most steps pass the predicate (unless one step per launch is all there is), one more does not
            const long long m = many_steps_max(s.n, s.u, s.b, lim);
            const bool one_step_only = m == 1 && B >= lim;
            const bool ok = m >= 1 && (one_step_only || many_steps_in_range(m, s.n, s.u, s.b, lim)) && !many_steps_in_range(m + 1, s.n, s.u, s.b, lim) &&
                            (one_step_only || ((unsigned long long)m * B < lim && (unsigned long long)(m + 1) * B >= lim));
            if (ok) ++bound_cases; else { std::printf("bound_consistent %llu %llu FAIL\n", B, lim); ++g_bad; }
            // piece coverage: the walk uavenv_step_many takes over a call of n_steps
            for (long long n_steps : {1LL, m, m + 1, 2 * m, 2 * m + 1, 63LL}) {
                const long long per = many_steps_per_piece(n_steps, s.n, s.u, s.b, lim, true);
                long long sum = 0, pieces = 0, short_before_last = 0, too_long = 0, out_of_range = 0;
                for (long long t = 0; per >= 1 && t < n_steps; t += per) {
                    const long long n = n_steps - t < per ? n_steps - t : per;
                    sum += n; ++pieces;
                    if (n > m) ++too_long;
                    if (n < m && t + n < n_steps) ++short_before_last;
                    if (!one_step_only && !many_steps_in_range(n, s.n, s.u, s.b, lim)) ++out_of_range;
                }
                const bool whole = many_steps_per_piece(n_steps, s.n, s.u, s.b, lim, false) == n_steps;   // a call that does not read the path is never cut
                if (per >= 1 && sum == n_steps && pieces == (n_steps + m - 1) / m && !too_long && !short_before_last && !out_of_range && whole) ++piece_cases;
                else { std::printf("piece_coverage %llu %llu %lld FAIL\n", B, lim, n_steps); ++g_bad; }
            }
        }
    }
    row("bound_consistent_cases", 3 * 7, bound_cases);
    row("piece_coverage_cases", 3 * 7 * 6, piece_cases);
    // the device test's calls: 23 and 40 steps in pieces of 6 are 4 + 7 launches, in pieces of 23 they are 1 + 2
    row("pieces_of_6_in_23", 6, many_steps_per_piece(23, 129, 20, 4, 6 * 10320ull + 1, true));
    row("pieces_of_23_in_23", 23, many_steps_per_piece(23, 129, 20, 4, 23 * 10320ull + 1, true));
    row("pieces_of_23_in_40", 23, many_steps_per_piece(40, 129, 20, 4, 23 * 10320ull + 1, true));
    row("pieces_default_whole", 100, many_steps_per_piece(100, 4096, 20, 4, top, true));
    row("pieces_no_steps", 1, many_steps_per_piece(0, 129, 20, 4, 10320ull, true));
    return g_bad == 0 ? 0 : 1;
}
