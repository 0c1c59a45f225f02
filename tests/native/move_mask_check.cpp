// Host side of csrc/move_mask.h, stand-alone (tests/test_move_mask.py compiles it with -fsanitize=address,undefined and compares its output
// with heuristics.move_mask): the predicate the two mask kernels compile, run on the CPU.
// stdin: one case per line, "G s D m B x0 y0 x1 y1 ...";  stdout: per case the B mask bytes in decimal.
#include <cstdio>
#include <vector>

#include "../../drl_uav_cellularnet_amd/csrc/move_mask.h"

int main() {
    int G, s, D, m, B;
    while (std::scanf("%d %d %d %d %d", &G, &s, &D, &m, &B) == 5) {
        if (B < 1 || B > 64) return 2;
        std::vector<move_mask::Cell> cells(B);
        for (int b = 0; b < B; ++b)
            if (std::scanf("%d %d", &cells[b].x, &cells[b].y) != 2) return 2;
        for (int b = 0; b < B; ++b)
            std::printf("%u%c", move_mask::allowed_bits(b, B, G, s, D, m, [&](int j) { return cells[j]; }), b + 1 < B ? ' ' : '\n');
    }
    return 0;
}
