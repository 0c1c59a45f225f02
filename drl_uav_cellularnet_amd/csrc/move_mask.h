// The move mask of the factored learner, stated ONCE for libuavagent (agent_mask.hip: the cells decoded from the
// index list) and libuavenv (uavenv_mask.hip: the cells of the handle's state), host and device.  Integers only, exact.
//
// For UAV b at cell c_b, digit d < 4 (0: +x, 1: -x, 2: +y, 3: -y -- BS_move's, ue_mobility.py:221-235), dest = c_b moved by s = bs_step:
//   wall    the bound guard of BS_move fails: x + s < G, x - s > 1, y + s < G, y - s > 1
//   frozen  some j != b has |c_b - c_j|^2 <= D^2, D = min_bs_dist  (sqrt(n) <= D  <=>  n <= D^2 for integers; ue_mobility.py:256-266)
//   crowd   m > 0 and some j != b has |dest - c_j|^2 <= m^2, m = the margin
//   allowed[d] = !(wall | frozen | crowd);  allowed[4] (stay) = 1 always
// Bit d of the result is allowed[d]; bit 4 is always set.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MOVE_MASK_HD __host__ __device__ inline
#else
#define MOVE_MASK_HD inline
#endif

namespace move_mask {

constexpr int kDigits = 5;                  // n_act of the mask: four moves and stay
constexpr unsigned kStayBit = 1u << 4;
constexpr unsigned kAllBits = 0x1Fu;        // every digit allowed
constexpr float kMaskedLogit = -3.0e38f;    // head_logits' padding sentinel (agent_loss_factored.h): exp(sentinel - max) == 0 exactly

struct Cell { int x, y; };

// cell(j) -> Cell of UAV j, 0 <= j < B.  64-bit differences and squares: exact for |x|, |y| <= 2^29 (both callers hold cells below 2^30 >= 0).
template <class Fetch>
MOVE_MASK_HD unsigned allowed_bits(int b, int B, int G, int s, int D, int m, Fetch cell) {
    const Cell c = cell(b);
    const long long D2 = (long long)D * D, m2 = (long long)m * m;
    const long long x = c.x, y = c.y;
    const long long dest_x[4] = {x + s, x - s, x, x};
    const long long dest_y[4] = {y, y, y + s, y - s};
    unsigned bits = (unsigned)(x + s < G) | ((unsigned)(x - s > 1) << 1) | ((unsigned)(y + s < G) << 2) | ((unsigned)(y - s > 1) << 3);
    bool frozen = false;
    for (int j = 0; j < B; ++j) {
        if (j == b) continue;
        const Cell o = cell(j);
        const long long dx = x - o.x, dy = y - o.y;
        frozen = frozen || (dx * dx + dy * dy <= D2);
        if (m > 0) {
            for (int d = 0; d < 4; ++d) {
                const long long ex = dest_x[d] - o.x, ey = dest_y[d] - o.y;
                if (ex * ex + ey * ey <= m2) bits &= ~(1u << d);
            }
        }
    }
    return (frozen ? 0u : bits) | kStayBit;
}

}  // namespace move_mask
