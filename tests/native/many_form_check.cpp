// Host check of the predicate that picks the multi-step kernel whose walker lanes carry their group's motion (csrc/state_layout.h:
// many_groups_carried, beside slot_sum_in_quads).  Prints one line per case: name, expected, got.  Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>

#include "../../drl_uav_cellularnet_amd/csrc/state_layout.h"

static int g_bad = 0;
static void row(const char *name, int want, int got) {
    std::printf("%s %d %d\n", name, want, got);
    if (want != got) ++g_bad;
}

int main() {
    using uavk::many_groups_carried;
    const int32_t even[16] = {5, 5, 5, 5}, one_member[16] = {1, 2, 5}, empty[16] = {10, 0, 5, 5}, last_empty[16] = {10, 5, 5, 0};
    const int32_t ten[16] = {3, 3, 4}, wide[16] = {9, 9, 9, 9}, forty[16] = {10, 10, 10, 10}, single[16] = {4}, thirty_two[16] = {8, 8, 8, 8};
    row("all_nonempty", 1, many_groups_carried(20, 4, even));
    row("one_member_group", 1, many_groups_carried(8, 3, one_member));
    row("one_empty", 0, many_groups_carried(20, 4, empty));
    row("last_empty", 0, many_groups_carried(20, 4, last_empty));
    row("sizes_past_n_groups_ignored", 1, many_groups_carried(20, 3, last_empty));
    row("u_no_multiple_of_4", 0, many_groups_carried(10, 3, ten));
    row("u_32", 1, many_groups_carried(32, 4, thirty_two));
    row("u_36_above_32", 0, many_groups_carried(36, 4, wide));
    row("u_40_above_32", 0, many_groups_carried(40, 4, forty));
    row("one_group", 1, many_groups_carried(4, 1, single));
    row("no_group", 0, many_groups_carried(4, 0, single));
    row("quads_20", 1, uavk::slot_sum_in_quads(20));
    row("quads_10", 0, uavk::slot_sum_in_quads(10));
    row("quads_64", 0, uavk::slot_sum_in_quads(64));
    return g_bad == 0 ? 0 : 1;
}
