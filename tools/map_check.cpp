// map_check.cpp -- the launch mapping of csrc/jg_engine.hpp (map_slot, grid_blocks) walked exhaustively on the host.
//
// A handle sizes every grid once, by ITS group count; after compaction the kernels map by the CURRENT count of active groups, which may fall in the other
// mapping class (pinned: 1, 2, 4 and the multiples of 8; balanced: every other count).  For every handle count 1..72, every active count up to it and a set
// of chunk counts around the edges of `chunk = (total + 7) >> 3`, the ids 0 .. grid_blocks(groups, nx) - 1 must
//   * produce every (slot < gact, x < nx) pair exactly once and nothing outside that range,
//   * pinned counts: slot == id % gact (workgroup id lands on XCD id % 8: a group stays on the XCDs congruent to it),
//   * balanced counts: the ids congruent to k mod 8 serve ONE contiguous run of the group-major list of pairs.
// Built by tests/test_launch_map_cpu.py with g++ -fsanitize=address,undefined; exit status 0 = all of it holds.
#include <cstdio>
#include <vector>

#include "../juliagrid.jl_amd/csrc/jg_engine.hpp"

int main() {
    const int NX[] = {1, 2, 3, 5, 7, 8, 9, 16, 63, 64, 65, 1000};
    long long combos = 0, ids = 0;
    int failures = 0;
    auto fail = [&](const char* what, int groups, int gact, int nx, int id, int slot, int x) {
        if (++failures <= 20) std::fprintf(stderr, "map_check: %s: groups %d, gact %d, nx %d, id %d -> slot %d, x %d\n", what, groups, gact, nx, id, slot, x);
    };
    std::vector<int> seen;
    for (int groups = 1; groups <= 72; ++groups)
        for (int gact = 1; gact <= groups; ++gact)
            for (int nx : NX) {
                const long long grid = jg::grid_blocks(groups, nx);
                const bool balanced = jg::groups_balanced(gact);
                seen.assign((size_t)gact * nx, 0);
                int last[8];
                for (int k = 0; k < 8; ++k) last[k] = -1;
                ++combos;
                for (int id = 0; id < grid; ++id, ++ids) {
                    int slot = -1, x = -1;
                    if (!jg::map_slot(gact, nx, id, slot, x)) continue;
                    if (slot < 0 || slot >= gact || x < 0 || x >= nx) { fail("pair out of range", groups, gact, nx, id, slot, x); continue; }
                    const int flat = slot * nx + x;
                    if (seen[flat]++) fail("pair served twice", groups, gact, nx, id, slot, x);
                    if (!balanced) {
                        if (slot != id % gact) fail("pinned count: slot != id % gact", groups, gact, nx, id, slot, x);
                    } else {
                        const int k = id & 7;
                        if (last[k] >= 0 && flat != last[k] + 1) fail("balanced count: the run of an XCD is not contiguous", groups, gact, nx, id, slot, x);
                        last[k] = flat;
                    }
                }
                for (int flat = 0; flat < gact * nx; ++flat)
                    if (!seen[flat]) fail("pair never served", groups, gact, nx, -1, flat / nx, flat % nx);
            }
    std::printf("map_check: %lld (groups, gact, nx) combinations, %lld workgroup ids, %d failures\n", combos, ids, failures);
    return failures ? 1 : 0;
}
