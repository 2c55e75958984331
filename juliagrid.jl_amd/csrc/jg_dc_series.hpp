// jg_dc_series.hpp -- the DC N-1 screen over a SERIES of injection profiles, on the ONE factor of a DcHandle (jg_dc.hpp) and the outage sensitivities
// the N-2 build keeps (jg_dc_pair.hpp).
//
// Reference counterpart: the user loop
//     for t in profiles:   updateBus!(...; active) / updateGenerator!(...; active)
//       for k in branches: updateBranch!(...; label = k, status = 0); solve!; power!; updateBranch!(...; status = 1)
// With Phi[m,k] = y_m a_m' B^-1 a_k (jg_dc_pair.hpp) and the base flows of profile t, F0[m,t] = y_m (a_m' theta_t - shiftAngle_m), theta_t = B^-1 rhs_t:
//     d_k      = 1 - Phi[k,k]                   |d_k| < DC_SINGULAR: k is a bridge (status 3 in every profile, the loading is NaN)
//     c_kt     = F0[k,t] / d_k
//     f_m(k,t) = F0[m,t] + Phi[m,k] c_kt        (m != k),   f_k(k,t) = 0
// so a case (k, t) costs no sweep: one FMA and one compare per monitored branch.  The sweeps run once per candidate (Phi) and once per profile (F0).
//
// Shed mode (jg_dc_series_set_island_mode 1 before the build): a candidate the handle's island table (dc_island_table: the graph, not |d_k|) calls a
// bridge is solved on the side M that holds the slack, as the lanes of jg_dc.hpp are.  With m its end in M, S the preorder interval [lo_k, hi_k] that leaves:
//     z_k      = B^-1 e_m (slack component dropped; m = slack: 0)         Z[l,k] = y_l a_l' z_k stands in the candidate's column of Phi
//     g_kt     = s_k F0[k,t]                s_k = +1 / -1: m is the from / to end -- what left m over the bridge before the outage
//     f_l(k,t) = F0[l,t] + Z[l,k] g_kt      for l with both ends in M;   0 for l = k and every branch with an end in S
// k is the only branch between S and M, so a row other than k left exactly when lo_k <= preorder[from_l] <= hi_k.  A non-bridge with |d_k| < DC_SINGULAR
// keeps status 3 and NaN.
//
// What is kept: Phi [rows][ldk] exactly as the pair build makes it (a DcPairState of the series' own: the pair screen's h->pair is not touched), and
// F0 [rows][ldt] doubles on the same rows, ldt = profiles rounded up to 64, 0 behind the last profile.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "jg_dc_pair.hpp"

namespace jg {

#ifndef JG_DC_SERIES_TILE
#define JG_DC_SERIES_TILE 4                  // probe builds: -DJG_DC_SERIES_TILE=8 (the register report of DESIGN.md 3.11)
#endif
constexpr int DC_SERIES_TILE = JG_DC_SERIES_TILE;   // candidates k a wave of k_series_screen keeps in registers: a row of F0 is loaded once for all of them
static_assert(DC_SERIES_TILE == 4 || DC_SERIES_TILE == 8, "a tile of k is one or two 32-byte scalar loads of a row of Phi");

struct DcSeriesState {
    DcPairState* phi = nullptr;              // Phi and the row / candidate tables of the shared build
    int T = 0, ldt = 0;                      // profiles, rounded up to 64
    double* F0 = nullptr;                    // [rows][ldt]
    std::vector<char> h_bridge;              // [nk] 1: |1 - Phi[k,k]| < DC_SINGULAR
    // the row block of a screen call (grown on demand)
    int blk_rows = 0;
    double* b_load = nullptr; int* b_branch = nullptr; int* b_count = nullptr;      // [blk_rows][ldt]
    int* r_viol = nullptr; double* r_max = nullptr; long long* r_off = nullptr;     // [blk_rows]
    double* c_max = nullptr; int* c_viol = nullptr;                                 // [ldt] over the block's candidates, per profile
    double* base = nullptr;                  // [ldt][3] the profiles' base case: worst loading, its branch, the count
    double* rec = nullptr; long long rec_cap = 0;       // [rec_cap][5]
    double build_ms[3] = {0, 0, 0};          // F0 of the last build: total, sweep pairs, F0 kernel (HIP events)
};

void dc_series_free(DcHandle* h);            // releases what the series screen holds (jg_dc_destroy, jg_dc_series_release)

// The lane-batch loop of the build is shared with the transfer screen (jg_dc_transfer.hpp):
//   dc_series_row_flows     F [rows of p][ldt] from `T` right-hand sides rhs [T][n] (the slack's entry is taken as 0): uploads DC_PAIR_LANES of them at a
//                           time, runs the sweep pair and turns the angles into row flows y_m (a_m' theta - shiftAngle_m); shift false: y_m a_m' theta,
//                           the sensitivity of the flow to the right-hand side.  Scratch of its own (dc_series_flows_scratch bytes), released on return;
//                           ms [2] gets the milliseconds of the sweep pairs and of the flow kernel added (HIP events).  Not 0: the text is in h->error
//   dc_series_bridges       bridge [nk] 1: |1 - Phi[k,k]| < DC_SINGULAR
//   dc_series_shed_table    the bridge candidates (shed mode) among the positions [k0, k1): their number, and per bridge the label, the buses that leave,
//                           m (1-based) and the side; null outputs are skipped
//   dc_series_shed_gather   out [bridges in [k0, k1)][T] on the host = s_k F[row of k][t], from the device (k_shed_gather: one thread per value)
size_t dc_series_flows_scratch(const DcHandle* h, int ldt);
int dc_series_shed_table(const DcHandle* h, const DcPairState* p, int k0, int k1, int64_t* labels, int64_t* buses, int64_t* m, int64_t* side);
int dc_series_shed_gather(DcHandle* h, const DcPairState* p, int k0, int k1, const double* F, int ldt, int T, double* out);
int dc_series_row_flows(DcHandle* h, const DcPairState* p, int T, const double* rhs, bool shift, double* F, int ldt, double* ms);
int dc_series_bridges(DcHandle* h, const DcPairState* p, std::vector<char>& bridge);

}  // namespace jg
