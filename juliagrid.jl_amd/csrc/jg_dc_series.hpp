// jg_dc_series.hpp -- the DC N-1 screen over a SERIES of injection profiles, on the ONE factor of a DcHandle (jg_dc.hpp) and the outage sensitivities
// the builds of the screens keep (a DcPhi, jg_dc_phi.hpp).
//
// Reference counterpart: the user loop
//     for t in profiles:   updateBus!(...; active) / updateGenerator!(...; active)
//       for k in branches: updateBranch!(...; label = k, status = 0); solve!; power!; updateBranch!(...; status = 1)
// With Phi[m,k] = y_m a_m' B^-1 a_k (jg_dc_pair.hpp has the algebra) and the base flows of profile t, F0[m,t] = y_m (a_m' theta_t - shiftAngle_m), theta_t = B^-1 rhs_t:
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
// What is kept: Phi [rows][ldk] as dc_phi_build makes it (a DcPhi of the series' own: the pair screen's h->pair is not touched), and
// F0 [rows][ldt] doubles on the same rows, ldt = profiles rounded up to 64, 0 behind the last profile.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "jg_dc_records.hpp"

namespace jg {

#ifndef JG_DC_SERIES_TILE
#define JG_DC_SERIES_TILE 4                  // probe builds: -DJG_DC_SERIES_TILE=8 (the register report of DESIGN.md 3.11)
#endif
constexpr int DC_SERIES_TILE = JG_DC_SERIES_TILE;   // candidates k a wave of k_series_screen keeps in registers: a row of F0 is loaded once for all of them
static_assert(DC_SERIES_TILE == 4 || DC_SERIES_TILE == 8, "a tile of k is one or two 32-byte scalar loads of a row of Phi");

struct DcSeriesState {
    DcPhi phi;                               // Phi and the row / candidate tables of the shared build
    int T = 0, ldt = 0;                      // profiles, rounded up to 64
    double* F0 = nullptr;                    // [rows][ldt]
    std::vector<char> h_bridge;              // [nk] 1: |1 - Phi[k,k]| < DC_SINGULAR
    // the row block of a screen call (grown on demand)
    int blk_rows = 0;
    double* b_load = nullptr; int* b_branch = nullptr; int* b_count = nullptr;      // [blk_rows][ldt]
    double* r_max = nullptr;                 // [blk_rows]
    double* c_max = nullptr; int* c_viol = nullptr;                                 // [ldt] over the block's candidates, per profile
    double* base = nullptr;                  // [ldt][3] the profiles' base case: worst loading, its branch, the count
    DcRecords viol{5 * sizeof(double)};      // the violators [5]
    double build_ms[3] = {0, 0, 0};          // F0 of the last build: total, sweep pairs, F0 kernel (HIP events)
    DcMem mem;                               // the device memory of the fields above (not the DcPhi's): what release frees
};

// The series' arithmetic on the arrays of ANY state that keeps a DcPhi and column flows on its rows (the series' own profiles, the generator screen's
// outage columns: jg_dc_generator.hpp): F0 [rows of phi][ldt], T columns, 0 behind them; the block's dense result load / branch / count [k1 - k0][ldt].
//   dc_series_launch_screen   k_series_screen on the candidate rows [k0, k1) (the <true> instance where phi was built in shed mode)
//   dc_series_launch_cols     per column over the `rb` rows of the block: c_max / c_viol [ldt], the worst loading (NaN aside) and the rows above thr
//   dc_series_launch_base     base [T][3]: a column's case without an outage -- worst loading, its branch (1-based, 0: none), branches above thr
// Launches on the handle's stream; phi->row_rinv is the caller's to set first (dc_phi_rinv).
struct DcSeriesBlock { const DcPhi* phi; const double* F0; int ldt, T; double* load; int* branch; int* count; };
void dc_series_launch_screen(DcHandle* h, const DcSeriesBlock& b, int k0, int k1, double thr);
void dc_series_launch_cols(DcHandle* h, const DcSeriesBlock& b, double* c_max, int* c_viol, double thr, int rb);
void dc_series_launch_base(DcHandle* h, const DcSeriesBlock& b, double* base, double thr);

void dc_series_free(DcHandle* h);            // releases what the series screen holds (jg_dc_destroy, jg_dc_series_release)

}  // namespace jg
