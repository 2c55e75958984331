// jg_dc_transfer.hpp -- the DC transfer-capability screen over transfers x N-1 outages, on the ONE factor of a DcHandle (jg_dc.hpp) and the outage
// sensitivities the builds of the screens keep (a DcPhi, jg_dc_phi.hpp).
//
// Reference counterpart: the user loop
//     repeat: updateBus!(...; active) / updateGenerator!(...; active) along a direction
//       for k in branches: updateBranch!(...; label = k, status = 0); solve!; power!; updateBranch!(...; status = 1)
//     until a monitored branch reaches its rating
// Base operating point: the handle's right-hand side (jg_dc_set_rhs), or a base profile given at build time.  Transfer t is a direction d_t [buses] of net
// active injection per unit of transfer, as setInjection_ means it: the injection is P0 + lambda d_t.  A direction need not sum to zero: the slack takes
// the rest, as the reference's solve! would have it.  With Phi[m,k] = y_m a_m' B^-1 a_k (jg_dc_pair.hpp has the algebra) and the base flows F0[m]:
//     G[m,t]    = y_m a_m' B^-1 d_t                  flow sensitivity of row m to transfer t: NO shift angle, NO shunt / shiftPower term, slack entry 0
//     d_k       = 1 - Phi[k,k]                       |d_k| < DC_SINGULAR: k is a bridge (status 3, NaN for all its transfers, never in a minimum or a record)
//     f_m(k)    = F0[m] + Phi[m,k] F0[k] / d_k       post-outage flow at zero transfer (m != k)
//     g_m(k,t)  = G[m,t]  + Phi[m,k] G[k,t] / d_k    post-outage sensitivity (m != k); the base case "k = none" uses F0[m], G[m,t]
//     limit_m   = (sign(g) r_m - f) / g              the lambda at which branch m reaches the rating on the side the transfer pushes it
//     TC(k,t)   = min over eligible m of limit_m     eligible: monitored, rated, m != k, |g_m(k,t)| > cutoff
// TC is negative when the limiting branch is already beyond that rating at zero transfer, and +inf with limiting branch 0 when no row is eligible.  Ties go
// to the lowest branch index: strict comparison, rows ascending.  cutoff is in per unit of flow per per unit of transfer (default 1e-6 on the Python
// side): a sensitivity the size of the sweeps' rounding (4e-13 on the 10k-bus grid) must never limit anything.  So a case (k, t) costs no sweep: two FMAs
// and one ratio comparison per monitored branch.  The sweeps run once per candidate (Phi) and once per direction (G).
//
// The kernel works in loading space: with rinv = 1 / r_m, limit_m = (1 - copysign(f rinv, g)) / (|g| rinv) = num / den with den > 0, the running minimum
// is a (num, den, row) triple compared by cross-multiplication, and the one division of a case comes after the last row.  (1, 0) is +inf.
//
// What is kept: Phi [rows][ldk] as dc_phi_build makes it (a DcPhi of the screen's own: h->pair and h->series are not touched), the base
// flows f0 [rows], and G [rows][ldt] doubles on the same rows, ldt = transfers rounded up to 64, 0 behind the last transfer.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "jg_dc_records.hpp"

namespace jg {

constexpr int DC_TRANSFER_TILE = 4;          // transfers t a wave of k_transfer_screen keeps in registers: G[m, t..t+3] is one 32-byte scalar load

struct DcTransferState {
    DcPhi phi;                               // Phi and the row / candidate tables of the shared build
    int T = 0, ldt = 0;                      // transfers, rounded up to 64
    double* G = nullptr;                     // [rows][ldt]
    double* f0 = nullptr;                    // [rows] base flows: of the handle's right-hand side, or of the build's base profile
    std::vector<char> h_bridge;              // [nk] 1: |1 - Phi[k,k]| < DC_SINGULAR
    std::vector<int> h_row_label;            // [rows] 1-based branch label of a row
    // the row block of a screen call (grown on demand)
    int blk_rows = 0;
    double* b_tc = nullptr; int* b_row = nullptr;                                   // [blk_rows][ldt] TC and the limiting ROW (-1: none)
    double* r_min = nullptr;                 // [blk_rows]
    double* c_min = nullptr; int* c_at = nullptr; int* c_row = nullptr;             // [ldt] over the block's candidates, per transfer: the least TC, its block row, its limiting row
    double* amount = nullptr;                // [ldt] the record threshold of a screen call
    double* base = nullptr;                  // [ldt][3] the transfers' base case: TC, the limiting row, branches above their rating at zero transfer
    DcRecords below{5 * sizeof(double)};     // the cases below their amount [5]
    double build_ms[3] = {0, 0, 0};          // G of the last build: total, sweep pairs, G kernel (HIP events)
    DcMem mem;                               // the device memory of the fields above (not the DcPhi's): what release frees
};

void dc_transfer_free(DcHandle* h);          // releases what the transfer screen holds (jg_dc_destroy, jg_dc_transfer_release)

}  // namespace jg
