// jg_dc_pair.hpp -- the DC N-2 screen over all pairs of a candidate list, on the ONE factor of a DcHandle (jg_dc.hpp) and the kept outage sensitivities.
//
// Reference counterpart: the user loop updateBranch!(analysis; label = k, status = 0), updateBranch!(analysis; label = l, status = 0), solve!, power!
// over all pairs k < l.  With B theta0 = rhs the base case, a_k = e_from - e_to of branch k (the slack's component dropped), z_k = B^-1 a_k and
//     Phi[m,k] = y_m a_m' z_k          the outage sensitivity of the flow of branch m to candidate k
//     f0_m     = y_m (a_m' theta0 - shiftAngle_m)      the base-case flow (what jg_dc_get_flows delivers)
// the outage of the set S moves the angles by Z_S c with (I - Y_S A_S' Z_S) c = f0_S, i.e. for a pair S = {k, l}
//     | 1 - Phi[k,k]    - Phi[k,l] | |c_k|   |f0_k|
//     |   - Phi[l,k]  1 - Phi[l,l] | |c_l| = |f0_l|,      f_m(S) = f0_m + Phi[m,k] c_k + Phi[m,l] c_l  (m not in S),  f_k(S) = f_l(S) = 0
// so a pair costs no sweep: a 2 x 2 solve and one pass over the monitored branches.  |det| < DC_SINGULAR: the pair islands a part of the grid (also when
// neither branch alone is a bridge): status 3, the worst loading is NaN.
//
// Shed mode (jg_dc_pair_set_island_mode 1 before the build; jg_dc_series.hpp has the single outage): a candidate c the handle's island table calls a bridge
// has s_c = +1 / -1 (its end m on the slack's side is the from / to end), the preorder interval [lo_c, hi_c] of the buses S_c that leave, the column
// Z[:,c] = y_l a_l' B^-1 e_m in place of Phi[:,c], and g_c = s_c f0_c, the flow that left m over it in the base case.  S_c hangs on the rest M as a stub:
// the sensitivities between branches of M do not see it, the flow over c is the net injection behind it whatever happens in M, and two such intervals are
// nested or disjoint.  So a pair with a bridge needs no 2 x 2 solve: it is f_m = f0_m + P[m,k] c_k + P[m,l] c_l with (the roles of k and l exchange)
//     k bridge, l not, l behind k (lo_k <= preorder[from_l] <= hi_k)     c_k = g_k   c_l = 0
//     k bridge, l not, l in M                                            c_k = g_k   c_l = (f0_l + Z[l,k] g_k) / (1 - Phi[l,l]); |1 - Phi[l,l]| < DC_SINGULAR: status 3
//     both bridges, disjoint intervals                                   c_k = g_k   c_l = g_l
//     both bridges, l's interval inside k's                              c_k = g_k   c_l = 0
// and 0 on the two branches and on every row whose from end lies in either interval.  "Behind" is one test for every kind of l: preorder[from_l] lies in
// k's interval exactly when l, bridge or not, leaves with k.  A pair of two non-bridges is the system above, bitwise.  What stays status 3: the joint cuts
// of two non-bridges (their S is no stub) and the pairs with a singular non-bridge.
//
// What is kept: Phi and its tables, a DcPhi (jg_dc_phi.hpp has the layout and the build, shared with the series and the transfer screen).
#pragma once
#include <hip/hip_runtime.h>

#include "jg_dc_records.hpp"

namespace jg {

#ifndef JG_DC_PAIR_TILE
#define JG_DC_PAIR_TILE 4                    // probe builds: -DJG_DC_PAIR_TILE=8 (the A/B of DESIGN.md 3.9)
#endif
constexpr int DC_PAIR_TILE = JG_DC_PAIR_TILE;   // candidates k a wave of the screen kernel keeps in registers: a row of Phi is loaded once for all of them
static_assert(DC_PAIR_TILE == 4 || DC_PAIR_TILE == 8, "a tile of k is one or two 32-byte scalar loads of a row of Phi");

struct DcPairState {
    DcPhi phi;                               // the kept sensitivities of the last build
    // the row block of a screen call (grown on demand)
    int blk_rows = 0;
    double* b_load = nullptr; int* b_branch = nullptr; int* b_count = nullptr; double* b_det = nullptr;     // [blk_rows][ldk]; b_det only on request
    double* r_max = nullptr;                 // [blk_rows]
    double* c_max = nullptr;                 // [ldk]
    DcRecords viol{5 * sizeof(double)}, isl{2 * sizeof(long long)};       // the violators [5] and the islanding pairs [2]
    DcMem mem;                               // the device memory of the fields above (not the DcPhi's): what release frees
};

void dc_pair_free(DcHandle* h);              // releases what the pair screen holds, on the device and on the host (jg_dc_destroy, jg_dc_pair_release)

}  // namespace jg
