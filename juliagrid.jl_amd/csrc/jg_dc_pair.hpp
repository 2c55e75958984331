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
// What is kept: Phi and its tables, a DcPhi (jg_dc_phi.hpp has the layout and the build, shared with the series and the transfer screen).
#pragma once
#include <hip/hip_runtime.h>

#include "jg_dc_phi.hpp"

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
    int* r_viol = nullptr; int* r_isl = nullptr; double* r_max = nullptr; long long* r_off = nullptr; long long* r_ioff = nullptr;    // [blk_rows]
    double* c_max = nullptr;                 // [ldk]
    double* rec = nullptr; long long rec_cap = 0;       // [rec_cap][5]
    long long* isl = nullptr; long long isl_cap = 0;    // [isl_cap][2]
    DcMem mem;                               // the device memory of the fields above (not the DcPhi's): what release frees
};

void dc_pair_free(DcHandle* h);              // releases what the pair screen holds, on the device and on the host (jg_dc_destroy, jg_dc_pair_release)

}  // namespace jg
