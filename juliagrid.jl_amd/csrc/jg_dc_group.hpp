// jg_dc_group.hpp -- the DC common-mode screen: named outage GROUPS of 1 to DC_GROUP_MAX branches, each one case, on the ONE factor of a DcHandle
// (jg_dc.hpp) and the kept outage sensitivities (jg_dc_phi.hpp).
//
// Reference counterpart: the user loop updateBranch!(analysis; label = s, status = 0) for every member s of a group, then solve!, power! -- one rebuild
// and one refactorisation per group.  jg_dc_pair.hpp has the algebra for a set S; the group screen is that set, stated for k = |S| members:
//     (I - Phi_SS) c = f0_S,      f_m(S) = f0_m + sum_{s in S} Phi[m,s] c_s   (m not in S),      f_s(S) = 0   (s in S)
// so a group costs no sweep: a k x k solve (k_group_solve) and one pass over the rows of Phi that gathers k columns per group (k_group_screen).  On a member
// the sum gives f0_s + Phi[s,:] c = c_s, not 0: the exclusion of the members' rows is part of the formula.
//
// The k x k system is solved by LU with partial pivoting.  A pivot below DC_SINGULAR in magnitude (jg_dc.hpp, the pair screen's rule): the group islands a
// part of the grid -- it holds a bridge, or its members form a joint cut -- status 3, the worst loading is NaN.  There is no shed mode.
//
// What is kept: Phi on the candidates = the sorted union of all members (a DcPhi), the groups as candidate positions g_pos [DC_GROUP_MAX][ldg] (-1: no such
// member; ldg = groups rounded up to 64), and per group the coefficients c [DC_GROUP_MAX][ldg] and the status [ldg] of the last solve.
#pragma once
#include <hip/hip_runtime.h>

#include "jg_dc_records.hpp"

namespace jg {

constexpr int DC_GROUP_MAX = 8;              // members of a group at the most; the kernels come as K = 2, 4, 8, chosen per block by its largest group

struct DcGroupState {
    DcPhi phi;                               // the kept sensitivities of the last build
    int ngroups = 0, ldg = 0;
    std::vector<int> h_size;                 // [ngroups] members of a group
    std::vector<int> h_mon_row;              // [monitored, ascending] the row of Phi of a monitored branch
    int* g_pos = nullptr;                    // [DC_GROUP_MAX][ldg] candidate positions of the members, -1 behind the last
    double* c = nullptr;                     // [DC_GROUP_MAX][ldg] the coefficients of the last solve
    int* status = nullptr;                   // [ldg] 0 / 3
    // the block of a screen call (grown on demand)
    int blk_groups = 0, blk_flow = 0;        // blk_flow: groups the dense flows hold (0: never asked for)
    double* b_worst = nullptr; int* b_branch = nullptr;      // [blk_groups]
    int* b_wcnt = nullptr;                   // [DC_PAIR_WAVES][blk_groups rounded up to 64] violators per wave's share of the rows: where a wave's records start
    double* b_flow = nullptr;                // [rows][blk_flow rounded up to 64] on request
    DcRecords viol{4 * sizeof(double)}, isl{sizeof(long long)};       // the violators [4] and the islanding groups [1]
    DcMem mem;                               // the device memory of the fields above (not the DcPhi's): what release frees
};

void dc_group_free(DcHandle* h);             // releases what the group screen holds, on the device and on the host (jg_dc_destroy, jg_dc_group_release)

}  // namespace jg
