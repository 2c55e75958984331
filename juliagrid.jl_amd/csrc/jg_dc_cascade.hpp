// jg_dc_cascade.hpp -- the DC cascading-outage screen: an initiating outage of 1 to DC_CASCADE_MAX branches, then every overloaded monitored branch trips
// and the flows are formed again, stage after stage, on the ONE factor of a DcHandle (jg_dc.hpp) and the kept outage sensitivities (jg_dc_phi.hpp).
//
// Reference counterpart: the user loop updateBranch!(analysis; label = s, status = 0) for the initiating members, solve!, power!; then updateBranch! for
// what is overloaded, solve!, power! again, until nothing is overloaded -- one rebuild and one refactorisation per stage and per initiating event.
//
// The algebra is that of an outage set S (jg_dc_group.hpp): (I - Phi_SS) c = f0_S, f_m(S) = f0_m + sum_s Phi[m,s] c_s (m not in S), f_s(S) = 0.  What is
// new is that S grows on the device by a rule that looks at the flows just formed.  Per cascade, stage 0 being the initiating set:
//   1. solve the |S| x |S| system (dc_group_lu, jg_dc_group_lu.hpp: the group screen's LU and its DC_SINGULAR rule);
//   2. singular: the set islands a part of the grid -- status 3, the cascade ends (no shed mode);
//   3. form the flows of the monitored rows not in S; a branch is overloaded when |flow| / rating > trip (strict); an unrated or unmonitored row never is;
//   4. rule 0 ("all"): every overloaded branch trips, ascending by branch within the stage; rule 1 ("worst"): the most loaded one (ties: lowest branch);
//   5. no trip: status 0 (stable).  |S| + trips > most: status DC_CASCADE_TRUNCATED, S stays, `pending` = the overloaded branches.  Else append, next stage.
// Any branch that can trip needs its column: the candidates are the sorted union of the initiating members and the monitored branches in service.
//
// One launch of k_cascade<K, RULE, MODE> runs a block of cascades to their ends (jg_dc_cascade.hip); the host never sees a stage.
#pragma once
#include <hip/hip_runtime.h>

#include "jg_dc_group.hpp"

namespace jg {

constexpr int DC_CASCADE_MAX = DC_GROUP_MAX;        // branches out of service in one cascade at the most, initiating ones included
constexpr int DC_CASCADE_TRUNCATED = 5;             // status: the next stage would exceed `most` (0 stable, 3 islanding; 4 is the lanes' shed status)

struct DcCascadeState {
    DcPhi phi;                               // the kept sensitivities of the last build
    int nevents = 0, lde = 0;                // lde: events rounded up to 64
    std::vector<int> h_size;                 // [nevents] initiating members
    std::vector<int> h_mon_row;              // [monitored, ascending] the row of Phi of a monitored branch
    int* e_pos = nullptr;                    // [DC_CASCADE_MAX][lde] candidate positions of the initiating members, -1 behind the last
    // the block of a run (grown on demand); ldb = its cascades rounded up to 64
    int blk_rows = 0;
    double last_trip = 1.0; int last_most = DC_CASCADE_MAX;     // of the last run: what jg_dc_cascade_time_kernel repeats
    int* b_int = nullptr;                    // [5 + 2 DC_CASCADE_MAX][ldb]: status, stages, size, pending, worst branch, the trips' labels, the trips' stages
    double* b_dbl = nullptr;                 // [1 + DC_CASCADE_MAX][ldb]: worst loading, the trips' loadings
    double* b_flow = nullptr;                // [rows][ldb] on request (kept once allocated)
    DcMem mem;                               // the device memory of the fields above (not the DcPhi's): what release frees
};

void dc_cascade_free(DcHandle* h);           // releases what the cascade screen holds, on the device and on the host (jg_dc_destroy, jg_dc_cascade_release)

}  // namespace jg
