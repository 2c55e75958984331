// jg_dc.hpp -- DC power flow and the batched DC N-1 screen on ONE shared scalar factor.
//
// Reference counterpart: dcPowerFlow / solve! (src/powerFlow/dcPowerFlow.jl:42-134: the slack row and column leave the nodal matrix
// B of dcModel! (src/powerSystem/model.jl:161-262), theta = B^-1 (supply - demand - shunt conductance - shiftPower)), and the user loop
// updateBranch!(analysis; label, status = 0) -> solve! that a planning tool runs over every branch before it spends an AC solve on the few that matter.
// An outage of branch k = (i, j) with admittance y_k moves the matrix by a rank-1 term and the right-hand side along the same vector:
//     B_s = B - y_k a a',   rhs_s = rhs - shiftAngle_k y_k a,   a = e_i - e_j  (the slack's component dropped)
// so the whole batch needs ONE factor, formed once per base case and never redone (nothing is iterated):
//     z_s     = B^-1 a                                   one sweep pair per scenario on the shared factor
//     x_s     = theta_0 - shiftAngle_k y_k z_s           theta_0 = B^-1 rhs, once per base; a lane with injections of its own: x_s = B^-1 rhs_s - ...
//     theta_s = x_s + z_s y_k (a' x_s) / (1 - y_k a' z_s)
// 1 - y_k a' z_s = 0: the branch is a bridge, the scenario gets status 3 (the code of islanding outages) and its angles are NaN.
//
// Island mode 1 ("shed") solves such a lane on the side M of the bridge that holds the slack instead.  With m the bridge's end in M, S the other side:
// every injection in S reaches M through m, so zeroing S's net injection leaves no flow on k and removing k then changes nothing in M:
//     theta_M = x_M + g z_M,   z = B^-1 e_m (slack component dropped),   g = the flow on k that LEAVES m before the outage
// the same sweep pair with ONE unit entry in the right-hand side, a combine without a denominator; status 4, NaN on S.  S is an interval of DFS preorder
// numbers (dc_island_table below), so a lane carries (lo, hi) and no bus list.
//
// It is the scalar counterpart of jg_comp.hip: the factor VALUES are wave-uniform (scalar loads of a few hundred KB), a wavefront is one row x 64
// scenarios, the only vector traffic is the right-hand sides (8 bytes per row and scenario), batch-minor with ld = batch rounded up to 64.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "jg_dc_sweep.hpp"

namespace jg {

constexpr double DC_SINGULAR = 1e-9;   // |1 - y_k a' z_s| below it: bridge.  The two sides of the difference are O(1) and carry the rounding of one sweep pair
                                       // (1e-13 on the 10k-bus grid); the smallest denominator of a non-bridge there is 3e-3.

struct DcPairState;
struct DcSeriesState;
struct DcTransferState;
struct DcGeneratorState;
struct DcGroupState;
struct DcChanceState;
struct DcCascadeState;

struct DcHandle : DcDevice {
    int n = 0, nbr = 0, batch = 0, ld = 0, slack = 0;
    double slack_angle = 0.0;
    DcFactor fac;                                           // of the nodal matrix (the factorisation tables, A, X and bad live only inside jg_dc_create)
    // base solve (one lane group, lane 0 carries the base case)
    double* rhs0 = nullptr; double* W0 = nullptr; double* th0 = nullptr;      // [n][64], [n + 1][64], [n][64]
    std::vector<double> h_rhs; bool base_dirty = true;
    // batch
    double* W = nullptr; double* Z = nullptr; double* TH = nullptr;           // [n + 1][ld], [n][ld], [n][ld]
    double* RHS = nullptr; double* XS = nullptr;                              // per-scenario injections (allocated on first use)
    int* ginj = nullptr; int* glist = nullptr; std::vector<int> h_ginj; int n_glist = 0;   // lane groups with injections of their own
    int* o_from = nullptr; int* o_to = nullptr; int* o_br = nullptr; double* o_y = nullptr; double* o_sh = nullptr;   // [ld] the lanes' outages
    int* status = nullptr;                                                     // [ld]
    // lanes with a SECOND outage (jg_dc_set_outage_pairs): allocated by the first call that names one, a handle without such a lane holds none of it
    int* o2_from = nullptr; int* o2_to = nullptr; int* o2_br = nullptr; double* o2_y = nullptr; double* o2_sh = nullptr;   // [ld]
    double* Z2 = nullptr;                                                      // [n][ld] z of the second outage, for the groups of glist2
    int* glist2 = nullptr; std::vector<int> h_o2; int n_glist2 = 0;            // lane groups that hold a second outage
    DcPairState* pair = nullptr;                                               // the N-2 screen over all pairs of a candidate list (jg_dc_pair.hpp)
    DcSeriesState* series = nullptr;                                           // the N-1 screen over a series of injection profiles (jg_dc_series.hpp)
    DcTransferState* transfer = nullptr;                                       // the transfer-capability screen over transfers x N-1 outages (jg_dc_transfer.hpp)
    DcGeneratorState* generator = nullptr;                                     // the generator-outage screen: G-1 and generator x branch cases (jg_dc_generator.hpp)
    DcGroupState* group = nullptr;                                             // the common-mode screen over named outage groups of up to 8 branches (jg_dc_group.hpp)
    DcChanceState* chance = nullptr;                                           // the probabilistic N-1 screen under Gaussian injection uncertainty (jg_dc_chance.hpp)
    DcCascadeState* cascade = nullptr;                                         // the cascading-outage screen: overload trips followed stage by stage (jg_dc_cascade.hpp)
    // island mode of the NEXT pair / series / transfer / generator build (the build takes it and sets it back to 0).  A sticky flag beside the build call is awkward -- the mode
    // belongs among the build's arguments -- but jg_dc_*_set_island_mode is part of the C ABI, so the flags stay
    int pair_shed = 0, series_shed = 0, transfer_shed = 0, generator_shed = 0;
    // bridge outages solved on the slack's island (jg_dc_set_island_mode 1): allocated by the first such call, a handle without it holds none of it
    int island_mode = 0, n_isl = 0;                                            // n_isl: lanes whose ONE outage is a bridge, set while the mode was 1
    std::vector<int> h_pre, h_blo, h_bhi, h_bside;                             // dc_island_table of the handle's branch table
    std::vector<int> h_isl_m;                                                  // [ld] m of an island lane (1-based), 0: not an island lane
    int* preorder = nullptr;                                                   // [n]
    int* isl = nullptr;                                                        // [ld][4] per lane: S end of the bridge (-1: not an island lane), lo, hi, side
    double* ipart = nullptr;                                                   // [island chunks][2][ld]: buses and right-hand side shed, per chunk of buses
    double* irec = nullptr;                                                    // [3][ld]: buses shed, right-hand side shed, g
    // branches
    std::vector<int> h_from, h_to; std::vector<double> h_y, h_shift;
    int* b_from = nullptr; int* b_to = nullptr; double* b_y = nullptr; double* b_shift = nullptr; double* b_rating = nullptr; double* rating_buf = nullptr;
    double* flows = nullptr; double* part = nullptr; double* screen = nullptr;  // [nbr][ld], [chunks][4][ld], [ld][5]
    int n_chunks = 0;
    bool solved = false;
};

int dc_base_solve(DcHandle* h);    // theta_0 = B^-1 rhs on lane 0 of the base buffers (jg_dc.hip; the build of Phi starts from it)

// Who leaves with a bridge: ONE DFS of the in-service bus graph (admittance != 0, self-loops aside) from the slack numbers the buses in preorder; the
// subtree below a tree edge is a contiguous interval of those numbers, and a tree edge (p, u) is a bridge iff no edge other than itself leaves u's subtree
// (low-link; the parent EDGE is skipped by its index, so one of two parallel branches is never a bridge).  Rooted at the slack, the subtree is the side S
// WITHOUT the slack.  Per branch: lo..hi the interval of S (lo > hi: not a bridge), side +1 / -1: the end m on the slack's side is the from / to end
// (0: not a bridge).  preorder is -1 on buses the slack does not reach.  Host only; 0-based buses.
void dc_island_table(int n, int nbr, const int* from, const int* to, const double* admittance, int slack, int* preorder, int* lo, int* hi, int* side);
// h_pre / h_blo / h_bhi / h_bside of the handle's branch table, made once (jg_dc.hip; jg_dc_set_island_mode and the shed build of jg_dc_phi.hip ask for it)
void dc_handle_island_table(DcHandle* h);

}  // namespace jg
