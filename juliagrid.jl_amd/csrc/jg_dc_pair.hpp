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
// What is kept: Phi on the rows R = monitored u candidates (ascending branch index), columns = candidates, [rows][ldk] doubles with ldk = candidates
// rounded up to 64 -- the sweep pair of jg_dc_sweep.hip runs once per candidate (a lane batch at a time), never per pair.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace jg {

#ifndef JG_DC_PAIR_TILE
#define JG_DC_PAIR_TILE 4                    // probe builds: -DJG_DC_PAIR_TILE=8 (the A/B of DESIGN.md 3.9)
#endif
constexpr int DC_PAIR_TILE = JG_DC_PAIR_TILE;   // candidates k a wave of the screen kernel keeps in registers: a row of Phi is loaded once for all of them
constexpr int DC_PAIR_WAVES = 4;             // waves of a workgroup of the screen kernel: they share ONE chunk of 64 l, so its Phi rows meet in the vector L1
constexpr int DC_PAIR_LANES = 512;           // candidates per sweep pair of the build (a lane batch)
constexpr double DC_PAIR_BUDGET = 0.8;       // default budget of jg_dc_pair_build: this fraction of the free device memory
static_assert(DC_PAIR_TILE == 4 || DC_PAIR_TILE == 8, "a tile of k is one or two 32-byte scalar loads of a row of Phi");

struct DcPairState {
    int nk = 0, ldk = 0, rows = 0;
    std::vector<int> h_cand;                 // [nk] candidate branches (0-based, strictly ascending)
    double* Phi = nullptr;                   // [rows][ldk]
    int* row_branch = nullptr;               // [rows] branch of a row (0-based, ascending)
    int* row_pos = nullptr;                  // [rows] position of the row's branch in the candidate list, -1: not a candidate
    int* row_mon = nullptr;                  // [rows] 1: monitored
    double* row_f0 = nullptr;                // [rows] base-case flow
    double* row_rinv = nullptr;              // [rows] 1 / rating of a monitored, rated row, else 0 (every screen call sets it from the handle's rating)
    int* cand_row = nullptr;                 // [ldk] row of a candidate
    int* cand_label = nullptr;               // [ldk] 1-based branch label of a candidate
    double* cand_diag = nullptr;             // [ldk] Phi[k,k]
    double* cand_f0 = nullptr;               // [ldk]
    // shed mode of the series / transfer build (jg_dc_series.hpp): a bridge candidate's column holds Z[:,k] = y_l a_l' B^-1 e_m instead of Phi[:,k]
    bool shed = false;
    std::vector<int> h_side, h_lo, h_hi;     // [nk] dc_island_table of the candidates: side 0: not a bridge; lo .. hi the preorder interval of what leaves
    int* cand_isl = nullptr;                 // [ldk][4] side, lo, hi, 0 ((0, 1, 0, 0): not a bridge, the interval is empty)
    int* row_pre = nullptr;                  // [rows] preorder number of the from end of the row's branch
    // the row block of a screen call (grown on demand)
    int blk_rows = 0;
    double* b_load = nullptr; int* b_branch = nullptr; int* b_count = nullptr; double* b_det = nullptr;     // [blk_rows][ldk]; b_det only on request
    int* r_viol = nullptr; int* r_isl = nullptr; double* r_max = nullptr; long long* r_off = nullptr; long long* r_ioff = nullptr;    // [blk_rows]
    double* c_max = nullptr;                 // [ldk]
    double* rec = nullptr; long long rec_cap = 0;       // [rec_cap][5]
    long long* isl = nullptr; long long isl_cap = 0;    // [isl_cap][2]
    double build_ms[3] = {0, 0, 0};          // the last build: total, sweep pairs, Phi kernel (HIP events)
};

struct DcHandle;
void dc_pair_free(DcHandle* h);              // releases what the pair screen holds, on the device and on the host (jg_dc_destroy, jg_dc_pair_release)

// The build of Phi is shared with the series screen (jg_dc_series.hpp), which keeps a state of its own beside h->pair:
//   dc_pair_lists        the candidate / monitored lists of a build call (1-based in, 0-based out) with the checks of jg_dc_pair_build; 1 and h->error
//   dc_pair_state_build  replaces `slot` by a fresh build.  `extra` bytes the caller keeps beside Phi count in the memory question (code 5, nothing
//                        allocated, `extra_text` names them in the message); info [8] as jg_dc_pair_build.  `shed`: the candidates the handle's island
//                        table (dc_island_table, the graph) calls bridges get the sweep pair on e_m and the tables above
//   dc_pair_state_rinv   row_rinv from the handle's rating (a launch on the handle's stream)
int dc_pair_lists(DcHandle* h, const std::string& who, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, std::vector<int>& cand,
                  std::vector<int>& mon);
int dc_pair_state_build(DcHandle* h, DcPairState*& slot, const char* who, const std::vector<int>& cand, const std::vector<int>& mon, int64_t budget,
                        size_t extra, const std::string& extra_text, double* info, bool shed = false);
void dc_pair_state_free(DcHandle* h, DcPairState*& slot);
void dc_pair_state_rinv(DcHandle* h, DcPairState* p);
std::string dc_pair_bytes_text(size_t b);

}  // namespace jg
