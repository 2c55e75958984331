// jg_dcse.hpp -- DC state estimation (weighted least squares on bus angles) with batched bad-data removal on ONE shared scalar factor.
//
// Reference counterpart: dcStateEstimation / solve! (src/stateEstimation/dcStateEstimation.jl:42-151, 342-371: rows of H are the wattmeters in stored
// order, then the PMUs at buses; the slack's column leaves H, G = H' W H with G[slack, slack] = 1, theta = G^-1 H' W z, + the slack's angle),
// residualTest! (badData.jl:48-117) and chiTest (:963-977).  H and W depend on the grid and the measurement set only, so does G: nothing is iterated,
// every realisation of a batch is one right-hand side, and a lane that drops the rows S of ITS bad measurements moves G by a low-rank term -- the
// counterpart of the outage compensation of jg_dc.hpp.  With x the lane's estimate on the FULL set, r = z - H x, U = G^-1 H_S' and
//     Omega_SS = W_SS^-1 - H_S U                               (the residual covariance of the rows S)
//     theta'   = x - U Omega_SS^-1 r_S                         (|S| = 1: theta' = x - u r_i / Omega_ii)
//     Omega'_ii = Omega_ii - q' Omega_SS^-1 q,  q = h_i U      (the residual variances of the reduced set, formed while the residual pass holds h_i)
// where Omega_ii = 1 / w_i - h_i G^-1 h_i' is computed once per factor for every row (rows of H as the lanes of the same sweep pair) and shared by all
// lanes.  Omega_SS = L D L' is extended by one row per removal; the reference refactorises G per removal and has no batch.
//
// A handle of batch 1 follows the reference instead: the caller sets the row's status to 0 and jg_dcse_set_weights re-assembles and refactorises.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "jg_dc.hpp"

namespace jg {

constexpr int DCSE_MAX_REMOVED = 4;     // |S| per lane: 4 x n x ld doubles of U (164 MB on the 10k-bus grid at 512 lanes), allocated at the first removal
constexpr int DCSE_ROWS = 32;           // rows of H per wavefront in the residual pass
constexpr int DCSE_OMEGA_LD = 512;      // lanes (= rows of H) per sweep pair of the Omega diagonal
// A pivot D_k of Omega_SS = L D L' is w_k Omega'_kk / w_k: the residual variance of row k in the set already reduced by the lane's earlier removals.
// D_k w_k <= DCSE_SINGULAR: row k is critical there (without it the grid is unobservable), the lane gets status 1 and NaN angles.  Exactly critical
// rows give 0 up to the rounding of one sweep pair against 1 / w_k (1e-13 .. 1e-10 on the grids of the tests); the smallest w_i Omega_ii of a
// non-critical row is 0.076 (case14test), 0.075 (case118) and 8.1e-4 (10k-bus grid, all 45 412 rows from a dense inverse of the gain) with injection + from
// + to wattmeters at 1e-2 and bus PMUs at 1e-5: three decades of room on either side.
constexpr double DCSE_SINGULAR = 1e-6;

struct DcseHandle : DcDevice {
    int n = 0, m = 0, batch = 0, ld = 0, slack = 0, nnz_gain = 0, nbr = 0;
    double slack_angle = 0.0;
    long long refactorisations = 0, omega_runs = 0;
    DcFactor fac;                                                       // of G (jg_dc_sweep.hpp); the tables stay for numeric refactorisations
    // H by rows (values with status 1), H' by state columns (the slack's list is empty), the terms of every entry of G
    std::vector<int> h_rptr, h_rcol; std::vector<double> h_rval, h_prec; std::vector<int> h_st;
    int* r_ptr = nullptr; int* r_col = nullptr; double* r_val = nullptr;
    int* c_ptr = nullptr; int* c_row = nullptr; double* c_val = nullptr;
    int* g_ptr = nullptr; int* g_row = nullptr; double* g_prod = nullptr; double* g_add = nullptr;
    int* st = nullptr; double* ws = nullptr; double* wi = nullptr;      // [m] status, status x precision, 1 / precision
    double* roff_t = nullptr; double* roff_c = nullptr;                 // [m] what the reference's residualTest! / chiTest subtract beyond z - H theta (jg_dcse.hip)
    double* omega = nullptr; bool omega_valid = false;                  // [m] Omega_ii of the full set
    // batch
    double* Z = nullptr; double* R = nullptr;                           // [m][ld] readings, residuals of the full-set estimate
    double* B = nullptr; double* W = nullptr; double* X0 = nullptr; double* TH = nullptr;   // [n][ld], [n + 1][ld], [n][ld] full-set estimate, [n][ld] estimate
    double* cur = nullptr;                                              // X0 or TH: the lanes' estimate, relative to the slack
    double* part = nullptr; int n_chunks = 0;                           // [chunks][3][ld]: objective, largest normalised residual, its row
    double* res = nullptr;                                              // [3][ld] the same, finished
    double* NRM = nullptr;                                              // [m][ld] all normalised residuals (allocated by the getter)
    // removal (allocated at the first removal)
    double* U = nullptr; double* TMP = nullptr;                         // [MAX_REMOVED][n][ld], [n][ld]
    double* LD = nullptr;                                               // [MAX_REMOVED^2][ld]: L below the diagonal, D on it
    int* rem = nullptr; int* cnt = nullptr; int* lstat = nullptr; int* newrow = nullptr; int* glist = nullptr;   // [MAX_REMOVED][ld], [ld], [ld], [ld], [ld / 64]
    std::vector<int> h_rem, h_cnt, h_stat; bool any_removed = false;
    // branches (power!)
    int* b_from = nullptr; int* b_to = nullptr; double* b_y = nullptr; double* b_shift = nullptr; int* o_none = nullptr;
    double* flows = nullptr; double* fpart = nullptr; int n_fchunks = 0;
    bool solved = false, have_z = false;
    // branch status tests (jg_dcse_topology.hpp): the candidates' meter columns, their denominators cached per factor like omega
    int t_count = 0; std::vector<long long> h_tbranch; std::vector<int> h_tstat; std::vector<double> h_tD, h_tnorm, h_tsgn; std::vector<int> h_tptr, h_trow;
    int* t_ptr = nullptr; int* t_row = nullptr; double* t_sgn = nullptr;        // [count + 1], [entries], [entries] +-1
    double* t_D = nullptr; double* t_norm = nullptr; int* t_stat = nullptr;     // [count]
    bool topo_valid = false; long long topo_factor = -1, topo_runs = 0;         // the value of `refactorisations` the cache belongs to
    double* XT = nullptr;                                                       // [n][ld] the corrected angles: never X0 / TH
};

// jg_dcse.hip, for jg_dcse_critical.hip: the Omega diagonal of the full set into h->omega (omega_valid), and k_dcse_row_rhs on the handle's stream --
// lane bl of B [n][ld] (zero on entry) gets row rowid[bl] of H (-1 or out of service: none) without the slack's entry
int compute_omega(DcseHandle* h);
void launch_row_rhs(DcseHandle* h, const int* rowid, double* B, int ld);

}  // namespace jg
