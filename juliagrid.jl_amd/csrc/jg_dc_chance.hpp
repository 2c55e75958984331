// jg_dc_chance.hpp -- the DC probabilistic N-1 screen under Gaussian injection uncertainty: with branch k out of service, how likely is branch m to exceed
// its rating?  On the ONE factor of a DcHandle (jg_dc.hpp) and the kept outage sensitivities (jg_dc_phi.hpp).
//
// Reference counterpart: the user loop that samples injections, updateBus! / updateGenerator! per sample around updateBranch!(k, status = 0), solve!,
// power! per branch, and counts -- dcSeriesScreen over thousands of sampled profiles.  In the DC model the question has an exact answer: the flows are
// linear in the injections, so Gaussian injections give Gaussian post-contingency flows.
//
// Injections are p = p0 + L' xi, xi ~ N(0, I_r), L [r][buses] the factors (a truncated PCA of a forecast-error covariance, one scaled unit vector per
// independent wind farm).  The slack takes what a factor does not balance: a factor's slack entry is taken as 0 (dc_phi_row_flows).  On the rows
// R = monitored u candidates of a DcPhi:
//     f0[m]                                  the base flow of p0, with the shift angles
//     S[m,j] = y_m a_m' B^-1 L_j             the sensitivity of the flow to factor j, without them (dc_phi_row_flows, shift false: r right-hand sides)
//     base case:   mu_m = f0[m],   sigma_m = ||S[m,:]||_2
//     outage of candidate k, d_k = 1 - Phi[k,k], |d_k| >= DC_SINGULAR, m != k:
//         g = Phi[m,k] / d_k,   mu_m(k) = f0[m] + g f0[k],   sigma_m(k) = sqrt(sum_j (S[m,j] + g S[k,j])^2);     m = k: mu = sigma = 0
//     P_m(k) = 1/2 erfc((R_m - mu) / (sigma sqrt 2)) + 1/2 erfc((R_m + mu) / (sigma sqrt 2)),   R_m the rating;   sigma == 0: 1 if |mu| > R_m, else 0
// An unrated row (row_rinv == 0) has P = 0 and enters no count and no record.  |d_k| < DC_SINGULAR: the candidate is a bridge, status 3, NaN, as in the
// series screen; there is no shed mode.
//
// The variance is summed as the squares of the COMBINED sensitivities, never expanded to v_m + 2 g <S_m, S_k> + g^2 v_k with a Gram matrix: where k is in
// series with m the flow of m is certain after the outage and g S_k = -S_m exactly; the expanded form then returns about 1e-16 v_m instead of 0, the square
// root turns that into about 1e-8 of scale in sigma -- above the project's 1e-9 bound -- while the direct sum returns the rounding of r additions.
//
// What is kept: a DcPhi of the state's own, S [rows][lds] with lds = r rounded up to 8 and zeros behind r, the bridges on the host, and the buffers of a
// block of candidates with ONE record list (jg_dc_records.hpp): records (k label, branch label, mu, sigma, P), sorted by (k, branch).
#pragma once
#include <hip/hip_runtime.h>

#include "jg_dc_records.hpp"

namespace jg {

constexpr int DC_CHANCE_MAX = 32;            // factors at the most; the screen kernel comes as R = 8, 16, 32, chosen by lds

struct DcChanceState {
    DcPhi phi;                               // the kept sensitivities of the last build (row_f0 / cand_f0: of `injection` where the build was given one)
    int r = 0, lds = 0;
    double* S = nullptr;                     // [rows][lds]
    std::vector<char> h_bridge;              // [nk] 1: |1 - Phi[k,k]| < DC_SINGULAR
    std::vector<int> h_mon_row;              // [monitored, ascending] the row of Phi of a monitored branch
    double* base = nullptr;                  // [rows][3] mu, sigma, P without an outage (k_chance_base)
    // the block of a screen call (grown on demand)
    int blk_rows = 0;
    double* b_worst = nullptr; int* b_branch = nullptr;      // [blk_rows]
    int* b_wcnt = nullptr;                   // [DC_PAIR_WAVES][blk_rows rounded up to 64] records per wave's share of the rows: where a wave's records start
    double* b_dense = nullptr;               // [3][rows][blk_rows rounded up to 64] mu, sigma, P on request
    DcRecords viol{5 * sizeof(double)};
    double build_ms[3] = {0, 0, 0};          // S of the last build: total, sweep pairs, flow kernel (HIP events)
    DcMem mem;                               // the device memory of the fields above (not the DcPhi's): what release frees
};

void dc_chance_free(DcHandle* h);            // releases what the chance screen holds, on the device and on the host (jg_dc_destroy, jg_dc_chance_release)

}  // namespace jg
