// jg_dcse_critical.hpp -- critical measurements and critical pairs of a DC measurement set, on the factor of the gain matrix the estimator holds.
//
// The residual covariance of the full set is Omega = W^-1 - H G^-1 H' (jg_dcse.hpp).  The bad-data test normalises r_i by sqrt(Omega_ii), so
//   a CRITICAL MEASUREMENT   w_i Omega_ii <= DCSE_SINGULAR: its residual is 0 whatever it reads, the test never names it, without it the grid is
//                            unobservable.  It takes part in no pair and is nobody's partner;
//   a CRITICAL PAIR i < j    w_j (Omega_jj - Omega_ij^2 / Omega_ii) <= DCSE_SINGULAR: the pivot k_dcse_extend meets when a lane removes i and then j
//                            (status 1), so the screen and the removal path agree by construction.  The two normalised residuals are equal up to their
//                            sign for an error on either row; the pair is reported with gamma = +-1;
//   gamma_ij = Omega_ij / sqrt(Omega_ii Omega_jj)   below that limit: how much of a bad reading on meter i shows on meter j ("interacting bad data").
// The diagonal is the handle's (compute_omega).  The off-diagonal part comes block by block: DCSE_OMEGA_LD rows j of H are the lanes of ONE sweep pair,
// U = G^-1 h_j', exactly as compute_omega forms them, and k_dcse_cross walks ALL rows i of H against that U: Omega_ij = -h_i . U[:, j] (i != j).  Per
// column j it keeps the largest |gamma_ij| and its row (strict comparison over ascending rows: the lowest row on ties; Omega is symmetric, so this is row
// j's strongest partner), and it counts -- in a second launch writes -- the records (i, j, gamma), i < j, that are critical or reach the caller's
// correlation.  No atomics: a column belongs to one lane, a (chunk of rows, group of 64 columns) to one wave.
//
// Records.  The count pass leaves one count per (chunk, column group); the host prefix-sums them in that order, so the totals are exact whatever the
// capacity.  The write pass repeats rhs + sweep pair + k_dcse_cross<true> for the blocks that hold a record below the cut and writes at offset + ballot
// rank: the device order is (chunk, group, i, j) and depends on nothing but the set.  Chunks are ranges of i, so the first `capacity` records by (i, j)
// are the whole chunks before the one where the running total passes the capacity plus a part of that chunk: the device writes through the end of that
// chunk, the host sorts by (i, j) and cuts.
#pragma once
#include "jg_dcse.hpp"

namespace jg {

// records [min(total, capacity)][3] = (i, j, gamma), 1-based rows, sorted by (i, j); totals {critical singles, critical pairs, the further pairs with
// |gamma| >= correlation}; single [m] 1: critical; partner [m] 1-based, 0: none (out of service, critical, or no other row left); partner_gamma [m]
// (NaN where partner is 0).  correlation < 0: critical pairs only.  Every pointer but totals may be null.
int dcse_critical_screen(DcseHandle* h, double correlation, long long capacity, double* records, long long* totals, int* single, int* partner,
                         double* partner_gamma);
// `reps` timings of the cross pass (k_dcse_cross count form + its finishing kernel) on the first block of columns, its sweep pair done before
int dcse_critical_time(DcseHandle* h, int reps, double* ms);

}  // namespace jg
