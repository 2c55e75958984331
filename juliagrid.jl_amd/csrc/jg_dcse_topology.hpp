// jg_dcse_topology.hpp -- branch status tests of a DC measurement set (topology errors), on the factor of the gain matrix the estimator holds.
//
// The model is z = c + H theta + e, cov(e) = W^-1, the slack's column dropped and the angles relative to the slack (jg_dcse.hpp).  The hypothesis for
// branch k: z = c + H theta + m_k phi + e with ONE more unknown phi, the flow branch k really carries from -> to minus the flow the model gives it.  The
// DC model is lossless, so the column m_k in R^m is +-1 whatever the reactance, tap or shift:
//   +1 on every from-end wattmeter of k and every injection wattmeter on from(k),
//   -1 on every to-end wattmeter of k and every injection wattmeter on to(k),
//    0 on PMUs and on rows out of service.
// Any branch is a candidate, in or out of service (then the hypothesis is "it is really closed"; its own flow meters belong to m_k although their rows
// of H are empty).  With r = z - c - H theta^ the WLS residual of the full set (the handle's R) and S = I - H G^-1 H' W:
//   g_k = H' W m_k            sparse: the columns of the few rows m_k touches, the slack's entry dropped
//   x_k = G^-1 g_k            one sweep pair on the handle's DcFactor
//   D_k = m_k' W m_k - g_k . x_k = m_k' W S m_k      grid and set only: once per factor, cached like omega
//   c_kl = m_k' W r_l         per lane l: a gather of a handful of rows of R
//   phi^_kl = c_kl / D_k,  t_kl = c_kl / sqrt(D_k)   t is N(0, 1) under "no error"; t^2 is the exact drop of the WLS objective when phi is freed
//   theta' = theta^ - x_k phi^_kl                    the WLS estimate of the augmented problem
// Status of a candidate, with N_k = m_k' W m_k:
//   0 testable          D_k > DCSE_SINGULAR N_k
//   1 critical branch   N_k > 0 but D_k at or below that: m_k lies in the range of H, a status error on k moves the estimate and leaves no residual
//                       (a leaf's only branch without a PMU behind it).  t and phi^ are NaN
//   2 unseen            m_k = 0: no meter in service sees the branch
// the same relative limit as w_i Omega_ii of a row (jg_dcse.hpp: exactly dependent columns give 0 up to the rounding of one sweep pair).
//
// What runs.  Denominators: DCSE_OMEGA_LD candidates are the lanes of ONE sweep pair; k_topo_rhs scatters +-w_i h_ij of a candidate's rows into its own
// column of B (one lane owns one column: no atomics, rows in the column's stored order), k_topo_denominator re-walks the same entries against the swept
// column.  Screen: k_topo_stat gives a wave 64 lanes of the batch and a chunk of TOPO_CHUNK candidates; D_k, the row ids, the signs and the weights are
// wave-uniform, the rows of R are read coalesced.  Per lane it keeps the largest |t| and its candidate (strict comparison over ascending candidates: the
// lowest on ties) and counts |t| >= threshold.  Correction: k_topo_rhs with the lane's own candidate, one sweep pair for the batch, k_topo_apply.
//
// Records (lane, candidate, t, phi^), the two-pass form of jg_dcse_critical.hpp: the count pass leaves one count per (chunk, group of 64 lanes); the host
// prefix-sums them in (group, chunk) order, so the totals are exact whatever the capacity; the write pass writes at offset + ballot rank, device order
// (group, chunk, candidate, lane).  Groups are ranges of lanes, so the first `capacity` records by (lane, candidate) lie in the groups up to the one where
// the running total passes the capacity: the device writes through the end of that group, the host sorts by (lane, candidate) and cuts.
#pragma once
#include "jg_dcse.hpp"

namespace jg {

constexpr int TOPO_CHUNK = 64;          // candidates per wavefront of k_topo_stat

// The candidates' meter columns: candidate q is branch `branch[q]` (1-based, kept for messages) with rows row[ptr[q] .. ptr[q + 1]) (1-based) and signs
// +-1.  Rows out of service on the handle are masked by the kernels (their weight is 0), so a status change needs no new call.  Forgets the denominators, unless the
// candidates are the ones the handle holds already.
int dcse_topology_set(DcseHandle* h, long long count, const int64_t* branch, const int64_t* ptr, const int64_t* row, const int32_t* sign);
// D, N [count] and the status into the handle's cache (topo_valid), formed if the candidates or the factor are new
int dcse_topology_denominators(DcseHandle* h);
// records [min(total, capacity)][4] = (lane, candidate, t, phi^), 1-based, sorted by (lane, candidate); totals {records, lanes with at least one};
// lane_best [batch] 1-based candidate of the largest |t| (0: no candidate is testable), lane_t / lane_phi [batch] (NaN there), lane_count [batch] the
// candidates with |t| >= threshold; dense_t [count][batch] nullable (NaN for a candidate that is not testable)
int dcse_topology_screen(DcseHandle* h, double threshold, long long capacity, double* records, long long* totals, int* lane_best, double* lane_t,
                         double* lane_phi, int* lane_count, double* dense_t);
// angle [batch][n]: lane l corrected for candidate cand[l] (1-based; <= 0 or not testable: the handle's estimate, bit for bit), the slack's angle added
int dcse_topology_correct(DcseHandle* h, const int32_t* cand, double* angle);
// `reps` timings of: 0 all denominators, 1 k_topo_rhs, 2 the sweep pair, 3 k_topo_denominator (1-3: the first block of candidates), 4 the screen's
// count pass with its finishing kernel, 5 the correction (lane l takes candidate l mod count)
int dcse_topology_time(DcseHandle* h, int kernel, int reps, double* ms);

}  // namespace jg
