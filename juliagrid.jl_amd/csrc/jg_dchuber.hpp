// jg_dchuber.hpp -- batched DC Huber / Schweppe-Huber state estimation: the interior-point method of jg_dclav.hpp on the Huber QP, per lane, on the
// lane-valued factor of the gain (jg_dc_lanefactor.hpp).
//
// The reference has no counterpart: its DC estimators are WLS (jg_dcse.hpp) and LAV (jg_dclav.hpp).  The rows are theirs, row i scaled by 1 / sigma_i on
// the host, so the device sees H~, z~ and unit weights, and a bound kappa_i = c omega_i > 0 per row, shared by the lanes (omega = 1: Huber; omega in
// (0, 1]: Schweppe's leverage weights):
//     minimise  1/2 sum s_i^2 + sum kappa_i (u_i + v_i)   subject to   h~_i theta + s_i + u_i - v_i = z~_i,  u, v >= 0,  theta_slack = 0
//               (= min sum rho_kappa_i(z~_i - h~_i theta), rho Huber's function: quadratic up to kappa, linear beyond)
//     dual:     maximise z~'y - 1/2 y'y   subject to   H~'y = 0,  -kappa <= y <= kappa,   with s = y
// Per lane, Mehrotra's predictor-corrector on that pair.  State theta, u > 0, v > 0, y in (-kappa, kappa);
//     rp = z~ - H~ theta - y - u + v,   rd = -H~'y,   complementarity u (kappa - y), v (kappa + y),   d = 1 + u / (kappa - y) + v / (kappa + y),   Q = 1 / d
// and with the targets cu, cv of the two complementarity products, c = cu / (kappa - y) - cv / (kappa + y):
//     (H~' Q H~) dtheta = H~' (Q (rp - c)) - rd,   dy = Q (rp - c - H~ dtheta),   du = (cu + u dy) / (kappa - y),   dv = (cv - v dy) / (kappa + y)
// This is the LAV iteration with 1 replaced by kappa_i and one more term, the 1 of the quadratic part, in d.  One iteration: assemble G = H~' Q H~ from
// the gain's term lists, factorise it per lane, predictor (cu = -u (kappa - y), cv = -v (kappa + y), so rp - c = r - y), step length to the boundary of u,
// v, kappa - y, kappa + y, sigma = (affine gap / gap)^3, mu = gap / (2 in-service rows), corrector (cu = sigma mu - u (kappa - y) + du_a dy_a,
// cv = sigma mu - v (kappa + y) - dv_a dy_a) on the same factor, a step of DCHUBER_STEP_BACK of the way to the boundary, one length for both sides.
// Start: theta the least-squares estimate (one solve with Q = 1: the WLS estimate itself), r0 = z~ - H~ theta, y = clip(r0, +-kappa / 2), r1 = r0 - y,
// s = max(mean |r1|, DCHUBER_START_FLOOR), u = max(r1, 0) + s, v = max(-r1, 0) + s.  A lane is finished when
//     max |rp| <= tol (1 + max |z~|),   max |rd| <= tol max_j sum_i |H~_ij| max kappa,   gap <= tol (1 + 1/2 y'y + kappa'(u + v))
// It is then frozen, and a group of 64 finished lanes leaves the launches through the group list.  After the last verdict one pass forms per row the
// unscaled residual sigma_i r~_i, the weight min(1, kappa_i / |r~_i|) (1 at r~_i = 0) and the lane's Huber loss sum rho.
// Status: 0 solved, 5 iteration limit, 1 the in-service rows do not observe the grid (a bad pivot of the Q = 1 factorisation: every lane, NaN), 3 a bad
// pivot in a later iteration of that lane (frozen at its last iterate).  tests/dchuber_reference.py restates the method in numpy.
//
// Every sum, maximum or minimum over rows or states that decides something is formed per chunk and finished over the chunks in ascending order (part /
// res of jg_dcse.hip), so a lane's iterates do not depend on the batch it runs in or on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "jg_dc_lanefactor.hpp"

namespace jg {

constexpr int DCHUBER_ROWS = 32;                // rows of H per wavefront in the row, step and final passes
constexpr int DCHUBER_COLS = 8;                 // state columns of H' per wavefront in the column pass
constexpr double DCHUBER_STEP_BACK = 0.995;
constexpr double DCHUBER_START_FLOOR = 1e-8;

struct DchuberHandle : DcDevice {
    int n = 0, m = 0, batch = 0, ld = 0, slack = 0, nnz_gain = 0, nbr = 0, m_in = 0;
    double slack_angle = 0.0, hnorm = 0.0, kmax = 0.0;      // hnorm: max_j sum_i |H_ij|, kmax: max kappa_i, both over the in-service rows
    DcLaneFactor fac;                           // of G = H' Q H, values per lane
    std::vector<int> h_rptr, h_rcol; std::vector<double> h_rval, h_kappa; std::vector<int> h_st;
    int* r_ptr = nullptr; int* r_col = nullptr; double* r_val = nullptr;            // H by rows, the slack's column zeroed
    int* c_ptr = nullptr; int* c_row = nullptr; double* c_val = nullptr;            // H' by state columns, the slack's list empty
    int* g_ptr = nullptr; int* g_row = nullptr; double* g_prod = nullptr; double* g_add = nullptr;
    int* st = nullptr; double* K = nullptr; double* SG = nullptr;                   // [m]: status, kappa, sigma (what the scaled residual is multiplied by)
    // per (row, lane), [m][ld]
    double* Z = nullptr; double* U = nullptr; double* V = nullptr; double* Y = nullptr;
    double* R = nullptr; double* RP = nullptr; double* Q = nullptr; double* T = nullptr;      // z - H theta, rp, Q, Q (rp - c)
    double* DYA = nullptr; double* DY = nullptr;                                                // dy of the predictor, of the corrector
    double* RES = nullptr; double* WT = nullptr;                                                // the final pass: unscaled residual, weight
    // per (state, lane), [n][ld] (W: [n + 1][ld])
    double* TH = nullptr; double* DT = nullptr; double* B = nullptr; double* RD = nullptr; double* W = nullptr;
    double* part = nullptr; int n_chunks = 0;   // [chunks][4][ld]: max |rp|, gap, primal objective, max |z| (row pass); slot 0 the boundary ratio, slot 1 the affine gap; slot 2 the loss (final pass)
    double* partc = nullptr; int n_cchunks = 0; // [column chunks][ld]: max |rd|
    double* lres = nullptr;                     // [6][ld]: primal objective, gap (both as of the lane's verdict), step length, sigma mu, the start's s, the Huber loss
    int* done = nullptr; int* lstat = nullptr; int* liter = nullptr;      // [ld]
    int* gact = nullptr; int* glist = nullptr; int* d_count = nullptr;    // [ld / 64] a group has a running lane; those groups; how many
    int* p_count = nullptr;                     // pinned: the word the host reads after an iteration's verdict
    int* b_from = nullptr; int* b_to = nullptr; double* b_y = nullptr; double* b_shift = nullptr; int* o_none = nullptr;
    double* flows = nullptr; double* fpart = nullptr; int n_fchunks = 0;
    size_t bytes_per_lane = 0;
    long long factorisations = 0; int last_iterations = 0;
    bool solved = false, have_z = false, unobservable = false;
};

}  // namespace jg
