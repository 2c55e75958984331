// jg_dclav.hpp -- batched DC least-absolute-value state estimation: a primal-dual interior-point method per lane on a lane-valued factor of the gain.
//
// Reference counterpart: dcLavStateEstimation / solve! (src/stateEstimation/dcStateEstimation.jl:201-313, src/backend/expressions.jl:381-421), where the
// model goes to a JuMP solver.  The rows are those of the DC WLS model (jg_dcse.hpp): wattmeters in stored order, then the PMUs at buses; the slack's angle
// is fixed; a row with status 0 has both deviations fixed at 0 and leaves the model.  Unweighted, as in the reference:
//     minimise  sum_i (u_i + v_i)   subject to   h_i theta + u_i - v_i = z_i,  u, v >= 0,  theta_slack = 0          (= min |z - H theta|_1)
//     dual:     maximise z'y        subject to   H'y = 0,  -1 <= y <= 1
// Per lane, Mehrotra's predictor-corrector on that pair.  State theta, u > 0, v > 0, y in (-1, 1);
//     rp = z - H theta - u + v,   rd = -H'y,   complementarity u (1 - y), v (1 + y),   d = u / (1 - y) + v / (1 + y),   Q = 1 / d
// and with the targets cu, cv of the two complementarity products, c = cu / (1 - y) - cv / (1 + y):
//     (H' Q H) dtheta = H' (Q (rp - c)) - rd,   dy = Q (rp - c - H dtheta),   du = (cu + u dy) / (1 - y),   dv = (cv - v dy) / (1 + y)
// One iteration: assemble G = H' Q H from the gain's term lists (the slack's row and column the identity), factorise it per lane
// (jg_dc_lanefactor.hpp), predictor (cu = -u (1 - y), cv = -v (1 + y)), step length a to the boundary, sigma = (affine gap / gap)^3, corrector
// (cu = sigma mu - u (1 - y) + du_a dy_a, cv = sigma mu - v (1 + y) - dv_a dy_a) on the same factor, a step of DCLAV_STEP_BACK of the way to the boundary,
// the same length on the primal and the dual side.  Start: theta the unit-weight least-squares estimate (one solve with Q = 1), u = max(r0, 0) + s,
// v = max(-r0, 0) + s, s = max(mean |r0|, DCLAV_START_FLOOR), y = 0.  A lane is finished when
//     max |rp| <= tol (1 + max |z|),   max |rd| <= tol max_j sum_i |H_ij|,   gap <= tol (1 + |z - H theta|_1)
// It is then frozen: nothing of its state is written again, and a group of 64 finished lanes leaves the launches through the group list.
// Status: 0 solved, 5 iteration limit, 1 the in-service rows do not observe the grid (a bad pivot of the Q = 1 factorisation: every lane, NaN
// angles), 3 a bad pivot in a later iteration of that lane (frozen at its last iterate).  tests/dclav_reference.py restates the method in numpy.
//
// Every sum over rows or states that decides something (the tests above, the step length, sigma) is formed per chunk and finished over the chunks in
// ascending order (part / res of jg_dcse.hip), so a lane's iterates do not depend on the batch it runs in or on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "jg_dc_lanefactor.hpp"

namespace jg {

constexpr int DCLAV_ROWS = 32;                  // rows of H per wavefront in the row, step and update passes
constexpr int DCLAV_COLS = 8;                   // state columns of H' per wavefront in the column pass
constexpr double DCLAV_STEP_BACK = 0.995;
constexpr double DCLAV_START_FLOOR = 1e-8;
constexpr int DCLAV_LRES_GAP = 1;               // the row of lres that holds the gap

struct DclavHandle : DcDevice {
    int n = 0, m = 0, batch = 0, ld = 0, slack = 0, nnz_gain = 0, nbr = 0, m_in = 0;
    double slack_angle = 0.0, hnorm = 0.0;      // hnorm: max_j sum_i |H_ij| over the in-service rows; slack = -1: no fixed state (lav_create)
    DcLaneFactor fac;                           // of G = H' Q H, values per lane
    std::vector<int> h_rptr, h_rcol; std::vector<double> h_rval; std::vector<int> h_st;
    int* r_ptr = nullptr; int* r_col = nullptr; double* r_val = nullptr;            // H by rows, the slack's column zeroed
    int* c_ptr = nullptr; int* c_row = nullptr; double* c_val = nullptr;            // H' by state columns, the slack's list empty
    int* g_ptr = nullptr; int* g_row = nullptr; double* g_prod = nullptr; double* g_add = nullptr;
    int* st = nullptr;                                                              // [m]
    // per (row, lane), [m][ld]
    double* Z = nullptr; double* U = nullptr; double* V = nullptr; double* Y = nullptr;
    double* R = nullptr; double* RP = nullptr; double* Q = nullptr; double* T = nullptr;      // z - H theta, rp, Q, Q (rp - c)
    double* DYA = nullptr; double* DY = nullptr;                                                // dy of the predictor, of the corrector
    // per (state, lane), [n][ld] (W: [n + 1][ld])
    double* TH = nullptr; double* DT = nullptr; double* B = nullptr; double* RD = nullptr; double* W = nullptr;
    double* part = nullptr; int n_chunks = 0;   // [chunks][4][ld]: max |rp|, gap, objective, max |z| (row pass); slot 0 the boundary ratio, slot 1 the affine gap
    double* partc = nullptr; int n_cchunks = 0; // [column chunks][ld]: max |rd|
    double* lres = nullptr;                     // [6][ld]: objective, gap (both as of the lane's verdict), step length, sigma mu, the start's s, spare
    int* done = nullptr; int* lstat = nullptr; int* liter = nullptr;      // [ld]
    int* gact = nullptr; int* glist = nullptr; int* d_count = nullptr;    // [ld / 64] a group has a running lane; those groups; how many
    int* p_count = nullptr;                     // pinned: the word the host reads after an iteration's verdict
    std::vector<double> h_theta0; bool have_init = false;
    int* b_from = nullptr; int* b_to = nullptr; double* b_y = nullptr; double* b_shift = nullptr; int* o_none = nullptr;
    double* flows = nullptr; double* fpart = nullptr; int n_fchunks = 0;
    size_t bytes_per_lane = 0;
    long long factorisations = 0; int last_iterations = 0;
    bool solved = false, have_z = false, unobservable = false;
};

// The same iteration WITHOUT a fixed state, for a model that observes its own reference (jg_pmulav.hpp: phasors): the gain carries no added diagonal
// entry, no column of H is zeroed and theta has no offset; every kernel, launch and table is the one jg_dclav_create builds.  `who` names the entry
// point in the text of a refused budget, `extra_b` is what it holds per lane beside the iterates.  h_theta0 / have_init: [batch][n], used once.
int lav_create(DclavHandle* h, const char* who, size_t extra_b, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status,
               int64_t batch, int device);
void lav_release(DclavHandle* h);                               // everything the handle owns but the handle itself
int lav_set_status(DclavHandle* h);                             // h_st -> the device, the in-service count and hnorm
int lav_run(DclavHandle* h, int maxit, double tol);            // the start and the iteration of jg_dclav_solve
int lav_time(DclavHandle* h, int kernel, int reps, double* ms); // the parts 0 .. 4 of jg_dclav_time_kernel
int lav_upload(DclavHandle* h, double* dev, size_t rows, const double* src, size_t lane0, size_t count);      // [count][rows] -> lanes lane0 .. of [rows][ld]
int lav_fetch(DclavHandle* h, const double* dev, size_t rows, double* out);                                   // [rows][ld] -> [batch][rows]

}  // namespace jg
