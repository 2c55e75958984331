// jg_dcopf.hpp -- batched DC optimal power flow: a convex QP per lane, solved by operator splitting (ADMM in OSQP's reduced form) on ONE shared factor.
//
// Reference counterpart: dcOptimalPowerFlow / solve! (src/optimalPowerFlow/dcOptimalPowerFlow.jl:44-198, 298-370), which hands the model to a JuMP
// solver one problem at a time.  Here every lane solves
//     min 1/2 x' P x + q' x   subject to   l <= A x <= u
// with P (diagonal), q and A shared by the batch and l, u the lane's own (demand profiles in the balance rows, generator limits and outages in the
// capability rows).  With z = A x, multipliers y, step sizes rho_i per row (1e3 rho on equality rows), sigma and the relaxation alpha, one iteration is
//     b   = sigma x - q + A' (rho o z - y)
//     x~  = K^-1 b,                K = P + sigma I + A' diag(rho) A        (the shared factor: jg_dc_sweep.hpp)
//     x+  = alpha x~ + (1 - alpha) x
//     z_r = alpha A x~ + (1 - alpha) z
//     z+  = clip(z_r + y / rho, l, u)
//     y+  = y + rho (z_r - z+)
// K depends on the grid, the costs and rho only: nothing per lane is factorised.  Every `check` iterations the residuals |A x - z|, |P x + q + A' y| and
// OSQP's certificate of primal infeasibility on dy give each lane a verdict; a finished lane is frozen (its x, z, y are not written again) and a lane
// group of 64 finished lanes leaves the launches through the sweeps' group list.  rho follows the median residual ratio of the unfinished lanes
// (K is re-assembled from its term lists and refactorised numerically on the same tables).
//
// A lane may also run with ONE branch out (jg_dcopf_set_branch_outages).  With branch k (admittance y_k, buses f and t, balance rows r_f and r_t) out the
// lane's matrix is A_s = A + p d', p = -y_k (E[r_f] e_rf - E[r_t] e_rt) in row space and d = e_f - e_t in variable space; its flow and angle rows stay in
// A and are free rows (l = -inf, u = +inf: their multiplier stays 0).  Then K_s = K + a d' + d a' + s d d' = K + U C U' with a = A' (rho o p),
// s = p' (rho o p), U = [a d], C = [[0, 1], [1, s]], and
//     x~ = x0 - W (C^-1 + U' W)^-1 U' x0,   x0 = K^-1 b,   W = K^-1 U
// K is not refactorised per lane: W is two sweep pairs of batch width after every numeric factorisation, the 2 x 2 inverse is kept per lane, and an
// iteration pays a gather, a 2 x 2 product and one pass over x~.  Everywhere the iteration uses A such a lane adds the term of p d'.  A lane whose
// outage is a bridge (the host says so) never iterates: status 3.  A handle without outages runs the launches it ran before there were any.
//
// The host scales the problem once: the objective by c = 1 / max(|P|, |q|), every row of A (with l, u) to unit 2-norm.  Residuals and tolerances are
// those of the scaled problem; x, y, z and the objective leave the handle unscaled.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "jg_dc_sweep.hpp"

namespace jg {

constexpr int OPF_CHUNK = 32;               // rows of A / variables per wavefront in the residual pass
constexpr int OPF_REC = 5;                  // verdict record per lane: state, primal residual, dual residual and the norms they are relative to
constexpr double OPF_INF = 1e20;            // a bound at or beyond it is none
constexpr double OPF_EPS_INFEASIBLE = 1e-4; // OSQP's eps_prim_inf
constexpr double OPF_RHO_MIN = 1e-6, OPF_RHO_MAX = 1e6, OPF_RHO_EQ = 1e3;
// a pivot of P + A' rho A (sigma left out) at or below this share of its largest diagonal: K is singular but for sigma -- a set of variables that no
// row ties down (an island without the slack).  Every lane gets status 3
constexpr double OPF_SINGULAR = 1e-10;

struct DcopfHandle : DcDevice {
    int n = 0, m = 0, batch = 0, ld = 0, nnz_k = 0;
    double rho = 0.1, sigma = 1e-6, alpha = 1.6, cscale = 1.0, q_norm = 0.0;
    long long refactorisations = 0;
    bool singular = false, have_bounds = false, solved = false;
    DcFactor fac;                                                       // of K; the tables stay for numeric refactorisations
    // host copies: the scaled problem
    std::vector<double> h_P, h_q, h_P0, h_q0, h_E, h_rval; std::vector<int> h_rptr, h_rcol, h_eq;
    // device: A by rows and by columns, P, q, rho per row and its reciprocal, the terms of every entry of K
    int* r_ptr = nullptr; int* r_col = nullptr; double* r_val = nullptr;
    int* c_ptr = nullptr; int* c_row = nullptr; double* c_val = nullptr;
    double* Pd = nullptr; double* qd = nullptr; double* rhov = nullptr; double* rinv = nullptr;
    int* g_ptr = nullptr; int* g_row = nullptr; double* g_prod = nullptr; double* g_add = nullptr; double* g_dg = nullptr;
    // lanes, [rows or variables][ld]
    double* X = nullptr; double* XT = nullptr; double* B = nullptr; double* W = nullptr;      // x, x~, right-hand side [n][ld]; sweep scratch [n + 1][ld]
    double* Z = nullptr; double* Y = nullptr; double* DY = nullptr; double* L = nullptr; double* U = nullptr;      // [m][ld]
    int* done = nullptr; int* iters = nullptr; int* glist = nullptr;   // [ld] 0 running / 1 solved / 2 infeasible, [ld], [ld / 64]
    double* part_r = nullptr; double* part_v = nullptr; int chunks_r = 0, chunks_v = 0;      // [chunks][5][ld], [chunks][4][ld]
    double* rec = nullptr;                                              // [OPF_REC][ld]
    std::vector<int> h_done, h_iters, h_status;
    // per-lane branch outages; the device tables exist from the first jg_dcopf_set_branch_outages on, lane-fastest [.][ld]
    bool outages = false;                                               // a lane with state 1 or 3: the second instances of the kernels run
    int o_depth = 0, o_room = 0;                                        // longest list of a = A' (rho o p) in the batch; what o_ai / o_av hold
    std::vector<int> h_ostate, h_ovar, h_orow; std::vector<double> h_oy;        // [batch] 0 none / 1 outage / 3 bridge, [2][batch] 0-based, [batch] y_k
    int* o_on = nullptr;                                                // [ld] 1: the lane is corrected
    int* o_var = nullptr; int* o_row = nullptr; double* o_p = nullptr;  // [2][ld] f, t (-1: none); r_f, r_t (-1); p on r_f, r_t
    int* o_ai = nullptr; double* o_av = nullptr;                        // [o_room][ld] a as a padded (index, value) list: a pad is (0, 0.0)
    double* o_s = nullptr; double* o_M = nullptr; double* o_g = nullptr;        // [ld] s; [4][ld] (C^-1 + U' W)^-1 by rows; [2][ld] its product with U' x0
    double* o_W = nullptr;                                              // [2][n][ld] K^-1 a, K^-1 d
};

}  // namespace jg
