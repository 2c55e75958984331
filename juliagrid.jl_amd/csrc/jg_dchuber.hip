// jg_dchuber.hip -- batched DC Huber / Schweppe-Huber state estimation (jg_dchuber.hpp has the model and the method).  The lane-valued factorisation and
// sweeps are jg_dc_lanefactor.hip's, the launch sequence is jg_dclav.hip's; here: the passes of the interior-point iteration on the Huber QP (a bound
// kappa per row, the 1 of the quadratic part in d), the verdict with the group list, the final pass (unscaled residual, weight, loss), the C ABI.
// Coefficient values, bounds and indices are wave-uniform and go through scalar loads; every store is a vector store.
#include "jg_dchuber.hpp"
#include "jg_dc_abi.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/jgrid.h"
#include "jg_engine.hpp"

namespace jg {

namespace {

// ---- gain assembly: the statement of k_lav_gain (jg_dclav.hip), restated: G[e][lane] = sum over the entry's terms of (coefficient product) x Q[row][lane],
// + 1 on the slack's diagonal -------------------------------------------------------------------------------------------------------------------------
struct HubGainArgs { const int* g_ptr; const int* g_row; const double* g_prod; const double* g_add; const double* Q; double* A; const int* groups; int nnz, ld; };
__global__ __launch_bounds__(256) void k_hub_gain(HubGainArgs a) {
    const int e = blockIdx.x * 4 + uniform(threadIdx.y);
    if (e >= a.nnz) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double s = ((CDbl)a.g_add)[e];
    for (int t = ((CInt)a.g_ptr)[e]; t < ((CInt)a.g_ptr)[e + 1]; ++t) s = fma(((CDbl)a.g_prod)[t], a.Q[(size_t)((CInt)a.g_row)[t] * ld + bl], s);
    a.A[(size_t)e * ld + bl] = s;
}

// ---- the passes over rows of H: DCHUBER_ROWS rows per wavefront, lanes as lanes ----------------------------------------------------------------
struct HubArgs {
    const int* r_ptr; const int* r_col; const double* r_val; const int* st; const double* K; const double* SG;
    const int* c_ptr; const int* c_row; const double* c_val;
    double* Z; double* U; double* V; double* Y; double* R; double* RP; double* Q; double* T; double* DYA; double* DY; double* RES; double* WT;
    double* TH; double* DT; double* B; double* RD;
    double* part; double* partc; double* lres;
    int* done; int* lstat; int* liter; const int* bad; int* gact;
    const int* groups;
    int m, n, ld, n_chunks, n_cchunks, m_in, batch;
};
constexpr int HR_OBJ = 0, HR_GAP = 1, HR_ALPHA = 2, HR_SMU = 3, HR_START = 4, HR_LOSS = 5;

__device__ __forceinline__ double hub_dot(const HubArgs& a, int i, const double* X, size_t ld, size_t bl) {
    double s = 0.0;
    for (int p = ((CInt)a.r_ptr)[i]; p < ((CInt)a.r_ptr)[i + 1]; ++p) s = fma(((CDbl)a.r_val)[p], X[(size_t)((CInt)a.r_col)[p] * ld + bl], s);
    return s;
}
__device__ __forceinline__ double hub_clip(double r, double b) { return fmin(fmax(r, -b), b); }
// the predictor's du, dv from its dy (targets -u (kappa - y), -v (kappa + y))
__device__ __forceinline__ void hub_affine(double u, double v, double y, double k, double dya, double& dua, double& dva) {
    dua = -u + u * dya / (k - y);
    dva = -v - v * dya / (k + y);
}
// the corrector's targets: sigma mu, minus the product, plus the second-order term of the predictor
__device__ __forceinline__ void hub_targets(double u, double v, double y, double k, double dya, double smu, double& cu, double& cv) {
    double dua, dva;
    hub_affine(u, v, y, k, dya, dua, dva);
    cu = smu - u * (k - y) + dua * dya;
    cv = smu - v * (k + y) - dva * dya;
}
// the largest step that keeps u, v, kappa - y, kappa + y at or above 0
__device__ __forceinline__ double hub_ratio(double u, double v, double y, double k, double du, double dv, double dy) {
    double r = HUGE_VAL;
    if (du < 0.0) r = fmin(r, -u / du);
    if (dv < 0.0) r = fmin(r, -v / dv);
    if (dy > 0.0) r = fmin(r, (k - y) / dy);
    if (dy < 0.0) r = fmin(r, -(k + y) / dy);
    return r;
}

// START: r0 = z - H theta and the partial of sum |r0 - clip(r0, +-kappa / 2)|.  Otherwise r, rp, d, Q, T = Q (r - y) (the predictor's rp - c) and the
// partials of max |rp|, the gap, the primal objective and max |z|
template <bool START>
__global__ __launch_bounds__(256) void k_hub_row(HubArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * DCHUBER_ROWS;
    if (i0 >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double pmax = 0.0, gap = 0.0, obj = 0.0, zmax = 0.0;
    for (int i = i0; i < min(i0 + DCHUBER_ROWS, a.m); ++i) {
        const size_t o = (size_t)i * ld + bl;
        if (!((CInt)a.st)[i]) {
            a.R[o] = 0.0;
            if (!START) { a.RP[o] = 0.0; a.Q[o] = 0.0; a.T[o] = 0.0; }
            continue;
        }
        const double k = ((CDbl)a.K)[i];
        const double z = a.Z[o], r = z - hub_dot(a, i, a.TH, ld, bl);
        a.R[o] = r;
        if (START) { obj += fabs(r - hub_clip(r, 0.5 * k)); continue; }
        const double u = a.U[o], v = a.V[o], y = a.Y[o];
        const double rp = r - y - u + v, q = 1.0 / (1.0 + u / (k - y) + v / (k + y));
        a.RP[o] = rp; a.Q[o] = q; a.T[o] = q * (r - y);
        pmax = fmax(pmax, fabs(rp));
        gap += u * (k - y) + v * (k + y);
        obj += 0.5 * y * y + k * (u + v);
        zmax = fmax(zmax, fabs(z));
    }
    double* p = a.part + (size_t)chunk * 4 * ld + bl;
    p[0] = pmax; p[ld] = gap; p[2 * ld] = obj; p[3 * ld] = zmax;
}
// the start: Q = status, T = status z (the right-hand side H'z of the least-squares estimate)
__global__ __launch_bounds__(256) void k_hub_prep(HubArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m) return;
    const size_t o = (size_t)i * a.ld + lane_of(a.groups);
    const int s = ((CInt)a.st)[i];
    a.Q[o] = s ? 1.0 : 0.0;
    a.T[o] = s ? a.Z[o] : 0.0;
}
// s = max(mean |r1|, floor), chunks in ascending order
__global__ __launch_bounds__(64) void k_hub_start_finish(HubArgs a) {
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double obj = 0.0;
    for (int c = 0; c < a.n_chunks; ++c) obj += a.part[((size_t)c * 4 + 2) * ld + bl];
    a.lres[(size_t)HR_START * ld + bl] = fmax(obj / (double)a.m_in, DCHUBER_START_FLOOR);
}
__global__ __launch_bounds__(256) void k_hub_init(HubArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups), o = (size_t)i * ld + bl;
    const int s = ((CInt)a.st)[i];
    const double r0 = a.R[o], y = hub_clip(r0, 0.5 * ((CDbl)a.K)[i]), r1 = r0 - y, e = a.lres[(size_t)HR_START * ld + bl];
    a.U[o] = s ? fmax(r1, 0.0) + e : 0.0;
    a.V[o] = s ? fmax(-r1, 0.0) + e : 0.0;
    a.Y[o] = s ? y : 0.0;
}

// ---- the pass over columns of H (rows of H'): a gather, DCHUBER_COLS states per wavefront -------------------------------------------------------
// B = H'T - rd.  WITH_RD: rd = -H'y is formed here, stored, and its largest magnitude goes to partc; otherwise the stored rd is read
template <bool WITH_RD>
__global__ __launch_bounds__(256) void k_hub_col(HubArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int j0 = chunk * DCHUBER_COLS;
    if (j0 >= a.n) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double dmax = 0.0;
    for (int j = j0; j < min(j0 + DCHUBER_COLS, a.n); ++j) {
        double t = 0.0, hy = 0.0;
        for (int p = ((CInt)a.c_ptr)[j]; p < ((CInt)a.c_ptr)[j + 1]; ++p) {
            const size_t o = (size_t)((CInt)a.c_row)[p] * ld + bl;
            const double v = ((CDbl)a.c_val)[p];
            t = fma(v, a.T[o], t);
            if (WITH_RD) hy = fma(v, a.Y[o], hy);
        }
        const size_t o = (size_t)j * ld + bl;
        double rd;
        if (WITH_RD) { rd = -hy; a.RD[o] = rd; dmax = fmax(dmax, fabs(rd)); }
        else rd = a.RD[o];
        a.B[o] = t - rd;
    }
    if (WITH_RD) a.partc[(size_t)chunk * ld + bl] = dmax;
}

// ---- the verdict: the three tests, the freeze, the groups that still run --------------------------------------------------------------------------
// one workgroup of 64 per lane group, ALL groups; chunks in ascending order.  dbound = max_j sum_i |H_ij| x max kappa
__global__ __launch_bounds__(64) void k_hub_verdict(HubArgs a, int it, int maxit, double tol, double dbound) {
    const size_t ld = (size_t)a.ld, bl = (size_t)blockIdx.x * 64 + threadIdx.x;
    int active = 0;
    if (!a.done[bl]) {
        double pmax = 0.0, gap = 0.0, obj = 0.0, zmax = 0.0, dmax = 0.0;
        for (int c = 0; c < a.n_chunks; ++c) {
            const double* p = a.part + (size_t)c * 4 * ld + bl;
            pmax = fmax(pmax, p[0]); gap += p[ld]; obj += p[2 * ld]; zmax = fmax(zmax, p[3 * ld]);
        }
        for (int c = 0; c < a.n_cchunks; ++c) dmax = fmax(dmax, a.partc[(size_t)c * ld + bl]);
        a.lres[(size_t)HR_OBJ * ld + bl] = obj;
        a.lres[(size_t)HR_GAP * ld + bl] = gap;
        if (it > 0 && a.bad[bl]) { a.lstat[bl] = 3; a.liter[bl] = it - 1; a.done[bl] = 1; }        // the step of iteration it - 1 was not applied
        else if (pmax <= tol * (1.0 + zmax) && dmax <= tol * dbound && gap <= tol * (1.0 + obj)) { a.lstat[bl] = 0; a.liter[bl] = it; a.done[bl] = 1; }
        else if (it >= maxit) { a.lstat[bl] = 5; a.liter[bl] = it; a.done[bl] = 1; }
        else active = 1;
    }
    const unsigned long long any = __ballot(active);
    if (threadIdx.x == 0) a.gact[blockIdx.x] = any != 0ull;
}
__global__ void k_hub_glist(const int* gact, int* glist, int* count, int groups) {
    if (blockIdx.x || threadIdx.x) return;
    int c = 0;
    for (int g = 0; g < groups; ++g)
        if (gact[g]) glist[c++] = g;
    *count = c;
}

// ---- steps ---------------------------------------------------------------------------------------------------------------------------------------
// dy = Q (rp - c - H dtheta), du, dv, and the chunk's ratio to the boundary.  CORR false: the predictor (rp - c = r - y); true: the corrector
template <bool CORR>
__global__ __launch_bounds__(256) void k_hub_step(HubArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * DCHUBER_ROWS;
    if (i0 >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    const double smu = CORR ? a.lres[(size_t)HR_SMU * ld + bl] : 0.0;
    double ratio = HUGE_VAL;
    for (int i = i0; i < min(i0 + DCHUBER_ROWS, a.m); ++i) {
        const size_t o = (size_t)i * ld + bl;
        if (!((CInt)a.st)[i]) { (CORR ? a.DY : a.DYA)[o] = 0.0; continue; }
        const double k = ((CDbl)a.K)[i];
        const double hd = hub_dot(a, i, a.DT, ld, bl);
        const double u = a.U[o], v = a.V[o], y = a.Y[o], q = a.Q[o];
        double dy, du, dv;
        if (!CORR) {
            dy = q * (a.R[o] - y - hd);
            a.DYA[o] = dy;
            hub_affine(u, v, y, k, dy, du, dv);
        } else {
            double cu, cv;
            hub_targets(u, v, y, k, a.DYA[o], smu, cu, cv);
            dy = q * (a.RP[o] - (cu / (k - y) - cv / (k + y)) - hd);
            a.DY[o] = dy;
            du = (cu + u * dy) / (k - y);
            dv = (cv - v * dy) / (k + y);
        }
        ratio = fmin(ratio, hub_ratio(u, v, y, k, du, dv, dy));
    }
    a.part[(size_t)chunk * 4 * ld + bl] = ratio;
}
// the step length of a lane: the minimum over the chunks; the corrector stops DCHUBER_STEP_BACK of the way to the boundary
template <bool CORR>
__global__ __launch_bounds__(64) void k_hub_alpha(HubArgs a) {
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double ratio = HUGE_VAL;
    for (int c = 0; c < a.n_chunks; ++c) ratio = fmin(ratio, a.part[(size_t)c * 4 * ld + bl]);
    a.lres[(size_t)HR_ALPHA * ld + bl] = fmin(1.0, CORR ? DCHUBER_STEP_BACK * ratio : ratio);
}
// the chunk's share of the gap after the predictor's step
__global__ __launch_bounds__(256) void k_hub_gapaff(HubArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * DCHUBER_ROWS;
    if (i0 >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    const double al = a.lres[(size_t)HR_ALPHA * ld + bl];
    double g = 0.0;
    for (int i = i0; i < min(i0 + DCHUBER_ROWS, a.m); ++i) {
        if (!((CInt)a.st)[i]) continue;
        const size_t o = (size_t)i * ld + bl;
        const double k = ((CDbl)a.K)[i];
        const double u = a.U[o], v = a.V[o], y = a.Y[o], dy = a.DYA[o];
        double du, dv;
        hub_affine(u, v, y, k, dy, du, dv);
        g += (u + al * du) * (k - y - al * dy) + (v + al * dv) * (k + y + al * dy);
    }
    a.part[((size_t)chunk * 4 + 1) * ld + bl] = g;
}
// sigma mu = (affine gap / gap)^3 x gap / (2 x in-service rows)
__global__ __launch_bounds__(64) void k_hub_sigma(HubArgs a) {
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double g = 0.0;
    for (int c = 0; c < a.n_chunks; ++c) g += a.part[((size_t)c * 4 + 1) * ld + bl];
    const double gap = a.lres[(size_t)HR_GAP * ld + bl], s = g / gap;
    a.lres[(size_t)HR_SMU * ld + bl] = s * s * s * gap / (2.0 * (double)a.m_in);
}
// T = Q (rp - c) of the corrector
__global__ __launch_bounds__(256) void k_hub_corr_rows(HubArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups), o = (size_t)i * ld + bl;
    if (!((CInt)a.st)[i]) { a.T[o] = 0.0; return; }
    const double k = ((CDbl)a.K)[i];
    const double u = a.U[o], v = a.V[o], y = a.Y[o];
    double cu, cv;
    hub_targets(u, v, y, k, a.DYA[o], a.lres[(size_t)HR_SMU * ld + bl], cu, cv);
    a.T[o] = a.Q[o] * (a.RP[o] - (cu / (k - y) - cv / (k + y)));
}
// the step: rows (u, v, y), then states (theta).  A finished lane, and a lane whose factorisation met a bad pivot, is not written
__global__ __launch_bounds__(256) void k_hub_update_rows(HubArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m || !((CInt)a.st)[i]) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups), o = (size_t)i * ld + bl;
    if (a.done[bl] || a.bad[bl]) return;
    const double k = ((CDbl)a.K)[i];
    const double u = a.U[o], v = a.V[o], y = a.Y[o], dy = a.DY[o], al = a.lres[(size_t)HR_ALPHA * ld + bl];
    double cu, cv;
    hub_targets(u, v, y, k, a.DYA[o], a.lres[(size_t)HR_SMU * ld + bl], cu, cv);
    a.U[o] = u + al * ((cu + u * dy) / (k - y));
    a.V[o] = v + al * ((cv - v * dy) / (k + y));
    a.Y[o] = y + al * dy;
}
__global__ __launch_bounds__(256) void k_hub_update_states(HubArgs a) {
    const int j = blockIdx.x * 4 + uniform(threadIdx.y);
    if (j >= a.n) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups), o = (size_t)j * ld + bl;
    if (a.done[bl] || a.bad[bl]) return;
    a.TH[o] = fma(a.lres[(size_t)HR_ALPHA * ld + bl], a.DT[o], a.TH[o]);
}

// ---- the final pass, after the last verdict, every lane: per row the unscaled residual and the weight, per chunk the share of the Huber loss ------
__global__ __launch_bounds__(256) void k_hub_final(HubArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * DCHUBER_ROWS;
    if (i0 >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double loss = 0.0;
    for (int i = i0; i < min(i0 + DCHUBER_ROWS, a.m); ++i) {
        const size_t o = (size_t)i * ld + bl;
        if (!((CInt)a.st)[i]) { a.RES[o] = 0.0; a.WT[o] = 1.0; continue; }
        const double k = ((CDbl)a.K)[i];
        const double r = a.R[o], ar = fabs(r);
        a.RES[o] = r * ((CDbl)a.SG)[i];
        a.WT[o] = ar <= k ? 1.0 : k / ar;
        loss += ar <= k ? 0.5 * ar * ar : k * ar - 0.5 * k * k;
    }
    a.part[((size_t)chunk * 4 + 2) * ld + bl] = loss;
}
__global__ __launch_bounds__(64) void k_hub_final_finish(HubArgs a) {
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double loss = 0.0;
    for (int c = 0; c < a.n_chunks; ++c) loss += a.part[((size_t)c * 4 + 2) * ld + bl];
    a.lres[(size_t)HR_LOSS * ld + bl] = loss;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
HubArgs args_of(const DchuberHandle* h, const int* glist) {
    HubArgs a{};
    a.r_ptr = h->r_ptr; a.r_col = h->r_col; a.r_val = h->r_val; a.st = h->st; a.K = h->K; a.SG = h->SG; a.c_ptr = h->c_ptr; a.c_row = h->c_row; a.c_val = h->c_val;
    a.Z = h->Z; a.U = h->U; a.V = h->V; a.Y = h->Y; a.R = h->R; a.RP = h->RP; a.Q = h->Q; a.T = h->T; a.DYA = h->DYA; a.DY = h->DY; a.RES = h->RES; a.WT = h->WT;
    a.TH = h->TH; a.DT = h->DT; a.B = h->B; a.RD = h->RD; a.part = h->part; a.partc = h->partc; a.lres = h->lres;
    a.done = h->done; a.lstat = h->lstat; a.liter = h->liter; a.bad = h->fac.bad; a.gact = h->gact; a.groups = glist;
    a.m = h->m; a.n = h->n; a.ld = h->ld; a.n_chunks = h->n_chunks; a.n_cchunks = h->n_cchunks; a.m_in = h->m_in; a.batch = h->batch;
    return a;
}
inline dim3 by4(int items, int groups) { return dim3((items + 3) / 4, groups); }
#define HUB_LAUNCH(kernel, grid, block, ...) hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, __VA_ARGS__)

void launch_gain(DchuberHandle* h, int groups, const int* glist) {
    HubGainArgs g{h->g_ptr, h->g_row, h->g_prod, h->g_add, h->Q, h->fac.A, glist, h->nnz_gain, h->ld};
    HUB_LAUNCH(k_hub_gain, by4(h->nnz_gain, groups), dim3(64, 4), g);
}
void launch_factor(DchuberHandle* h, int groups, const int* glist) {
    lane_factor_numeric(h->fac, h->stream, groups, glist);
    h->factorisations++;
}
void launch_sweeps(DchuberHandle* h, double* out, int groups, const int* glist) { lane_sweep_pair(h->fac, h->stream, h->B, h->W, out, groups, glist); }
// the row pass and the column pass that feed the verdict and the predictor
void launch_residuals(DchuberHandle* h, const HubArgs& a, int groups) {
    HUB_LAUNCH(k_hub_row<false>, by4(h->n_chunks, groups), dim3(64, 4), a);
    HUB_LAUNCH(k_hub_col<true>, by4(h->n_cchunks, groups), dim3(64, 4), a);
}
// predictor, step length, sigma, corrector, step length: everything of an iteration between the factorisation and the update
void launch_steps(DchuberHandle* h, const HubArgs& a, int groups) {
    const dim3 rows = by4(h->n_chunks, groups), lanes = dim3(1, groups), wg(64, 4);
    launch_sweeps(h, h->DT, groups, a.groups);
    HUB_LAUNCH(k_hub_step<false>, rows, wg, a);
    HUB_LAUNCH(k_hub_alpha<false>, lanes, dim3(64), a);
    HUB_LAUNCH(k_hub_gapaff, rows, wg, a);
    HUB_LAUNCH(k_hub_sigma, lanes, dim3(64), a);
    HUB_LAUNCH(k_hub_corr_rows, by4(h->m, groups), wg, a);
    HUB_LAUNCH(k_hub_col<false>, by4(h->n_cchunks, groups), wg, a);
    launch_sweeps(h, h->DT, groups, a.groups);
    HUB_LAUNCH(k_hub_step<true>, rows, wg, a);
    HUB_LAUNCH(k_hub_alpha<true>, lanes, dim3(64), a);
}
void launch_update(DchuberHandle* h, const HubArgs& a, int groups) {
    HUB_LAUNCH(k_hub_update_rows, by4(h->m, groups), dim3(64, 4), a);
    HUB_LAUNCH(k_hub_update_states, by4(h->n, groups), dim3(64, 4), a);
}

// the start of every solve: observability from the factorisation with Q = 1, theta (the WLS estimate), then y, u, v by the start rule
int hub_start(DchuberHandle* h) {
    const size_t ld = (size_t)h->ld;
    const int ng = h->ld / 64;
    std::vector<int> done(ld, 0);
    for (size_t s = (size_t)h->batch; s < ld; ++s) done[s] = 1;           // the padding of the last group never runs
    DC_HIP(sync_copy(h->done, done.data(), ld * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DC_HIP(hipMemsetAsync(h->lstat, 0, ld * sizeof(int), h->stream));
    DC_HIP(hipMemsetAsync(h->liter, 0, ld * sizeof(int), h->stream));
    DC_HIP(hipMemsetAsync(h->RD, 0, (size_t)h->n * ld * sizeof(double), h->stream));
    const HubArgs a = args_of(h, nullptr);
    HUB_LAUNCH(k_hub_prep, by4(h->m, ng), dim3(64, 4), a);
    launch_gain(h, ng, nullptr);
    launch_factor(h, ng, nullptr);
    DC_HIP(hipGetLastError());
    std::vector<int> bad(ld);
    DC_HIP(sync_copy(bad.data(), h->fac.bad, ld * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    h->unobservable = h->m_in == 0;
    for (int s = 0; s < h->batch; ++s) h->unobservable = h->unobservable || bad[s];
    if (h->unobservable) return 0;
    HUB_LAUNCH(k_hub_col<false>, by4(h->n_cchunks, ng), dim3(64, 4), a);
    launch_sweeps(h, h->TH, ng, nullptr);
    HUB_LAUNCH(k_hub_row<true>, by4(h->n_chunks, ng), dim3(64, 4), a);
    HUB_LAUNCH(k_hub_start_finish, dim3(1, ng), dim3(64), a);
    HUB_LAUNCH(k_hub_init, by4(h->m, ng), dim3(64, 4), a);
    DC_HIP(hipGetLastError());
    return 0;
}

int hub_solve(DchuberHandle* h, int maxit, double tol) {
    DC_TRY(hub_start(h));
    h->last_iterations = 0;
    if (h->unobservable) return 0;
    const int ng = h->ld / 64;
    int groups = ng;
    for (int it = 0;; ++it) {
        // the lanes of the groups that still run: residuals, verdict, group list; the host reads how many groups go on
        HubArgs a = args_of(h, it ? h->glist : nullptr);
        launch_residuals(h, a, groups);
        HUB_LAUNCH(k_hub_verdict, dim3(ng), dim3(64), a, it, maxit, tol, h->hnorm * h->kmax);
        HUB_LAUNCH(k_hub_glist, dim3(1), dim3(1), h->gact, h->glist, h->d_count, ng);
        DC_HIP(hipGetLastError());
        DC_HIP(hipMemcpyAsync(h->p_count, h->d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(hipStreamSynchronize(h->stream));
        groups = *h->p_count;
        h->last_iterations = it;
        if (groups <= 0 || it >= maxit) break;
        a.groups = h->glist;
        launch_gain(h, groups, h->glist);
        launch_factor(h, groups, h->glist);
        launch_steps(h, a, groups);
        launch_update(h, a, groups);
    }
    const HubArgs a = args_of(h, nullptr);
    HUB_LAUNCH(k_hub_final, by4(h->n_chunks, ng), dim3(64, 4), a);
    HUB_LAUNCH(k_hub_final_finish, dim3(1, ng), dim3(64), a);
    DC_HIP(hipGetLastError());
    return 0;
}

std::string bytes_text(size_t b) {
    char t[64];
    snprintf(t, sizeof t, "%.1f MB", (double)b / 1048576.0);
    return t;
}

// status -> st, the in-service count, max_j sum_i |H_ij| and max kappa over the in-service rows; kappa -> K
int hub_apply_rows(DchuberHandle* h) {
    std::vector<double> colsum(h->n, 0.0);
    h->m_in = 0;
    h->kmax = 0.0;
    for (int i = 0; i < h->m; ++i) {
        if (!h->h_st[i]) continue;
        h->m_in++;
        h->kmax = std::max(h->kmax, h->h_kappa[i]);
        for (int p = h->h_rptr[i]; p < h->h_rptr[i + 1]; ++p) if (h->h_rcol[p] != h->slack) colsum[h->h_rcol[p]] += std::fabs(h->h_rval[p]);
    }
    h->hnorm = *std::max_element(colsum.begin(), colsum.end());
    DC_HIP(sync_copy(h->st, h->h_st.data(), (size_t)h->m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->K, h->h_kappa.data(), (size_t)h->m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h->solved = false;
    return 0;
}

bool bad_bounds(const double* kappa, int m) {
    for (int i = 0; i < m; ++i) if (!(kappa[i] > 0.0) || !std::isfinite(kappa[i])) return true;
    return false;
}

int dchuber_create(DchuberHandle* h, int64_t n64, int64_t m64, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, const double* kappa,
                   const double* sigma, int64_t slack1, double slack_angle, int64_t batch, int device) {
    const int n = (int)n64, m = (int)m64;
    h->n = n; h->m = m; h->batch = (int)batch; h->ld = (int)((batch + 63) / 64 * 64); h->device = device; h->slack = (int)slack1 - 1; h->slack_angle = slack_angle;
    if (rowptr[0] != 0) { h->error = "rowptr is not 0-based"; return 1; }
    const int64_t nnz = rowptr[m];
    if (nnz < 1 || nnz > (1 << 28)) { h->error = "the coefficient matrix is empty or too large"; return 1; }
    if (bad_bounds(kappa, m)) { h->error = "kappa: a bound is not positive and finite"; return 1; }
    std::vector<double> sg(m, 1.0);
    if (sigma)
        for (int i = 0; i < m; ++i) {
            if (!(sigma[i] > 0.0) || !std::isfinite(sigma[i])) { h->error = "sigma: a deviation is not positive and finite"; return 1; }
            sg[i] = sigma[i];
        }
    h->h_kappa.assign(kappa, kappa + m);
    h->h_rptr.resize(m + 1); h->h_rcol.resize(nnz); h->h_rval.assign(val, val + nnz); h->h_st.resize(m);
    for (int i = 0; i <= m; ++i) h->h_rptr[i] = (int)rowptr[i];
    for (int i = 0; i < m; ++i) {
        if (rowptr[i + 1] < rowptr[i] || rowptr[i + 1] > nnz) { h->error = "rowptr is not monotone"; return 1; }
        if (status[i] != 0 && status[i] != 1) { h->error = "status must be 0 or 1"; return 1; }
        h->h_st[i] = status[i];
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            if (col[p] < 1 || col[p] > n || (p > rowptr[i] && col[p] <= col[p - 1])) { h->error = "col: columns of a row must be ascending, unique and in 1..n"; return 1; }
            if (!std::isfinite(val[p])) { h->error = "val: a coefficient is not finite"; return 1; }
            h->h_rcol[p] = (int)col[p] - 1;
        }
    }
    const int slack = h->slack;
    // pattern of G: the union over ALL rows of H of their column pairs, plus the whole diagonal -- the pattern of jg_dcse and jg_dclav, so a row's status
    // changes values only and a state no in-service row touches is a zero pivot
    std::vector<std::vector<int>> adj(n);
    for (int j = 0; j < n; ++j) adj[j].push_back(j);
    for (int i = 0; i < m; ++i)
        for (int p = h->h_rptr[i]; p < h->h_rptr[i + 1]; ++p)
            for (int q = h->h_rptr[i]; q < h->h_rptr[i + 1]; ++q) adj[h->h_rcol[p]].push_back(h->h_rcol[q]);
    std::vector<int> rp(n + 1, 0), ci;
    for (int j = 0; j < n; ++j) {
        std::sort(adj[j].begin(), adj[j].end());
        adj[j].erase(std::unique(adj[j].begin(), adj[j].end()), adj[j].end());
        rp[j + 1] = rp[j] + (int)adj[j].size();
        ci.insert(ci.end(), adj[j].begin(), adj[j].end());
    }
    const int nnzg = rp[n];
    h->nnz_gain = nnzg;
    auto entry = [&](int r, int c) { return (int)(std::lower_bound(ci.begin() + rp[r], ci.begin() + rp[r + 1], c) - ci.begin()); };
    // per entry of G its (row of H, coefficient product) terms, rows ascending; the slack's row and column carry none (G[slack, slack] = 1)
    std::vector<int> g_ptr(nnzg + 1, 0), g_row;
    std::vector<double> g_prod;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int> fill(g_ptr.begin(), g_ptr.end() - 1);
        if (pass == 1) { g_row.assign(g_ptr[nnzg], 0); g_prod.assign(g_ptr[nnzg], 0.0); }
        for (int i = 0; i < m; ++i)
            for (int p = h->h_rptr[i]; p < h->h_rptr[i + 1]; ++p)
                for (int q = h->h_rptr[i]; q < h->h_rptr[i + 1]; ++q) {
                    const int r = h->h_rcol[p], c = h->h_rcol[q];
                    if (r == slack || c == slack) continue;
                    const int e = entry(r, c);
                    if (pass == 0) g_ptr[e + 1]++;
                    else { g_row[fill[e]] = i; g_prod[fill[e]++] = h->h_rval[p] * h->h_rval[q]; }
                }
        if (pass == 0) for (int e = 0; e < nnzg; ++e) g_ptr[e + 1] += g_ptr[e];
    }
    std::vector<double> g_add(nnzg, 0.0);
    g_add[entry(slack, slack)] = 1.0;
    // H' by state columns (rows ascending), the slack's list empty; H by rows with the slack's column zeroed
    std::vector<int> c_ptr(n + 1, 0);
    for (int64_t p = 0; p < nnz; ++p) if (h->h_rcol[p] != slack) c_ptr[h->h_rcol[p] + 1]++;
    for (int j = 0; j < n; ++j) c_ptr[j + 1] += c_ptr[j];
    std::vector<int> c_row(c_ptr[n]), cfill(c_ptr.begin(), c_ptr.end() - 1);
    std::vector<double> c_val(c_ptr[n]), r_val(h->h_rval);
    for (int i = 0; i < m; ++i)
        for (int p = h->h_rptr[i]; p < h->h_rptr[i + 1]; ++p) {
            const int j = h->h_rcol[p];
            if (j != slack) { c_row[cfill[j]] = i; c_val[cfill[j]++] = h->h_rval[p]; }
            else r_val[p] = 0.0;
        }
    BlockSymbolic S;
    if (analyze(n, rp.data(), ci.data(), DC_POLICY_NO_TOP, S) != 0) { h->error = "symbolic analysis of the gain pattern failed"; return 1; }
    // the footprint, before anything of it is allocated
    const size_t M = (size_t)m, N = (size_t)n, ld = (size_t)h->ld;
    h->n_chunks = (m + DCHUBER_ROWS - 1) / DCHUBER_ROWS;
    h->n_cchunks = (n + DCHUBER_COLS - 1) / DCHUBER_COLS;
    const size_t fac_b = lane_factor_bytes_per_lane(nnzg, S.n_entries, n);
    const size_t it_b = (12 * M + 5 * N + 1 + 4 * (size_t)h->n_chunks + (size_t)h->n_cchunks + 6) * sizeof(double) + 3 * sizeof(int);
    h->bytes_per_lane = fac_b + it_b;
    DC_HIP(hipSetDevice(device));
    size_t free_b = 0, total_b = 0;
    DC_HIP(hipMemGetInfo(&free_b, &total_b));
    if (h->bytes_per_lane * ld > free_b) {
        h->error = "jg_dchuber_create: " + std::to_string(ld) + " lanes need " + bytes_text(h->bytes_per_lane * ld) + " (" + bytes_text(fac_b * ld) + " of lane-valued factor, " +
                   bytes_text(it_b * ld) + " of iterates), " + bytes_text(free_b) + " are free: use a smaller batch";
        return 5;
    }
    DC_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    DC_TRY(dev_alloc(h, &h->g_ptr, g_ptr.size(), g_ptr.data()));
    DC_TRY(dev_alloc(h, &h->g_row, g_row.size(), g_row.data()));
    DC_TRY(dev_alloc(h, &h->g_prod, g_prod.size(), g_prod.data()));
    DC_TRY(dev_alloc(h, &h->g_add, g_add.size(), g_add.data()));
    DC_TRY(dev_alloc(h, &h->c_ptr, c_ptr.size(), c_ptr.data()));
    DC_TRY(dev_alloc(h, &h->c_row, c_row.size(), c_row.data()));
    DC_TRY(dev_alloc(h, &h->c_val, c_val.size(), c_val.data()));
    DC_TRY(dev_alloc(h, &h->r_ptr, h->h_rptr.size(), h->h_rptr.data()));
    DC_TRY(dev_alloc(h, &h->r_col, h->h_rcol.size(), h->h_rcol.data()));
    DC_TRY(dev_alloc(h, &h->r_val, r_val.size(), r_val.data()));
    DC_TRY(dev_alloc(h, &h->st, M, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->K, M, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->SG, M, sg.data()));
    DC_TRY(lane_factor_create(h, h->fac, n, nnzg, S, h->ld));
    for (double** p : {&h->Z, &h->U, &h->V, &h->Y, &h->R, &h->RP, &h->Q, &h->T, &h->DYA, &h->DY, &h->RES, &h->WT}) DC_TRY(dev_alloc(h, p, M * ld, (const double*)nullptr, true));
    for (double** p : {&h->TH, &h->DT, &h->B, &h->RD}) DC_TRY(dev_alloc(h, p, N * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->W, (N + 1) * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->part, (size_t)h->n_chunks * 4 * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->partc, (size_t)h->n_cchunks * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->lres, 6 * ld, (const double*)nullptr, true));
    for (int** p : {&h->done, &h->lstat, &h->liter}) DC_TRY(dev_alloc(h, p, ld, (const int*)nullptr, true));
    for (int** p : {&h->gact, &h->glist}) DC_TRY(dev_alloc(h, p, ld / 64, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->d_count, (size_t)1, (const int*)nullptr, true));
    DC_HIP(hipHostMalloc((void**)&h->p_count, sizeof(int), hipHostMallocDefault));
    *h->p_count = 0;
    DC_TRY(hub_apply_rows(h));
    return 0;
}

void dchuber_destroy(DchuberHandle* h) {
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void* p : h->allocs) hipFree(p);
    if (h->p_count) hipHostFree(h->p_count);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

// [count][rows] on the host -> lanes lane0 .. of [rows][ld] on the device
int upload_lanes(DchuberHandle* d, double* dev, size_t rows, const double* src, size_t lane0, size_t count) {
    std::vector<double> t(rows * count);
    for (size_t s = 0; s < count; ++s)
        for (size_t i = 0; i < rows; ++i) t[i * count + s] = src[s * rows + i];
    hipError_t e = hipMemcpy2DAsync(dev + lane0, (size_t)d->ld * sizeof(double), t.data(), count * sizeof(double), count * sizeof(double), rows, hipMemcpyHostToDevice, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) { d->error = std::string("host to device copy failed: ") + hipGetErrorString(e); return 2; }
    return 0;
}
// [rows][ld] on the device -> [batch][rows] on the host
int fetch_lanes(DchuberHandle* d, const double* dev, size_t rows, double* out, double add) {
    const size_t ld = (size_t)d->ld;
    std::vector<double> t(rows * ld);
    if (sync_copy(t.data(), dev, rows * ld * sizeof(double), hipMemcpyDeviceToHost, d->stream) != hipSuccess) { d->error = "device to host copy failed"; return 2; }
    for (size_t s = 0; s < (size_t)d->batch; ++s)
        for (size_t i = 0; i < rows; ++i) out[s * rows + i] = t[i * ld + s] + add;
    return 0;
}
// a per-(row, lane) result, NaN on an unobservable set
int fetch_rows(DchuberHandle* d, const double* dev, double* out) {
    if (d->unobservable) { std::fill(out, out + (size_t)d->batch * d->m, std::nan("")); return 0; }
    return fetch_lanes(d, dev, (size_t)d->m, out, 0.0);
}

}  // namespace
}  // namespace jg

using jg::DchuberHandle;
using jg::api_fail;

#define HUB_ENTER(h) DC_API_ENTER(jg::DchuberHandle, "null DC Huber state estimation handle", h)

extern "C" {

int jg_dchuber_create(int64_t* out, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, const double* kappa,
                      const double* sigma, int64_t slack, double slack_angle, int64_t batch, int device) {
    if (!out || !rowptr || !col || !val || !status || !kappa || n < 1 || n > (1 << 24) || m < 1 || m > (1 << 26) || slack < 1 || slack > n || batch < 1 || batch > (1 << 20))
        return api_fail(1, "jg_dchuber_create: bad argument");
    DchuberHandle* h = new DchuberHandle();
    const int rc = jg::dchuber_create(h, n, m, rowptr, col, val, status, kappa, sigma, slack, slack_angle, batch, device);
    if (rc) { const std::string msg = h->error; jg::dchuber_destroy(h); *out = 0; return api_fail(rc, msg); }
    *out = (int64_t)reinterpret_cast<intptr_t>(h);
    return 0;
}

void jg_dchuber_destroy(int64_t h) {
    if (h) jg::dchuber_destroy(reinterpret_cast<DchuberHandle*>(static_cast<intptr_t>(h)));
}

int jg_dchuber_dims(int64_t h, int64_t* dims) {
    HUB_ENTER(h);
    if (!dims) return api_fail(1, "jg_dchuber_dims: null pointer");
    const jg::DcFactor& Y = d->fac.sym;
    dims[0] = d->n; dims[1] = d->m; dims[2] = d->batch; dims[3] = d->ld; dims[4] = d->nnz_gain; dims[5] = Y.n_entries; dims[6] = Y.n_fact_levels;
    dims[7] = (int64_t)Y.fwd.h_lev.size() - 1; dims[8] = (int64_t)Y.bwd.h_lev.size() - 1; dims[9] = (int64_t)(Y.fwd.launches.size() + Y.bwd.launches.size());
    dims[10] = (int64_t)d->bytes_per_lane; dims[11] = d->m_in; dims[12] = d->factorisations; dims[13] = d->last_iterations;
    return 0;
}

int jg_dchuber_set_readings(int64_t h, int64_t lane0, int64_t count, const double* z) {
    HUB_ENTER(h);
    if (lane0 < 0 || count < 1 || lane0 + count > d->batch || !z) return api_fail(1, "jg_dchuber_set_readings: lanes out of range");
    for (size_t k = 0; k < (size_t)count * d->m; ++k) if (!std::isfinite(z[k])) return api_fail(1, "jg_dchuber_set_readings: a reading is not finite");
    DC_RET(jg::upload_lanes(d, d->Z, (size_t)d->m, z, (size_t)lane0, (size_t)count));
    d->have_z = true; d->solved = false;
    return 0;
}

int jg_dchuber_set_status(int64_t h, const int32_t* status) {
    HUB_ENTER(h);
    if (!status) return api_fail(1, "jg_dchuber_set_status: null pointer");
    for (int i = 0; i < d->m; ++i) if (status[i] != 0 && status[i] != 1) return api_fail(1, "jg_dchuber_set_status: status must be 0 or 1");
    for (int i = 0; i < d->m; ++i) d->h_st[i] = status[i];
    DC_RET(jg::hub_apply_rows(d));
    return 0;
}

int jg_dchuber_set_bounds(int64_t h, const double* kappa) {
    HUB_ENTER(h);
    if (!kappa) return api_fail(1, "jg_dchuber_set_bounds: null pointer");
    if (jg::bad_bounds(kappa, d->m)) return api_fail(1, "jg_dchuber_set_bounds: a bound is not positive and finite");
    d->h_kappa.assign(kappa, kappa + d->m);
    DC_RET(jg::hub_apply_rows(d));
    return 0;
}

int jg_dchuber_solve(int64_t h, int iteration, double tolerance) {
    HUB_ENTER(h);
    if (iteration < 0 || !(tolerance > 0.0)) return api_fail(1, "jg_dchuber_solve: iteration must not be negative, tolerance positive");
    if (!d->have_z) return api_fail(4, "jg_dchuber_solve: jg_dchuber_set_readings first");
    DC_RET(jg::hub_solve(d, iteration, tolerance));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    d->solved = true;
    return 0;
}

int jg_dchuber_get_angle(int64_t h, double* theta, int32_t* status, double* objective, int32_t* iterations) {
    HUB_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dchuber_get_angle: jg_dchuber_solve first");
    const size_t B = (size_t)d->batch, ld = (size_t)d->ld;
    const double nan = std::nan("");
    if (theta) {
        if (d->unobservable) std::fill(theta, theta + B * d->n, nan);
        else {
            DC_RET(jg::fetch_lanes(d, d->TH, (size_t)d->n, theta, d->slack_angle));
            for (size_t s = 0; s < B; ++s) theta[s * d->n + d->slack] = d->slack_angle;
        }
    }
    std::vector<int> t(ld);
    if (status) {
        if (!d->unobservable) DC_API_HIP(jg::sync_copy(t.data(), d->lstat, ld * sizeof(int), hipMemcpyDeviceToHost, d->stream));
        for (size_t s = 0; s < B; ++s) status[s] = d->unobservable ? 1 : t[s];
    }
    if (iterations) {
        if (!d->unobservable) DC_API_HIP(jg::sync_copy(t.data(), d->liter, ld * sizeof(int), hipMemcpyDeviceToHost, d->stream));
        for (size_t s = 0; s < B; ++s) iterations[s] = d->unobservable ? 0 : t[s];
    }
    if (objective) {
        if (d->unobservable) std::fill(objective, objective + B, nan);
        else DC_RET(jg::fetch_lanes(d, d->lres + (size_t)jg::HR_LOSS * ld, 1, objective, 0.0));
    }
    return 0;
}

int jg_dchuber_get_residual(int64_t h, double* r) {
    HUB_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dchuber_get_residual: jg_dchuber_solve first");
    if (!r) return api_fail(1, "jg_dchuber_get_residual: null pointer");
    DC_RET(jg::fetch_rows(d, d->RES, r));
    return 0;
}

int jg_dchuber_get_weight(int64_t h, double* w) {
    HUB_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dchuber_get_weight: jg_dchuber_solve first");
    if (!w) return api_fail(1, "jg_dchuber_get_weight: null pointer");
    DC_RET(jg::fetch_rows(d, d->WT, w));
    return 0;
}

int jg_dchuber_get_dual(int64_t h, double* y, double* gap) {
    HUB_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dchuber_get_dual: jg_dchuber_solve first");
    if (y) DC_RET(jg::fetch_rows(d, d->Y, y));
    if (gap) {
        if (d->unobservable) std::fill(gap, gap + d->batch, std::nan(""));
        else DC_RET(jg::fetch_lanes(d, d->lres + (size_t)jg::HR_GAP * d->ld, 1, gap, 0.0));
    }
    return 0;
}

int jg_dchuber_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, const double* shift) {
    HUB_ENTER(h);
    if (nbr < 1 || !from || !to || !admittance || !shift) return api_fail(1, "jg_dchuber_set_branches: bad argument");
    if (d->nbr) return api_fail(1, "jg_dchuber_set_branches: the branch table is already set");
    std::vector<int> f(nbr), t(nbr);
    for (int64_t k = 0; k < nbr; ++k) {
        if (from[k] < 1 || from[k] > d->n || to[k] < 1 || to[k] > d->n) return api_fail(1, "jg_dchuber_set_branches: bus index out of range");
        f[k] = (int)from[k] - 1; t[k] = (int)to[k] - 1;
    }
    d->n_fchunks = (int)((nbr + jg::DC_FLOW_BRANCHES - 1) / jg::DC_FLOW_BRANCHES);
    DC_RET(jg::dev_alloc(d, &d->b_from, (size_t)nbr, f.data()));
    DC_RET(jg::dev_alloc(d, &d->b_to, (size_t)nbr, t.data()));
    DC_RET(jg::dev_alloc(d, &d->b_y, (size_t)nbr, admittance));
    DC_RET(jg::dev_alloc(d, &d->b_shift, (size_t)nbr, shift));
    DC_RET(jg::dev_alloc(d, &d->fpart, (size_t)d->n_fchunks * 4 * d->ld, (const double*)nullptr, true));
    DC_RET(jg::dev_alloc(d, &d->flows, (size_t)nbr * d->ld, (const double*)nullptr, true));
    DC_RET(jg::dev_alloc(d, &d->o_none, (size_t)d->ld, (const int*)nullptr, false));
    DC_API_HIP(jg::sync_fill(d->o_none, 0xff, (size_t)d->ld * sizeof(int), d->stream));       // -1: no lane has an outage
    d->nbr = (int)nbr;
    return 0;
}

int jg_dchuber_get_flows(int64_t h, double* from) {
    HUB_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dchuber_get_flows: jg_dchuber_solve first");
    if (!d->nbr) return api_fail(1, "jg_dchuber_get_flows: jg_dchuber_set_branches first");
    if (!from) return api_fail(1, "jg_dchuber_get_flows: null pointer");
    if (d->unobservable) { std::fill(from, from + (size_t)d->batch * d->nbr, std::nan("")); return 0; }
    jg::DcFlowArgs f{};
    f.TH = d->TH; f.bf = d->b_from; f.bt = d->b_to; f.by = d->b_y; f.bs = d->b_shift; f.rating = nullptr; f.obr = d->o_none;
    f.flows = d->flows; f.part = d->fpart; f.nbr = d->nbr; f.ld = d->ld;
    jg::launch_dc_flows(f, false, dim3((d->n_fchunks + 3) / 4, d->ld / 64), d->stream);
    DC_API_HIP(hipGetLastError());
    DC_RET(jg::fetch_lanes(d, d->flows, (size_t)d->nbr, from, 0.0));
    return 0;
}

int jg_dchuber_time_kernel(int64_t h, int kernel, int reps, double* ms) {
    HUB_ENTER(h);
    if (!ms || reps < 1 || kernel < 0 || kernel > 4) return api_fail(1, "jg_dchuber_time_kernel: bad argument");
    if (!d->solved || d->unobservable) return api_fail(4, "jg_dchuber_time_kernel: jg_dchuber_solve first, on an observable set");
    const int ng = d->ld / 64;
    const jg::HubArgs a = jg::args_of(d, nullptr);
    // every lane of every group runs, finished or not; nothing of a lane's state is written (the update pass is left out), so the handle stays solved
    int rc = jg::time_events(d->stream, reps, ms, d->error, [&]() -> int {
        if (kernel == 0 || kernel == 4) jg::launch_residuals(d, a, ng);
        if (kernel == 0 || kernel == 1) jg::launch_gain(d, ng, nullptr);
        if (kernel == 0 || kernel == 2) jg::launch_factor(d, ng, nullptr);
        if (kernel == 0) jg::launch_steps(d, a, ng);
        if (kernel == 3) jg::launch_sweeps(d, d->DT, ng, nullptr);
        if (kernel == 4) {
            const dim3 rows = jg::by4(d->n_chunks, ng), wg(64, 4);
            hipLaunchKernelGGL(jg::k_hub_step<false>, rows, wg, 0, d->stream, a);
            hipLaunchKernelGGL(jg::k_hub_gapaff, rows, wg, 0, d->stream, a);
            hipLaunchKernelGGL(jg::k_hub_corr_rows, jg::by4(d->m, ng), wg, 0, d->stream, a);
            hipLaunchKernelGGL(jg::k_hub_col<false>, jg::by4(d->n_cchunks, ng), wg, 0, d->stream, a);
            hipLaunchKernelGGL(jg::k_hub_step<true>, rows, wg, 0, d->stream, a);
        }
        return 0;
    });
    return rc ? api_fail(rc, d->error) : 0;
}

}  // extern "C"
