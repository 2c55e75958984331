// jg_dclav.hip -- batched DC least-absolute-value state estimation (jg_dclav.hpp has the model, the method and the reference lines it stands for).  The
// lane-valued factorisation and sweeps are jg_dc_lanefactor.hip's; here: the gain assembly with a weight per lane, the row, column, step and update
// passes of the interior-point iteration, the verdict with the group list, the C ABI.  Coefficient values and indices are wave-uniform and go through
// scalar loads; every store is a vector store.
#include "jg_dclav.hpp"
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

// ---- gain assembly: G[e][lane] = sum over the entry's terms of (coefficient product) x Q[row][lane], + 1 on the slack's diagonal ------------------
struct LavGainArgs { const int* g_ptr; const int* g_row; const double* g_prod; const double* g_add; const double* Q; double* A; const int* groups; int nnz, ld; };
__global__ __launch_bounds__(256) void k_lav_gain(LavGainArgs a) {
    const int e = blockIdx.x * 4 + uniform(threadIdx.y);
    if (e >= a.nnz) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double s = ((CDbl)a.g_add)[e];
    for (int t = ((CInt)a.g_ptr)[e]; t < ((CInt)a.g_ptr)[e + 1]; ++t) s = fma(((CDbl)a.g_prod)[t], a.Q[(size_t)((CInt)a.g_row)[t] * ld + bl], s);
    a.A[(size_t)e * ld + bl] = s;
}

// ---- the passes over rows of H: DCLAV_ROWS rows per wavefront, lanes as lanes ------------------------------------------------------------------
struct LavArgs {
    const int* r_ptr; const int* r_col; const double* r_val; const int* st;
    const int* c_ptr; const int* c_row; const double* c_val;
    double* Z; double* U; double* V; double* Y; double* R; double* RP; double* Q; double* T; double* DYA; double* DY;
    double* TH; double* DT; double* B; double* RD;
    double* part; double* partc; double* lres;
    int* done; int* lstat; int* liter; const int* bad; int* gact;
    const int* groups;
    int m, n, ld, n_chunks, n_cchunks, m_in, batch;
};
constexpr int LR_OBJ = 0, LR_GAP = DCLAV_LRES_GAP, LR_ALPHA = 2, LR_SMU = 3, LR_START = 4;

__device__ __forceinline__ double lav_dot(const LavArgs& a, int i, const double* X, size_t ld, size_t bl) {
    double s = 0.0;
    for (int p = ((CInt)a.r_ptr)[i]; p < ((CInt)a.r_ptr)[i + 1]; ++p) s = fma(((CDbl)a.r_val)[p], X[(size_t)((CInt)a.r_col)[p] * ld + bl], s);
    return s;
}
// the predictor's du, dv from its dy (targets -u (1 - y), -v (1 + y))
__device__ __forceinline__ void lav_affine(double u, double v, double y, double dya, double& dua, double& dva) {
    dua = -u + u * dya / (1.0 - y);
    dva = -v - v * dya / (1.0 + y);
}
// the corrector's targets: sigma mu, minus the product, plus the second-order term of the predictor
__device__ __forceinline__ void lav_targets(double u, double v, double y, double dya, double smu, double& cu, double& cv) {
    double dua, dva;
    lav_affine(u, v, y, dya, dua, dva);
    cu = smu - u * (1.0 - y) + dua * dya;
    cv = smu - v * (1.0 + y) - dva * dya;
}
// the largest step that keeps u, v, 1 - y, 1 + y at or above 0
__device__ __forceinline__ double lav_ratio(double u, double v, double y, double du, double dv, double dy) {
    double r = HUGE_VAL;
    if (du < 0.0) r = fmin(r, -u / du);
    if (dv < 0.0) r = fmin(r, -v / dv);
    if (dy > 0.0) r = fmin(r, (1.0 - y) / dy);
    if (dy < 0.0) r = fmin(r, -(1.0 + y) / dy);
    return r;
}

// START: r0 = z - H theta and the partial of sum |r0|.  Otherwise r, rp, d, Q, T = Q r (the predictor's rp - c is r) and the partials of max |rp|,
// the gap, the objective and max |z|
template <bool START>
__global__ __launch_bounds__(256) void k_lav_row(LavArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * DCLAV_ROWS;
    if (i0 >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double pmax = 0.0, gap = 0.0, obj = 0.0, zmax = 0.0;
    for (int i = i0; i < min(i0 + DCLAV_ROWS, a.m); ++i) {
        const size_t o = (size_t)i * ld + bl;
        if (!((CInt)a.st)[i]) {
            a.R[o] = 0.0;
            if (!START) { a.RP[o] = 0.0; a.Q[o] = 0.0; a.T[o] = 0.0; }
            continue;
        }
        const double z = a.Z[o], r = z - lav_dot(a, i, a.TH, ld, bl);
        a.R[o] = r;
        obj += fabs(r);
        if (START) continue;
        const double u = a.U[o], v = a.V[o], y = a.Y[o];
        const double rp = r - u + v, q = 1.0 / (u / (1.0 - y) + v / (1.0 + y));
        a.RP[o] = rp; a.Q[o] = q; a.T[o] = q * r;
        pmax = fmax(pmax, fabs(rp));
        gap += u * (1.0 - y) + v * (1.0 + y);
        zmax = fmax(zmax, fabs(z));
    }
    double* p = a.part + (size_t)chunk * 4 * ld + bl;
    p[0] = pmax; p[ld] = gap; p[2 * ld] = obj; p[3 * ld] = zmax;
}
// the start: Q = status, T = status z (the right-hand side H'z of the unit-weight estimate)
__global__ __launch_bounds__(256) void k_lav_prep(LavArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m) return;
    const size_t o = (size_t)i * a.ld + lane_of(a.groups);
    const int s = ((CInt)a.st)[i];
    a.Q[o] = s ? 1.0 : 0.0;
    a.T[o] = s ? a.Z[o] : 0.0;
}
// s = max(mean |r0|, floor), chunks in ascending order
__global__ __launch_bounds__(64) void k_lav_start_finish(LavArgs a) {
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double obj = 0.0;
    for (int c = 0; c < a.n_chunks; ++c) obj += a.part[((size_t)c * 4 + 2) * ld + bl];
    a.lres[(size_t)LR_START * ld + bl] = fmax(obj / (double)a.m_in, DCLAV_START_FLOOR);
}
__global__ __launch_bounds__(256) void k_lav_init(LavArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups), o = (size_t)i * ld + bl;
    const int s = ((CInt)a.st)[i];
    const double r = a.R[o], e = a.lres[(size_t)LR_START * ld + bl];
    a.U[o] = s ? fmax(r, 0.0) + e : 0.0;
    a.V[o] = s ? fmax(-r, 0.0) + e : 0.0;
    a.Y[o] = 0.0;
}

// ---- the pass over columns of H (rows of H'): a gather, DCLAV_COLS states per wavefront ---------------------------------------------------------
// B = H'T - rd.  WITH_RD: rd = -H'y is formed here, stored, and its largest magnitude goes to partc; otherwise the stored rd is read
template <bool WITH_RD>
__global__ __launch_bounds__(256) void k_lav_col(LavArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int j0 = chunk * DCLAV_COLS;
    if (j0 >= a.n) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double dmax = 0.0;
    for (int j = j0; j < min(j0 + DCLAV_COLS, a.n); ++j) {
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
// one workgroup of 64 per lane group, ALL groups; chunks in ascending order
__global__ __launch_bounds__(64) void k_lav_verdict(LavArgs a, int it, int maxit, double tol, double hnorm) {
    const size_t ld = (size_t)a.ld, bl = (size_t)blockIdx.x * 64 + threadIdx.x;
    int active = 0;
    if (!a.done[bl]) {
        double pmax = 0.0, gap = 0.0, obj = 0.0, zmax = 0.0, dmax = 0.0;
        for (int c = 0; c < a.n_chunks; ++c) {
            const double* p = a.part + (size_t)c * 4 * ld + bl;
            pmax = fmax(pmax, p[0]); gap += p[ld]; obj += p[2 * ld]; zmax = fmax(zmax, p[3 * ld]);
        }
        for (int c = 0; c < a.n_cchunks; ++c) dmax = fmax(dmax, a.partc[(size_t)c * ld + bl]);
        a.lres[(size_t)LR_OBJ * ld + bl] = obj;
        a.lres[(size_t)LR_GAP * ld + bl] = gap;
        if (it > 0 && a.bad[bl]) { a.lstat[bl] = 3; a.liter[bl] = it - 1; a.done[bl] = 1; }        // the step of iteration it - 1 was not applied
        else if (pmax <= tol * (1.0 + zmax) && dmax <= tol * hnorm && gap <= tol * (1.0 + obj)) { a.lstat[bl] = 0; a.liter[bl] = it; a.done[bl] = 1; }
        else if (it >= maxit) { a.lstat[bl] = 5; a.liter[bl] = it; a.done[bl] = 1; }
        else active = 1;
    }
    const unsigned long long any = __ballot(active);
    if (threadIdx.x == 0) a.gact[blockIdx.x] = any != 0ull;
}
__global__ void k_lav_glist(const int* gact, int* glist, int* count, int groups) {
    if (blockIdx.x || threadIdx.x) return;
    int c = 0;
    for (int g = 0; g < groups; ++g)
        if (gact[g]) glist[c++] = g;
    *count = c;
}

// ---- steps ---------------------------------------------------------------------------------------------------------------------------------------
// dy = Q (rp - c - H dtheta), du, dv, and the chunk's ratio to the boundary.  CORR false: the predictor (c = -u + v, so rp - c = r); true: the corrector
template <bool CORR>
__global__ __launch_bounds__(256) void k_lav_step(LavArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * DCLAV_ROWS;
    if (i0 >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    const double smu = CORR ? a.lres[(size_t)LR_SMU * ld + bl] : 0.0;
    double ratio = HUGE_VAL;
    for (int i = i0; i < min(i0 + DCLAV_ROWS, a.m); ++i) {
        const size_t o = (size_t)i * ld + bl;
        if (!((CInt)a.st)[i]) { (CORR ? a.DY : a.DYA)[o] = 0.0; continue; }
        const double hd = lav_dot(a, i, a.DT, ld, bl);
        const double u = a.U[o], v = a.V[o], y = a.Y[o], q = a.Q[o];
        double dy, du, dv;
        if (!CORR) {
            dy = q * (a.R[o] - hd);
            a.DYA[o] = dy;
            lav_affine(u, v, y, dy, du, dv);
        } else {
            double cu, cv;
            lav_targets(u, v, y, a.DYA[o], smu, cu, cv);
            dy = q * (a.RP[o] - (cu / (1.0 - y) - cv / (1.0 + y)) - hd);
            a.DY[o] = dy;
            du = (cu + u * dy) / (1.0 - y);
            dv = (cv - v * dy) / (1.0 + y);
        }
        ratio = fmin(ratio, lav_ratio(u, v, y, du, dv, dy));
    }
    a.part[(size_t)chunk * 4 * ld + bl] = ratio;
}
// the step length of a lane: the minimum over the chunks; the corrector stops DCLAV_STEP_BACK of the way to the boundary
template <bool CORR>
__global__ __launch_bounds__(64) void k_lav_alpha(LavArgs a) {
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double ratio = HUGE_VAL;
    for (int c = 0; c < a.n_chunks; ++c) ratio = fmin(ratio, a.part[(size_t)c * 4 * ld + bl]);
    a.lres[(size_t)LR_ALPHA * ld + bl] = fmin(1.0, CORR ? DCLAV_STEP_BACK * ratio : ratio);
}
// the chunk's share of the gap after the predictor's step
__global__ __launch_bounds__(256) void k_lav_gapaff(LavArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * DCLAV_ROWS;
    if (i0 >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    const double al = a.lres[(size_t)LR_ALPHA * ld + bl];
    double g = 0.0;
    for (int i = i0; i < min(i0 + DCLAV_ROWS, a.m); ++i) {
        if (!((CInt)a.st)[i]) continue;
        const size_t o = (size_t)i * ld + bl;
        const double u = a.U[o], v = a.V[o], y = a.Y[o], dy = a.DYA[o];
        double du, dv;
        lav_affine(u, v, y, dy, du, dv);
        g += (u + al * du) * (1.0 - y - al * dy) + (v + al * dv) * (1.0 + y + al * dy);
    }
    a.part[((size_t)chunk * 4 + 1) * ld + bl] = g;
}
// sigma mu = (affine gap / gap)^3 x gap / (2 x in-service rows)
__global__ __launch_bounds__(64) void k_lav_sigma(LavArgs a) {
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    double g = 0.0;
    for (int c = 0; c < a.n_chunks; ++c) g += a.part[((size_t)c * 4 + 1) * ld + bl];
    const double gap = a.lres[(size_t)LR_GAP * ld + bl], s = g / gap;
    a.lres[(size_t)LR_SMU * ld + bl] = s * s * s * gap / (2.0 * (double)a.m_in);
}
// T = Q (rp - c) of the corrector
__global__ __launch_bounds__(256) void k_lav_corr_rows(LavArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups), o = (size_t)i * ld + bl;
    if (!((CInt)a.st)[i]) { a.T[o] = 0.0; return; }
    const double u = a.U[o], v = a.V[o], y = a.Y[o];
    double cu, cv;
    lav_targets(u, v, y, a.DYA[o], a.lres[(size_t)LR_SMU * ld + bl], cu, cv);
    a.T[o] = a.Q[o] * (a.RP[o] - (cu / (1.0 - y) - cv / (1.0 + y)));
}
// the step: rows (u, v, y), then states (theta).  A finished lane, and a lane whose factorisation met a bad pivot, is not written
__global__ __launch_bounds__(256) void k_lav_update_rows(LavArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m || !((CInt)a.st)[i]) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups), o = (size_t)i * ld + bl;
    if (a.done[bl] || a.bad[bl]) return;
    const double u = a.U[o], v = a.V[o], y = a.Y[o], dy = a.DY[o], al = a.lres[(size_t)LR_ALPHA * ld + bl];
    double cu, cv;
    lav_targets(u, v, y, a.DYA[o], a.lres[(size_t)LR_SMU * ld + bl], cu, cv);
    a.U[o] = u + al * ((cu + u * dy) / (1.0 - y));
    a.V[o] = v + al * ((cv - v * dy) / (1.0 + y));
    a.Y[o] = y + al * dy;
}
__global__ __launch_bounds__(256) void k_lav_update_states(LavArgs a) {
    const int j = blockIdx.x * 4 + uniform(threadIdx.y);
    if (j >= a.n) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups), o = (size_t)j * ld + bl;
    if (a.done[bl] || a.bad[bl]) return;
    a.TH[o] = fma(a.lres[(size_t)LR_ALPHA * ld + bl], a.DT[o], a.TH[o]);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
LavArgs args_of(const DclavHandle* h, const int* glist) {
    LavArgs a{};
    a.r_ptr = h->r_ptr; a.r_col = h->r_col; a.r_val = h->r_val; a.st = h->st; a.c_ptr = h->c_ptr; a.c_row = h->c_row; a.c_val = h->c_val;
    a.Z = h->Z; a.U = h->U; a.V = h->V; a.Y = h->Y; a.R = h->R; a.RP = h->RP; a.Q = h->Q; a.T = h->T; a.DYA = h->DYA; a.DY = h->DY;
    a.TH = h->TH; a.DT = h->DT; a.B = h->B; a.RD = h->RD; a.part = h->part; a.partc = h->partc; a.lres = h->lres;
    a.done = h->done; a.lstat = h->lstat; a.liter = h->liter; a.bad = h->fac.bad; a.gact = h->gact; a.groups = glist;
    a.m = h->m; a.n = h->n; a.ld = h->ld; a.n_chunks = h->n_chunks; a.n_cchunks = h->n_cchunks; a.m_in = h->m_in; a.batch = h->batch;
    return a;
}
inline dim3 by4(int items, int groups) { return dim3((items + 3) / 4, groups); }
#define LAV_LAUNCH(kernel, grid, block, ...) hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, __VA_ARGS__)

void launch_gain(DclavHandle* h, int groups, const int* glist) {
    LavGainArgs g{h->g_ptr, h->g_row, h->g_prod, h->g_add, h->Q, h->fac.A, glist, h->nnz_gain, h->ld};
    LAV_LAUNCH(k_lav_gain, by4(h->nnz_gain, groups), dim3(64, 4), g);
}
void launch_factor(DclavHandle* h, int groups, const int* glist) {
    lane_factor_numeric(h->fac, h->stream, groups, glist);
    h->factorisations++;
}
void launch_sweeps(DclavHandle* h, double* out, int groups, const int* glist) { lane_sweep_pair(h->fac, h->stream, h->B, h->W, out, groups, glist); }
// the row pass and the column pass that feed the verdict and the predictor
void launch_residuals(DclavHandle* h, const LavArgs& a, int groups) {
    LAV_LAUNCH(k_lav_row<false>, by4(h->n_chunks, groups), dim3(64, 4), a);
    LAV_LAUNCH(k_lav_col<true>, by4(h->n_cchunks, groups), dim3(64, 4), a);
}
// predictor, step length, sigma, corrector, step length: everything of an iteration between the factorisation and the update
void launch_steps(DclavHandle* h, const LavArgs& a, int groups) {
    const dim3 rows = by4(h->n_chunks, groups), lanes = dim3(1, groups), wg(64, 4);
    launch_sweeps(h, h->DT, groups, a.groups);
    LAV_LAUNCH(k_lav_step<false>, rows, wg, a);
    LAV_LAUNCH(k_lav_alpha<false>, lanes, dim3(64), a);
    LAV_LAUNCH(k_lav_gapaff, rows, wg, a);
    LAV_LAUNCH(k_lav_sigma, lanes, dim3(64), a);
    LAV_LAUNCH(k_lav_corr_rows, by4(h->m, groups), wg, a);
    LAV_LAUNCH(k_lav_col<false>, by4(h->n_cchunks, groups), wg, a);
    launch_sweeps(h, h->DT, groups, a.groups);
    LAV_LAUNCH(k_lav_step<true>, rows, wg, a);
    LAV_LAUNCH(k_lav_alpha<true>, lanes, dim3(64), a);
}
void launch_update(DclavHandle* h, const LavArgs& a, int groups) {
    LAV_LAUNCH(k_lav_update_rows, by4(h->m, groups), dim3(64, 4), a);
    LAV_LAUNCH(k_lav_update_states, by4(h->n, groups), dim3(64, 4), a);
}

// the start of every solve: observability from the factorisation with Q = 1, theta, then u, v, y by the start rule
int lav_start(DclavHandle* h) {
    const size_t ld = (size_t)h->ld;
    const int ng = h->ld / 64;
    std::vector<int> done(ld, 0);
    for (size_t s = (size_t)h->batch; s < ld; ++s) done[s] = 1;           // the padding of the last group never runs
    DC_HIP(sync_copy(h->done, done.data(), ld * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DC_HIP(hipMemsetAsync(h->lstat, 0, ld * sizeof(int), h->stream));
    DC_HIP(hipMemsetAsync(h->liter, 0, ld * sizeof(int), h->stream));
    DC_HIP(hipMemsetAsync(h->RD, 0, (size_t)h->n * ld * sizeof(double), h->stream));
    const LavArgs a = args_of(h, nullptr);
    LAV_LAUNCH(k_lav_prep, by4(h->m, ng), dim3(64, 4), a);
    launch_gain(h, ng, nullptr);
    launch_factor(h, ng, nullptr);
    DC_HIP(hipGetLastError());
    std::vector<int> bad(ld);
    DC_HIP(sync_copy(bad.data(), h->fac.bad, ld * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    h->unobservable = h->m_in == 0;
    for (int s = 0; s < h->batch; ++s) h->unobservable = h->unobservable || bad[s];
    if (h->unobservable) return 0;
    if (h->have_init) {
        std::vector<double> t((size_t)h->n * ld, 0.0);
        for (size_t s = 0; s < (size_t)h->batch; ++s)
            for (size_t j = 0; j < (size_t)h->n; ++j) t[j * ld + s] = (int)j == h->slack ? 0.0 : h->h_theta0[s * h->n + j] - h->slack_angle;
        DC_HIP(sync_copy(h->TH, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h->have_init = false;
    } else {
        LAV_LAUNCH(k_lav_col<false>, by4(h->n_cchunks, ng), dim3(64, 4), a);
        launch_sweeps(h, h->TH, ng, nullptr);
    }
    LAV_LAUNCH(k_lav_row<true>, by4(h->n_chunks, ng), dim3(64, 4), a);
    LAV_LAUNCH(k_lav_start_finish, dim3(1, ng), dim3(64), a);
    LAV_LAUNCH(k_lav_init, by4(h->m, ng), dim3(64, 4), a);
    DC_HIP(hipGetLastError());
    return 0;
}

int lav_solve(DclavHandle* h, int maxit, double tol) {
    DC_TRY(lav_start(h));
    h->last_iterations = 0;
    if (h->unobservable) return 0;
    const int ng = h->ld / 64;
    int groups = ng;
    for (int it = 0;; ++it) {
        // the lanes of the groups that still run: residuals, verdict, group list; the host reads how many groups go on
        LavArgs a = args_of(h, it ? h->glist : nullptr);
        launch_residuals(h, a, groups);
        LAV_LAUNCH(k_lav_verdict, dim3(ng), dim3(64), a, it, maxit, tol, h->hnorm);
        LAV_LAUNCH(k_lav_glist, dim3(1), dim3(1), h->gact, h->glist, h->d_count, ng);
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
    return 0;
}

std::string bytes_text(size_t b) {
    char t[64];
    snprintf(t, sizeof t, "%.1f MB", (double)b / 1048576.0);
    return t;
}

// status -> st, the in-service count and max_j sum_i |H_ij|
int lav_apply_status(DclavHandle* h) {
    std::vector<double> colsum(h->n, 0.0);
    h->m_in = 0;
    for (int i = 0; i < h->m; ++i) {
        if (!h->h_st[i]) continue;
        h->m_in++;
        for (int p = h->h_rptr[i]; p < h->h_rptr[i + 1]; ++p) if (h->h_rcol[p] != h->slack) colsum[h->h_rcol[p]] += std::fabs(h->h_rval[p]);
    }
    h->hnorm = *std::max_element(colsum.begin(), colsum.end());
    DC_HIP(sync_copy(h->st, h->h_st.data(), (size_t)h->m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    h->solved = false;
    return 0;
}

// slack1 = 0: no fixed state (jg_pmulav.hip) -- no g_add entry, no zeroed column, no offset; `who` names the entry point in the budget's text and
// `extra_b` is what that entry point holds per lane beside the iterates
int dclav_create(DclavHandle* h, int64_t n64, int64_t m64, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, int64_t slack1,
                 double slack_angle, int64_t batch, int device, const char* who = "jg_dclav_create", size_t extra_b = 0) {
    const int n = (int)n64, m = (int)m64;
    h->n = n; h->m = m; h->batch = (int)batch; h->ld = (int)((batch + 63) / 64 * 64); h->device = device; h->slack = (int)slack1 - 1; h->slack_angle = slack_angle;
    if (rowptr[0] != 0) { h->error = "rowptr is not 0-based"; return 1; }
    const int64_t nnz = rowptr[m];
    if (nnz < 1 || nnz > (1 << 28)) { h->error = "the coefficient matrix is empty or too large"; return 1; }
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
    // pattern of G: the union over ALL rows of H of their column pairs, plus the whole diagonal -- the pattern of jg_dcse, so a row's status changes
    // values only and a state no in-service row touches is a zero pivot
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
    if (slack >= 0) g_add[entry(slack, slack)] = 1.0;
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
    h->n_chunks = (m + DCLAV_ROWS - 1) / DCLAV_ROWS;
    h->n_cchunks = (n + DCLAV_COLS - 1) / DCLAV_COLS;
    const size_t fac_b = lane_factor_bytes_per_lane(nnzg, S.n_entries, n);
    const size_t it_b = (10 * M + 5 * N + 1 + 4 * (size_t)h->n_chunks + (size_t)h->n_cchunks + 6) * sizeof(double) + 3 * sizeof(int) + extra_b;
    h->bytes_per_lane = fac_b + it_b;
    DC_HIP(hipSetDevice(device));
    size_t free_b = 0, total_b = 0;
    DC_HIP(hipMemGetInfo(&free_b, &total_b));
    if (h->bytes_per_lane * ld > free_b) {
        h->error = std::string(who) + ": " + std::to_string(ld) + " lanes need " + bytes_text(h->bytes_per_lane * ld) + " (" + bytes_text(fac_b * ld) + " of lane-valued factor, " +
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
    DC_TRY(lane_factor_create(h, h->fac, n, nnzg, S, h->ld));
    for (double** p : {&h->Z, &h->U, &h->V, &h->Y, &h->R, &h->RP, &h->Q, &h->T, &h->DYA, &h->DY}) DC_TRY(dev_alloc(h, p, M * ld, (const double*)nullptr, true));
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
    DC_TRY(lav_apply_status(h));
    return 0;
}

void dclav_release(DclavHandle* h) {
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void* p : h->allocs) hipFree(p);
    if (h->p_count) hipHostFree(h->p_count);
    if (h->stream) hipStreamDestroy(h->stream);
}
void dclav_destroy(DclavHandle* h) {
    dclav_release(h);
    delete h;
}

// [count][rows] on the host -> lanes lane0 .. of [rows][ld] on the device
int upload_lanes(DclavHandle* d, double* dev, size_t rows, const double* src, size_t lane0, size_t count) {
    std::vector<double> t(rows * count);
    for (size_t s = 0; s < count; ++s)
        for (size_t i = 0; i < rows; ++i) t[i * count + s] = src[s * rows + i];
    hipError_t e = hipMemcpy2DAsync(dev + lane0, (size_t)d->ld * sizeof(double), t.data(), count * sizeof(double), count * sizeof(double), rows, hipMemcpyHostToDevice, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) { d->error = std::string("host to device copy failed: ") + hipGetErrorString(e); return 2; }
    return 0;
}
// [rows][ld] on the device -> [batch][rows] on the host
int fetch_lanes(DclavHandle* d, const double* dev, size_t rows, double* out, double add) {
    const size_t ld = (size_t)d->ld;
    std::vector<double> t(rows * ld);
    if (sync_copy(t.data(), dev, rows * ld * sizeof(double), hipMemcpyDeviceToHost, d->stream) != hipSuccess) { d->error = "device to host copy failed"; return 2; }
    for (size_t s = 0; s < (size_t)d->batch; ++s)
        for (size_t i = 0; i < rows; ++i) out[s * rows + i] = t[i * ld + s] + add;
    return 0;
}

// `reps` timings of part `kernel` (0 .. 4, jgrid.h: jg_dclav_time_kernel) of an iteration of a solved, observable handle
int lav_time_parts(DclavHandle* d, int kernel, int reps, double* ms) {
    const int ng = d->ld / 64;
    const LavArgs a = args_of(d, nullptr);
    // every lane of every group runs, finished or not; nothing of a lane's state is written (the update pass is left out), so the handle stays solved
    return time_events(d->stream, reps, ms, d->error, [&]() -> int {
        if (kernel == 0 || kernel == 4) launch_residuals(d, a, ng);
        if (kernel == 0 || kernel == 1) launch_gain(d, ng, nullptr);
        if (kernel == 0 || kernel == 2) launch_factor(d, ng, nullptr);
        if (kernel == 0) launch_steps(d, a, ng);
        if (kernel == 3) launch_sweeps(d, d->DT, ng, nullptr);
        if (kernel == 4) {
            const dim3 rows = by4(d->n_chunks, ng), wg(64, 4);
            hipLaunchKernelGGL(k_lav_step<false>, rows, wg, 0, d->stream, a);
            hipLaunchKernelGGL(k_lav_gapaff, rows, wg, 0, d->stream, a);
            hipLaunchKernelGGL(k_lav_corr_rows, by4(d->m, ng), wg, 0, d->stream, a);
            hipLaunchKernelGGL(k_lav_col<false>, by4(d->n_cchunks, ng), wg, 0, d->stream, a);
            hipLaunchKernelGGL(k_lav_step<true>, rows, wg, 0, d->stream, a);
        }
        return 0;
    });
}

}  // namespace

// what jg_pmulav.hip reaches the iteration through (jg_dclav.hpp)
int lav_create(DclavHandle* h, const char* who, size_t extra_b, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status,
               int64_t batch, int device) {
    return dclav_create(h, n, m, rowptr, col, val, status, 0, 0.0, batch, device, who, extra_b);
}
void lav_release(DclavHandle* h) { dclav_release(h); }
int lav_set_status(DclavHandle* h) { return lav_apply_status(h); }
int lav_run(DclavHandle* h, int maxit, double tol) { return lav_solve(h, maxit, tol); }
int lav_time(DclavHandle* h, int kernel, int reps, double* ms) { return lav_time_parts(h, kernel, reps, ms); }
int lav_upload(DclavHandle* h, double* dev, size_t rows, const double* src, size_t lane0, size_t count) { return upload_lanes(h, dev, rows, src, lane0, count); }
int lav_fetch(DclavHandle* h, const double* dev, size_t rows, double* out) { return fetch_lanes(h, dev, rows, out, 0.0); }

}  // namespace jg

using jg::DclavHandle;
using jg::api_fail;

#define LAV_ENTER(h) DC_API_ENTER(jg::DclavHandle, "null DC LAV state estimation handle", h)

extern "C" {

int jg_dclav_create(int64_t* out, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, int64_t slack,
                    double slack_angle, int64_t batch, int device) {
    if (!out || !rowptr || !col || !val || !status || n < 1 || n > (1 << 24) || m < 1 || m > (1 << 26) || slack < 1 || slack > n || batch < 1 || batch > (1 << 20))
        return api_fail(1, "jg_dclav_create: bad argument");
    DclavHandle* h = new DclavHandle();
    const int rc = jg::dclav_create(h, n, m, rowptr, col, val, status, slack, slack_angle, batch, device);
    if (rc) { const std::string msg = h->error; jg::dclav_destroy(h); *out = 0; return api_fail(rc, msg); }
    *out = (int64_t)reinterpret_cast<intptr_t>(h);
    return 0;
}

void jg_dclav_destroy(int64_t h) {
    if (h) jg::dclav_destroy(reinterpret_cast<DclavHandle*>(static_cast<intptr_t>(h)));
}

int jg_dclav_dims(int64_t h, int64_t* dims) {
    LAV_ENTER(h);
    if (!dims) return api_fail(1, "jg_dclav_dims: null pointer");
    const jg::DcFactor& Y = d->fac.sym;
    dims[0] = d->n; dims[1] = d->m; dims[2] = d->batch; dims[3] = d->ld; dims[4] = d->nnz_gain; dims[5] = Y.n_entries; dims[6] = Y.n_fact_levels;
    dims[7] = (int64_t)Y.fwd.h_lev.size() - 1; dims[8] = (int64_t)Y.bwd.h_lev.size() - 1; dims[9] = (int64_t)(Y.fwd.launches.size() + Y.bwd.launches.size());
    dims[10] = (int64_t)d->bytes_per_lane; dims[11] = d->m_in; dims[12] = d->factorisations; dims[13] = d->last_iterations;
    return 0;
}

int jg_dclav_set_readings(int64_t h, int64_t lane0, int64_t count, const double* z) {
    LAV_ENTER(h);
    if (lane0 < 0 || count < 1 || lane0 + count > d->batch || !z) return api_fail(1, "jg_dclav_set_readings: lanes out of range");
    for (size_t k = 0; k < (size_t)count * d->m; ++k) if (!std::isfinite(z[k])) return api_fail(1, "jg_dclav_set_readings: a reading is not finite");
    DC_RET(jg::upload_lanes(d, d->Z, (size_t)d->m, z, (size_t)lane0, (size_t)count));
    d->have_z = true; d->solved = false;
    return 0;
}

int jg_dclav_set_status(int64_t h, const int32_t* status) {
    LAV_ENTER(h);
    if (!status) return api_fail(1, "jg_dclav_set_status: null pointer");
    for (int i = 0; i < d->m; ++i) if (status[i] != 0 && status[i] != 1) return api_fail(1, "jg_dclav_set_status: status must be 0 or 1");
    for (int i = 0; i < d->m; ++i) d->h_st[i] = status[i];
    DC_RET(jg::lav_apply_status(d));
    return 0;
}

int jg_dclav_set_initial(int64_t h, const double* theta) {
    LAV_ENTER(h);
    if (!theta) return api_fail(1, "jg_dclav_set_initial: null pointer");
    for (size_t k = 0; k < (size_t)d->batch * d->n; ++k) if (!std::isfinite(theta[k])) return api_fail(1, "jg_dclav_set_initial: an angle is not finite");
    d->h_theta0.assign(theta, theta + (size_t)d->batch * d->n);
    d->have_init = true; d->solved = false;
    return 0;
}

int jg_dclav_solve(int64_t h, int iteration, double tolerance) {
    LAV_ENTER(h);
    if (iteration < 0 || !(tolerance > 0.0)) return api_fail(1, "jg_dclav_solve: iteration must not be negative, tolerance positive");
    if (!d->have_z) return api_fail(4, "jg_dclav_solve: jg_dclav_set_readings first");
    DC_RET(jg::lav_solve(d, iteration, tolerance));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    d->solved = true;
    return 0;
}

int jg_dclav_get_angle(int64_t h, double* theta, int32_t* status, double* objective, int32_t* iterations) {
    LAV_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dclav_get_angle: jg_dclav_solve first");
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
        else DC_RET(jg::fetch_lanes(d, d->lres, 1, objective, 0.0));
    }
    return 0;
}

int jg_dclav_get_residual(int64_t h, double* r) {
    LAV_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dclav_get_residual: jg_dclav_solve first");
    if (!r) return api_fail(1, "jg_dclav_get_residual: null pointer");
    if (d->unobservable) { std::fill(r, r + (size_t)d->batch * d->m, std::nan("")); return 0; }
    DC_RET(jg::fetch_lanes(d, d->R, (size_t)d->m, r, 0.0));
    return 0;
}

int jg_dclav_get_dual(int64_t h, double* y, double* gap) {
    LAV_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dclav_get_dual: jg_dclav_solve first");
    if (d->unobservable) {
        if (y) std::fill(y, y + (size_t)d->batch * d->m, std::nan(""));
        if (gap) std::fill(gap, gap + d->batch, std::nan(""));
        return 0;
    }
    if (y) DC_RET(jg::fetch_lanes(d, d->Y, (size_t)d->m, y, 0.0));
    if (gap) DC_RET(jg::fetch_lanes(d, d->lres + (size_t)jg::LR_GAP * d->ld, 1, gap, 0.0));
    return 0;
}

int jg_dclav_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, const double* shift) {
    LAV_ENTER(h);
    if (nbr < 1 || !from || !to || !admittance || !shift) return api_fail(1, "jg_dclav_set_branches: bad argument");
    if (d->nbr) return api_fail(1, "jg_dclav_set_branches: the branch table is already set");
    std::vector<int> f(nbr), t(nbr);
    for (int64_t k = 0; k < nbr; ++k) {
        if (from[k] < 1 || from[k] > d->n || to[k] < 1 || to[k] > d->n) return api_fail(1, "jg_dclav_set_branches: bus index out of range");
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

int jg_dclav_get_flows(int64_t h, double* from) {
    LAV_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dclav_get_flows: jg_dclav_solve first");
    if (!d->nbr) return api_fail(1, "jg_dclav_get_flows: jg_dclav_set_branches first");
    if (!from) return api_fail(1, "jg_dclav_get_flows: null pointer");
    if (d->unobservable) { std::fill(from, from + (size_t)d->batch * d->nbr, std::nan("")); return 0; }
    jg::DcFlowArgs f{};
    f.TH = d->TH; f.bf = d->b_from; f.bt = d->b_to; f.by = d->b_y; f.bs = d->b_shift; f.rating = nullptr; f.obr = d->o_none;
    f.flows = d->flows; f.part = d->fpart; f.nbr = d->nbr; f.ld = d->ld;
    jg::launch_dc_flows(f, false, dim3((d->n_fchunks + 3) / 4, d->ld / 64), d->stream);
    DC_API_HIP(hipGetLastError());
    DC_RET(jg::fetch_lanes(d, d->flows, (size_t)d->nbr, from, 0.0));
    return 0;
}

int jg_dclav_factor_solve(int64_t h, const double* q, const double* rhs, double* x, int32_t* bad) {
    LAV_ENTER(h);
    if (!q || !rhs || !x || !bad) return api_fail(1, "jg_dclav_factor_solve: null pointer");
    const size_t B = (size_t)d->batch, ld = (size_t)d->ld;
    const int ng = d->ld / 64;
    DC_RET(jg::upload_lanes(d, d->Q, (size_t)d->m, q, 0, B));
    DC_RET(jg::upload_lanes(d, d->B, (size_t)d->n, rhs, 0, B));
    jg::launch_gain(d, ng, nullptr);
    jg::launch_factor(d, ng, nullptr);
    jg::launch_sweeps(d, d->DT, ng, nullptr);
    DC_API_HIP(hipGetLastError());
    DC_RET(jg::fetch_lanes(d, d->DT, (size_t)d->n, x, 0.0));
    std::vector<int> t(ld);
    DC_API_HIP(jg::sync_copy(t.data(), d->fac.bad, ld * sizeof(int), hipMemcpyDeviceToHost, d->stream));
    for (size_t s = 0; s < B; ++s) bad[s] = t[s];
    d->solved = false;
    return 0;
}

int jg_dclav_time_kernel(int64_t h, int kernel, int reps, double* ms) {
    LAV_ENTER(h);
    if (!ms || reps < 1 || kernel < 0 || kernel > 4) return api_fail(1, "jg_dclav_time_kernel: bad argument");
    if (!d->solved || d->unobservable) return api_fail(4, "jg_dclav_time_kernel: jg_dclav_solve first, on an observable set");
    const int rc = jg::lav_time(d, kernel, reps, ms);
    return rc ? api_fail(rc, d->error) : 0;
}

}  // extern "C"
