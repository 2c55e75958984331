// jg_dcopf.hip -- batched DC optimal power flow by ADMM on one shared factor (jg_dcopf.hpp has the iteration and the reference lines it stands for).
// The factorisation and the sweeps are jg_dc_sweep.hip's, on the pattern of K = P + sigma I + A' diag(rho) A; here: the host set-up (scaling, pattern and
// term lists of K), the assembly of K, the right-hand side, the projection step, the residual pass and the verdict, the run loop, the C ABI.
// Row ids, coefficient values and rho are wave-uniform and go through scalar loads; a wavefront owns one row or variable x 64 lanes, so nothing is
// accumulated across waves: no atomics, every store is a vector store.
#include "jg_dcopf.hpp"
#include "jg_dc_abi.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/jgrid.h"
#include "jg_engine.hpp"

namespace jg {

namespace {

// ---- host set-up: the scaled problem, the pattern of K and the terms of its entries ----------------------------------------------------------
struct OpfModel {
    int n = 0, m = 0;
    double cscale = 1.0, q_norm = 0.0;
    std::vector<double> P, q, E, rval;                 // scaled: c P, c q, 1 / |a_i|, E A
    std::vector<int> rptr, rcol, eq;
    std::vector<int> kp, kc;                            // pattern of K, row-CSR
    std::vector<int> g_ptr, g_row; std::vector<double> g_prod, g_add, g_dg;
};

int opf_model(OpfModel& M, std::string& error, int64_t n64, int64_t m64, const int64_t* rowptr, const int64_t* col, const double* val, const double* P,
              const double* q, const int32_t* eq) {
    const int n = (int)n64, m = (int)m64;
    M.n = n; M.m = m;
    if (rowptr[0] != 0) { error = "rowptr is not 0-based"; return 1; }
    const int64_t nnz = rowptr[m];
    if (nnz < 1 || nnz > (1 << 28)) { error = "the constraint matrix is empty or too large"; return 1; }
    double big = 0.0;
    for (int j = 0; j < n; ++j) {
        if (!(P[j] >= 0.0) || !std::isfinite(P[j]) || !std::isfinite(q[j])) { error = "P must be non-negative and finite, q finite"; return 1; }
        big = std::max(big, std::max(P[j], std::fabs(q[j])));
    }
    M.cscale = big > 0.0 ? 1.0 / big : 1.0;
    M.P.resize(n); M.q.resize(n);
    for (int j = 0; j < n; ++j) { M.P[j] = M.cscale * P[j]; M.q[j] = M.cscale * q[j]; M.q_norm = std::max(M.q_norm, std::fabs(M.q[j])); }
    M.rptr.resize(m + 1); M.rcol.resize(nnz); M.rval.resize(nnz); M.E.resize(m); M.eq.resize(m);
    for (int i = 0; i <= m; ++i) M.rptr[i] = (int)rowptr[i];
    for (int i = 0; i < m; ++i) {
        if (rowptr[i + 1] <= rowptr[i] || rowptr[i + 1] > nnz) { error = "rowptr is not monotone or a row is empty"; return 1; }
        if (eq[i] != 0 && eq[i] != 1) { error = "a row class must be 0 (inequality) or 1 (equality)"; return 1; }
        M.eq[i] = eq[i];
        double s = 0.0;
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            if (col[p] < 1 || col[p] > n || (p > rowptr[i] && col[p] <= col[p - 1])) { error = "col: columns of a row must be ascending, unique and in 1..n"; return 1; }
            if (!std::isfinite(val[p])) { error = "a coefficient is not finite"; return 1; }
            M.rcol[p] = (int)col[p] - 1;
            s += val[p] * val[p];
        }
        if (!(s > 0.0)) { error = "a row of the constraint matrix is zero"; return 1; }
        M.E[i] = 1.0 / std::sqrt(s);
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) M.rval[p] = M.E[i] * val[p];
    }
    // pattern of K: the union over rows of A of all column pairs, plus the whole diagonal
    std::vector<std::vector<int>> adj(n);
    for (int j = 0; j < n; ++j) adj[j].push_back(j);
    for (int i = 0; i < m; ++i)
        for (int p = M.rptr[i]; p < M.rptr[i + 1]; ++p)
            for (int r = M.rptr[i]; r < M.rptr[i + 1]; ++r) adj[M.rcol[p]].push_back(M.rcol[r]);
    M.kp.assign(n + 1, 0);
    for (int j = 0; j < n; ++j) {
        std::sort(adj[j].begin(), adj[j].end());
        adj[j].erase(std::unique(adj[j].begin(), adj[j].end()), adj[j].end());
        M.kp[j + 1] = M.kp[j] + (int)adj[j].size();
        M.kc.insert(M.kc.end(), adj[j].begin(), adj[j].end());
    }
    const int nnzk = M.kp[n];
    auto entry = [&](int r, int c) { return (int)(std::lower_bound(M.kc.begin() + M.kp[r], M.kc.begin() + M.kp[r + 1], c) - M.kc.begin()); };
    // per entry of K its (row of A, coefficient product) terms, rows ascending
    M.g_ptr.assign(nnzk + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int> fill(M.g_ptr.begin(), M.g_ptr.end() - 1);
        if (pass == 1) { M.g_row.assign(M.g_ptr[nnzk], 0); M.g_prod.assign(M.g_ptr[nnzk], 0.0); }
        for (int i = 0; i < m; ++i)
            for (int p = M.rptr[i]; p < M.rptr[i + 1]; ++p)
                for (int r = M.rptr[i]; r < M.rptr[i + 1]; ++r) {
                    const int e = entry(M.rcol[p], M.rcol[r]);
                    if (pass == 0) M.g_ptr[e + 1]++;
                    else { M.g_row[fill[e]] = i; M.g_prod[fill[e]++] = M.rval[p] * M.rval[r]; }
                }
        if (pass == 0) for (int e = 0; e < nnzk; ++e) M.g_ptr[e + 1] += M.g_ptr[e];
    }
    M.g_add.assign(nnzk, 0.0); M.g_dg.assign(nnzk, 0.0);
    for (int j = 0; j < n; ++j) { const int e = entry(j, j); M.g_add[e] = M.P[j]; M.g_dg[e] = 1.0; }
    return 0;
}
void rho_rows(const std::vector<int>& eq, double rho, std::vector<double>& rhov, std::vector<double>& rinv) {
    rhov.resize(eq.size()); rinv.resize(eq.size());
    for (size_t i = 0; i < eq.size(); ++i) { rhov[i] = eq[i] ? OPF_RHO_EQ * rho : rho; rinv[i] = 1.0 / rhov[i]; }
}

// ---- K entries from their term lists: P + sigma on the diagonal, products of A values x rho of the row ---------------------------------------------
__host__ __device__ inline double gain_entry(const int* g_ptr, const int* g_row, const double* g_prod, const double* g_add, const double* g_dg,
                                             const double* rhov, double sigma, int e) {
    double s = g_add[e] + sigma * g_dg[e];
    for (int t = g_ptr[e]; t < g_ptr[e + 1]; ++t) s = fma(g_prod[t], rhov[g_row[t]], s);
    return s;
}
__global__ void k_opf_gain(const int* g_ptr, const int* g_row, const double* g_prod, const double* g_add, const double* g_dg, const double* rhov,
                           double sigma, double* A, int nnz) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) A[e] = gain_entry(g_ptr, g_row, g_prod, g_add, g_dg, rhov, sigma, e);
}

// ---- the lanes' branch outages: A_s = A + p d'.  The kernels below have a second instance (OUT) that a handle launches only while it holds an outage;
// in it a lane adds the term of p d' where the wavefront's row is r_f or r_t, or its variable f or t.  These indices are the lane's own, not
// wave-uniform: vector loads.  A lane without an outage carries -1 and takes no branch, so its arithmetic is the first instance's
struct OpfOut { const int* var; const int* row; const double* p; };     // [2][ld] each
// p' v on the lane's two balance rows, v [m][ld]
__device__ __forceinline__ double opf_out_rows(const OpfOut& o, const double* v, size_t ld, size_t bl, int rf, int rt) {
    return fma(o.p[bl], v[(size_t)rf * ld + bl], o.p[ld + bl] * v[(size_t)rt * ld + bl]);
}

// ---- b = sigma x - q + A' (rho o z - y): a wavefront = one variable x 64 lanes; `blend` first takes x+ = alpha x~ + (1 - alpha) x of the step before
struct OpfRhsArgs {
    const int* c_ptr; const int* c_row; const double* c_val; const double* rhov; const double* q; const double* Z; const double* Y; const double* XT;
    double* X; double* B; const int* done; const int* groups;
    double sigma, alpha; int n, ld, blend, form;
    OpfOut out;
};
template <bool OUT>
__global__ __launch_bounds__(256) void k_opf_rhs(OpfRhsArgs a) {
    const int j = blockIdx.x * 4 + uniform(threadIdx.y);
    if (j >= a.n) return;
    const int grp = ((CInt)a.groups)[blockIdx.y];
    const size_t ld = (size_t)a.ld, bl = (size_t)grp * 64 + threadIdx.x, at = (size_t)j * ld + bl;
    double x = a.X[at];
    if (a.blend) {
        x = fma(a.alpha, a.XT[at], (1.0 - a.alpha) * x);
        if (!a.done[bl]) a.X[at] = x;                                   // a finished lane is frozen
    }
    if (!a.form) return;
    double acc = fma(a.sigma, x, -((CDbl)a.q)[j]);
    for (int p = ((CInt)a.c_ptr)[j]; p < ((CInt)a.c_ptr)[j + 1]; ++p) {
        const int i = ((CInt)a.c_row)[p];
        const size_t r = (size_t)i * ld + bl;
        acc = fma(((CDbl)a.c_val)[p], fma(((CDbl)a.rhov)[i], a.Z[r], -a.Y[r]), acc);
    }
    if (OUT) {                                                          // + d_j p' (rho o z - y)
        const int f = a.out.var[bl], t = a.out.var[ld + bl];
        if (j == f || j == t) {
            const int rf = a.out.row[bl], rt = a.out.row[ld + bl];
            const size_t qf = (size_t)rf * ld + bl, qt = (size_t)rt * ld + bl;
            const double w = fma(a.out.p[bl], fma(a.rhov[rf], a.Z[qf], -a.Y[qf]), a.out.p[ld + bl] * fma(a.rhov[rt], a.Z[qt], -a.Y[qt]));
            acc += j == f ? w : -w;
        }
    }
    a.B[at] = acc;
}

// ---- z~ = a_i x~, relaxation, projection on [l, u], multiplier step: a wavefront = one row of A x 64 lanes -------------------------------------------
struct OpfUpdateArgs {
    const int* r_ptr; const int* r_col; const double* r_val; const double* rhov; const double* rinv; const double* XT; const double* L; const double* U;
    double* Z; double* Y; double* DY; const int* done; const int* groups;
    double alpha; int m, ld, keep_dy;
    OpfOut out;
};
template <bool OUT>
__global__ __launch_bounds__(256) void k_opf_update(OpfUpdateArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.m) return;
    const int grp = ((CInt)a.groups)[blockIdx.y];
    const size_t ld = (size_t)a.ld, bl = (size_t)grp * 64 + threadIdx.x, at = (size_t)i * ld + bl;
    double zt = 0.0;
    for (int p = ((CInt)a.r_ptr)[i]; p < ((CInt)a.r_ptr)[i + 1]; ++p) zt = fma(((CDbl)a.r_val)[p], a.XT[(size_t)((CInt)a.r_col)[p] * ld + bl], zt);
    if (OUT) {                                                          // + p_i (x~_f - x~_t)
        const int rf = a.out.row[bl], rt = a.out.row[ld + bl];
        if (i == rf || i == rt) {
            const double dx = a.XT[(size_t)a.out.var[bl] * ld + bl] - a.XT[(size_t)a.out.var[ld + bl] * ld + bl];
            zt = fma(a.out.p[(i == rf ? 0 : ld) + bl], dx, zt);
        }
    }
    const double rho = ((CDbl)a.rhov)[i], ri = ((CDbl)a.rinv)[i];
    const double z = a.Z[at], y = a.Y[at];
    const double zr = fma(a.alpha, zt, (1.0 - a.alpha) * z);
    const double zn = fmin(fmax(fma(y, ri, zr), a.L[at]), a.U[at]);
    const double yn = fma(rho, zr - zn, y);
    if (a.done[bl]) return;                                             // frozen
    a.Z[at] = zn; a.Y[at] = yn;
    if (a.keep_dy) a.DY[at] = yn - y;
}

// ---- residual pass: OPF_CHUNK rows (ROWS) or variables per wavefront, partial maxima per lane -------------------------------------------------------
// dy of the certificate: a component that pushes against a bound that is none is left out (OSQP's projection of delta y)
__device__ __forceinline__ double opf_dy(double dy, double l, double u) {
    if (u >= OPF_INF) dy = fmin(dy, 0.0);
    if (l <= -OPF_INF) dy = fmax(dy, 0.0);
    return dy;
}
struct OpfResArgs {
    const int* ptr; const int* idx; const double* val;          // ROWS: A by rows; else A by columns
    const double* P; const double* q; const double* X; const double* Z; const double* Y; const double* DY; const double* L; const double* U;
    double* part; const int* groups; int count, ld;
    OpfOut out;
};
template <bool ROWS, bool OUT>
__global__ __launch_bounds__(256) void k_opf_residual(OpfResArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int k0 = chunk * OPF_CHUNK;
    if (k0 >= a.count) return;
    const int grp = ((CInt)a.groups)[blockIdx.y];
    const size_t ld = (size_t)a.ld, bl = (size_t)grp * 64 + threadIdx.x;
    int of = -1, ot = -1, orf = -1, ort = -1;
    double ow0 = 0.0, ow1 = 0.0;                                         // ROWS: x_f - x_t; else p' y and p' dy on the lane's two balance rows
    if (OUT) {
        of = a.out.var[bl]; ot = a.out.var[ld + bl]; orf = a.out.row[bl]; ort = a.out.row[ld + bl];
        if (of >= 0) {
            if (ROWS) ow0 = a.X[(size_t)of * ld + bl] - a.X[(size_t)ot * ld + bl];
            else {
                const size_t qf = (size_t)orf * ld + bl, qt = (size_t)ort * ld + bl;
                ow0 = opf_out_rows(a.out, a.Y, ld, bl, orf, ort);
                ow1 = fma(a.out.p[bl], opf_dy(a.DY[qf], a.L[qf], a.U[qf]), a.out.p[ld + bl] * opf_dy(a.DY[qt], a.L[qt], a.U[qt]));
            }
        }
    }
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r4 = 0.0;
    for (int k = k0; k < min(k0 + OPF_CHUNK, a.count); ++k) {
        if (ROWS) {                                                     // |A x - z|, |A x|, |z|, |dy|, u' dy+ + l' dy-
            double ax = 0.0;
            for (int p = ((CInt)a.ptr)[k]; p < ((CInt)a.ptr)[k + 1]; ++p) ax = fma(((CDbl)a.val)[p], a.X[(size_t)((CInt)a.idx)[p] * ld + bl], ax);
            if (OUT && (k == orf || k == ort)) ax = fma(a.out.p[(k == orf ? 0 : ld) + bl], ow0, ax);
            const size_t at = (size_t)k * ld + bl;
            const double z = a.Z[at], l = a.L[at], u = a.U[at], dy = opf_dy(a.DY[at], l, u);
            r0 = fmax(r0, fabs(ax - z)); r1 = fmax(r1, fabs(ax)); r2 = fmax(r2, fabs(z)); r3 = fmax(r3, fabs(dy));
            if (dy > 0.0) r4 = fma(u, dy, r4);
            else if (dy < 0.0) r4 = fma(l, dy, r4);
        } else {                                                        // |P x + q + A' y|, |P x|, |A' y|, |A' dy|
            double aty = 0.0, atd = 0.0;
            for (int p = ((CInt)a.ptr)[k]; p < ((CInt)a.ptr)[k + 1]; ++p) {
                const size_t at = (size_t)((CInt)a.idx)[p] * ld + bl;
                const double v = ((CDbl)a.val)[p];
                aty = fma(v, a.Y[at], aty);
                atd = fma(v, opf_dy(a.DY[at], a.L[at], a.U[at]), atd);
            }
            if (OUT && (k == of || k == ot)) { aty += k == of ? ow0 : -ow0; atd += k == of ? ow1 : -ow1; }
            const double px = ((CDbl)a.P)[k] * a.X[(size_t)k * ld + bl];
            r0 = fmax(r0, fabs(px + ((CDbl)a.q)[k] + aty)); r1 = fmax(r1, fabs(px)); r2 = fmax(r2, fabs(aty)); r3 = fmax(r3, fabs(atd));
        }
    }
    double* o = a.part + (size_t)chunk * (ROWS ? 5 : 4) * ld + bl;
    o[0] = r0; o[ld] = r1; o[2 * ld] = r2; o[3 * ld] = r3;
    if (ROWS) o[4 * ld] = r4;
}
// chunks in ascending order; a lane that is finished keeps its state.  Solved: both residuals within tol + tol x their norms (OSQP's rule).  Primal
// infeasible: |A' dy| <= eps |dy| and u' dy+ + l' dy- <= -eps |dy|
struct OpfVerdictArgs { const double* part_r; const double* part_v; double* rec; int* done; int* iters; double tol, q_norm; int chunks_r, chunks_v, ld, iteration; };
__global__ __launch_bounds__(64) void k_opf_verdict(OpfVerdictArgs a) {
    const size_t bl = (size_t)blockIdx.x * 64 + threadIdx.x, ld = (size_t)a.ld;
    double prim = 0.0, nax = 0.0, nz = 0.0, ndy = 0.0, sup = 0.0, dual = 0.0, npx = 0.0, naty = 0.0, natd = 0.0;
    for (int c = 0; c < a.chunks_r; ++c) {
        const double* o = a.part_r + (size_t)c * 5 * ld + bl;
        prim = fmax(prim, o[0]); nax = fmax(nax, o[ld]); nz = fmax(nz, o[2 * ld]); ndy = fmax(ndy, o[3 * ld]); sup += o[4 * ld];
    }
    for (int c = 0; c < a.chunks_v; ++c) {
        const double* o = a.part_v + (size_t)c * 4 * ld + bl;
        dual = fmax(dual, o[0]); npx = fmax(npx, o[ld]); naty = fmax(naty, o[2 * ld]); natd = fmax(natd, o[3 * ld]);
    }
    const double pn = fmax(nax, nz), dn = fmax(fmax(npx, naty), a.q_norm);
    int state = a.done[bl];
    if (!state) {
        // (NaN residuals compare false: the lane runs on to the iteration limit)
        if (prim <= a.tol + a.tol * pn && dual <= a.tol + a.tol * dn) state = 1;
        else if (ndy > OPF_EPS_INFEASIBLE && sup <= -OPF_EPS_INFEASIBLE * ndy && natd <= OPF_EPS_INFEASIBLE * ndy) state = 2;
        if (state) { a.done[bl] = state; a.iters[bl] = a.iteration; }
    }
    a.rec[bl] = (double)state; a.rec[ld + bl] = prim; a.rec[2 * ld + bl] = dual; a.rec[3 * ld + bl] = pn; a.rec[4 * ld + bl] = dn;
}

// ---- the low-rank correction of an outaged lane's solve: x~ = x0 - W M U' x0, M = (C^-1 + U' W)^-1 -------------------------------------------------
struct OpfCorrArgs {
    const int* on; const int* var; const int* ai; const double* av; const double* s; const double* W; double* M; double* G; double* XT; double* B;
    const int* groups;                                                  // nullable: groups 0 .. gridDim - 1
    int n, ld, depth;
};
__device__ __forceinline__ size_t corr_lane(const OpfCorrArgs& a, int block) { return (size_t)(a.groups ? a.groups[block] : block) * 64 + threadIdx.x; }
// a thread = a lane: U' x0 is a gather over the lane's short list (depth x 16 bytes of list, depth + 2 gathered doubles), then the 2 x 2 product
__global__ __launch_bounds__(64) void k_opf_outage_g(OpfCorrArgs a) {
    const size_t ld = (size_t)a.ld, bl = corr_lane(a, blockIdx.x);
    double g0 = 0.0, g1 = 0.0;
    if (a.on[bl]) {
        double u0 = 0.0;
        for (int q = 0; q < a.depth; ++q) u0 = fma(a.av[(size_t)q * ld + bl], a.XT[(size_t)a.ai[(size_t)q * ld + bl] * ld + bl], u0);
        const double u1 = a.XT[(size_t)a.var[bl] * ld + bl] - a.XT[(size_t)a.var[ld + bl] * ld + bl];
        g0 = fma(a.M[bl], u0, a.M[ld + bl] * u1);
        g1 = fma(a.M[2 * ld + bl], u0, a.M[3 * ld + bl] * u1);
    }
    a.G[bl] = g0; a.G[ld + bl] = g1;
}
// a wavefront = one variable x 64 lanes, coalesced like k_opf_rhs.  Bound by memory: it streams 2 n ld doubles of W and reads and writes n ld of x~ per
// iteration (32 bytes per variable and lane), beside the update pass's traffic; a wavefront none of whose lanes is corrected moves nothing
__global__ __launch_bounds__(256) void k_opf_outage_apply(OpfCorrArgs a) {
    const int j = blockIdx.x * 4 + uniform(threadIdx.y);
    if (j >= a.n) return;
    const size_t ld = (size_t)a.ld, bl = corr_lane(a, blockIdx.y), at = (size_t)j * ld + bl;
    if (!a.on[bl]) return;
    a.XT[at] = fma(-a.W[at], a.G[bl], fma(-a.W[(size_t)a.n * ld + at], a.G[ld + bl], a.XT[at]));
}
// the right-hand sides of W into B (zeroed before): column 0 the lane's a, column 1 its d.  A thread = a lane; a pad of the list adds 0 to variable 0
__global__ __launch_bounds__(64) void k_opf_outage_scatter(OpfCorrArgs a, int column) {
    const size_t ld = (size_t)a.ld, bl = corr_lane(a, blockIdx.x);
    if (!a.on[bl]) return;
    if (column == 0)
        for (int q = 0; q < a.depth; ++q) a.B[(size_t)a.ai[(size_t)q * ld + bl] * ld + bl] += a.av[(size_t)q * ld + bl];
    else { a.B[(size_t)a.var[bl] * ld + bl] = 1.0; a.B[(size_t)a.var[ld + bl] * ld + bl] = -1.0; }
}
// M = (C^-1 + U' W)^-1 with C^-1 = [[-s, 1], [1, 0]]; a thread = a lane.  A capacitance that cannot be inverted leaves NaN: the lane then runs to the limit
__global__ __launch_bounds__(64) void k_opf_outage_cap(OpfCorrArgs a) {
    const size_t ld = (size_t)a.ld, bl = corr_lane(a, blockIdx.x), nl = (size_t)a.n * ld;
    double m00 = 0.0, m01 = 0.0, m10 = 0.0, m11 = 0.0;
    if (a.on[bl]) {
        double aa = 0.0, ad = 0.0;
        for (int q = 0; q < a.depth; ++q) {
            const size_t at = (size_t)a.ai[(size_t)q * ld + bl] * ld + bl;
            aa = fma(a.av[(size_t)q * ld + bl], a.W[at], aa);
            ad = fma(a.av[(size_t)q * ld + bl], a.W[nl + at], ad);
        }
        const size_t f = (size_t)a.var[bl] * ld + bl, t = (size_t)a.var[ld + bl] * ld + bl;
        const double s00 = aa - a.s[bl], s01 = 1.0 + ad, s10 = 1.0 + (a.W[f] - a.W[t]), s11 = a.W[nl + f] - a.W[nl + t];
        const double det = s00 * s11 - s01 * s10;
        m00 = s11 / det; m01 = -s01 / det; m10 = -s10 / det; m11 = s00 / det;
    }
    a.M[bl] = m00; a.M[ld + bl] = m01; a.M[2 * ld + bl] = m10; a.M[3 * ld + bl] = m11;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
OpfOut out_of(const DcopfHandle* h) { return OpfOut{h->o_var, h->o_row, h->o_p}; }
OpfCorrArgs corr_of(const DcopfHandle* h, const int* glist) {
    return OpfCorrArgs{h->o_on, h->o_var, h->o_ai, h->o_av, h->o_s, h->o_W, h->o_M, h->o_g, h->XT, h->B, glist, h->n, h->ld, h->o_depth};
}
void launch_rhs(DcopfHandle* h, int groups, int blend, int form) {
    OpfRhsArgs a{h->c_ptr, h->c_row, h->c_val, h->rhov, h->qd, h->Z, h->Y, h->XT, h->X, h->B, h->done, h->glist, h->sigma, h->alpha, h->n, h->ld, blend, form,
                 out_of(h)};
    if (h->outages) hipLaunchKernelGGL((k_opf_rhs<true>), dim3((h->n + 3) / 4, groups), dim3(64, 4), 0, h->stream, a);
    else hipLaunchKernelGGL((k_opf_rhs<false>), dim3((h->n + 3) / 4, groups), dim3(64, 4), 0, h->stream, a);
}
void launch_correct(DcopfHandle* h, int groups) {
    const OpfCorrArgs c = corr_of(h, h->glist);
    hipLaunchKernelGGL(k_opf_outage_g, dim3(groups), dim3(64), 0, h->stream, c);
    hipLaunchKernelGGL(k_opf_outage_apply, dim3((h->n + 3) / 4, groups), dim3(64, 4), 0, h->stream, c);
}
void launch_sweep(DcopfHandle* h, int groups) {
    sweep_pair(h->fac, h->stream, 0, h->B, nullptr, nullptr, h->W, h->XT, h->ld, groups, h->glist);
    if (h->outages) launch_correct(h, groups);
}
void launch_update(DcopfHandle* h, int groups, int keep_dy) {
    OpfUpdateArgs a{h->r_ptr, h->r_col, h->r_val, h->rhov, h->rinv, h->XT, h->L, h->U, h->Z, h->Y, h->DY, h->done, h->glist, h->alpha, h->m, h->ld, keep_dy,
                    out_of(h)};
    if (h->outages) hipLaunchKernelGGL((k_opf_update<true>), dim3((h->m + 3) / 4, groups), dim3(64, 4), 0, h->stream, a);
    else hipLaunchKernelGGL((k_opf_update<false>), dim3((h->m + 3) / 4, groups), dim3(64, 4), 0, h->stream, a);
}
void launch_check(DcopfHandle* h, int groups, double tol, int iteration) {
    OpfResArgs r{h->r_ptr, h->r_col, h->r_val, h->Pd, h->qd, h->X, h->Z, h->Y, h->DY, h->L, h->U, h->part_r, h->glist, h->m, h->ld, out_of(h)};
    if (h->outages) hipLaunchKernelGGL((k_opf_residual<true, true>), dim3((h->chunks_r + 3) / 4, groups), dim3(64, 4), 0, h->stream, r);
    else hipLaunchKernelGGL((k_opf_residual<true, false>), dim3((h->chunks_r + 3) / 4, groups), dim3(64, 4), 0, h->stream, r);
    OpfResArgs v = r;
    v.ptr = h->c_ptr; v.idx = h->c_row; v.val = h->c_val; v.part = h->part_v; v.count = h->n;
    if (h->outages) hipLaunchKernelGGL((k_opf_residual<false, true>), dim3((h->chunks_v + 3) / 4, groups), dim3(64, 4), 0, h->stream, v);
    else hipLaunchKernelGGL((k_opf_residual<false, false>), dim3((h->chunks_v + 3) / 4, groups), dim3(64, 4), 0, h->stream, v);
    OpfVerdictArgs w{h->part_r, h->part_v, h->rec, h->done, h->iters, tol, h->q_norm, h->chunks_r, h->chunks_v, h->ld, iteration};
    hipLaunchKernelGGL(k_opf_verdict, dim3(h->ld / 64), dim3(64), 0, h->stream, w);     // every group: a group that left keeps its record
}

// rho per row, K's values from the term lists, the numeric factorisation on the kept tables
int assemble_and_factor(DcopfHandle* h, double sigma, bool compact) {
    std::vector<double> rhov, rinv;
    rho_rows(h->h_eq, h->rho, rhov, rinv);
    DC_HIP(sync_copy(h->rhov, rhov.data(), rhov.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->rinv, rinv.data(), rinv.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_fill(h->fac.bad, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_opf_gain, dim3((h->nnz_k + 255) / 256), dim3(256), 0, h->stream, h->g_ptr, h->g_row, h->g_prod, h->g_add, h->g_dg, h->rhov, sigma,
                       h->fac.A, h->nnz_k);
    factor_numeric(h->fac, h->stream);
    if (compact) { compact_sweep(h->fac, h->fac.fwd, h->stream); compact_sweep(h->fac, h->fac.bwd, h->stream); }
    DC_HIP(hipGetLastError());
    return 0;
}
// the outaged lanes' a = A' (rho o p) and s = p' (rho o p) at the handle's rho, W = K^-1 [a d] on the factor as it stands (two sweep pairs of batch
// width through B and the sweeps' scratch, which an iteration rewrites anyway) and the lanes' 2 x 2 inverses.  After every numeric factorisation
int build_outage(DcopfHandle* h) {
    if (!h->outages) return 0;
    const size_t ld = (size_t)h->ld, nb = (size_t)h->batch;
    std::vector<double> rhov, rinv, sv(ld, 0.0);
    rho_rows(h->h_eq, h->rho, rhov, rinv);
    std::vector<std::vector<std::pair<int, double>>> list(nb);
    int depth = 1;
    for (size_t s = 0; s < nb; ++s) {
        if (h->h_ostate[s] != 1) continue;
        std::vector<std::pair<int, double>>& a = list[s];
        for (int e = 0; e < 2; ++e) {
            const int r = h->h_orow[e * nb + s];
            const double pr = (e ? h->h_oy[s] : -h->h_oy[s]) * h->h_E[r], w = rhov[r] * pr;
            sv[s] = std::fma(w, pr, sv[s]);
            for (int p = h->h_rptr[r]; p < h->h_rptr[r + 1]; ++p) a.push_back({h->h_rcol[p], h->h_rval[p] * w});
        }
        std::sort(a.begin(), a.end());                                  // a column of both rows: its two terms added
        size_t k = 0;
        for (size_t q = 0; q < a.size(); ++q)
            if (k && a[k - 1].first == a[q].first) a[k - 1].second += a[q].second;
            else a[k++] = a[q];
        a.resize(k);
        depth = std::max(depth, (int)k);
    }
    if (depth > h->o_room) {
        dev_release(h, h->o_ai); dev_release(h, h->o_av);
        DC_TRY(dev_alloc(h, &h->o_ai, (size_t)depth * ld, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &h->o_av, (size_t)depth * ld, (const double*)nullptr, true));
        h->o_room = depth;
    }
    h->o_depth = depth;
    std::vector<int> ai((size_t)depth * ld, 0);
    std::vector<double> av((size_t)depth * ld, 0.0);
    for (size_t s = 0; s < nb; ++s)
        for (size_t q = 0; q < list[s].size(); ++q) { ai[q * ld + s] = list[s][q].first; av[q * ld + s] = list[s][q].second; }
    DC_HIP(sync_copy(h->o_ai, ai.data(), ai.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->o_av, av.data(), av.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->o_s, sv.data(), ld * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const int groups = h->ld / 64;
    const OpfCorrArgs c = corr_of(h, nullptr);
    for (int column = 0; column < 2; ++column) {
        DC_HIP(hipMemsetAsync(h->B, 0, (size_t)h->n * ld * sizeof(double), h->stream));
        hipLaunchKernelGGL(k_opf_outage_scatter, dim3(groups), dim3(64), 0, h->stream, c, column);
        sweep_pair(h->fac, h->stream, 0, h->B, nullptr, nullptr, h->W, h->o_W + (size_t)column * h->n * ld, h->ld, groups, nullptr);
    }
    hipLaunchKernelGGL(k_opf_outage_cap, dim3(groups), dim3(64), 0, h->stream, c);
    DC_HIP(hipGetLastError());
    return 0;
}

// K without sigma: a zero, negative, non-finite or vanishing pivot means variables that no row ties down
int probe_singular(DcopfHandle* h, const OpfModel& M) {
    DC_TRY(assemble_and_factor(h, 0.0, false));
    int bad = 0;
    std::vector<double> dinv(h->n), rhov, rinv;
    DC_HIP(sync_copy(&bad, h->fac.bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(sync_copy(dinv.data(), h->fac.dinv, dinv.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    rho_rows(M.eq, h->rho, rhov, rinv);
    double top = 0.0;
    for (int e = 0; e < h->nnz_k; ++e)
        if (M.g_dg[e] != 0.0) top = std::max(top, gain_entry(M.g_ptr.data(), M.g_row.data(), M.g_prod.data(), M.g_add.data(), M.g_dg.data(), rhov.data(), 0.0, e));
    h->singular = bad != 0;
    for (int k = 0; k < h->n; ++k)
        if (!(dinv[k] > 0.0) || !std::isfinite(dinv[k]) || !(1.0 / dinv[k] > OPF_SINGULAR * top)) h->singular = true;
    return 0;
}

int dcopf_create(DcopfHandle* h, const OpfModel& M, int64_t batch, double rho, double sigma, double alpha, int device) {
    const int n = M.n, m = M.m;
    h->n = n; h->m = m; h->batch = (int)batch; h->ld = (int)((batch + 63) / 64 * 64); h->device = device;
    h->rho = rho; h->sigma = sigma; h->alpha = alpha; h->cscale = M.cscale; h->q_norm = M.q_norm;
    h->h_P = M.P; h->h_q = M.q; h->h_E = M.E; h->h_rptr = M.rptr; h->h_rcol = M.rcol; h->h_rval = M.rval; h->h_eq = M.eq;
    h->nnz_k = M.kp[n];
    DC_HIP(hipSetDevice(device));
    DC_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    // A by columns, rows ascending
    std::vector<int> c_ptr(n + 1, 0);
    for (size_t p = 0; p < M.rcol.size(); ++p) c_ptr[M.rcol[p] + 1]++;
    for (int j = 0; j < n; ++j) c_ptr[j + 1] += c_ptr[j];
    std::vector<int> c_row(c_ptr[n]), cfill(c_ptr.begin(), c_ptr.end() - 1);
    std::vector<double> c_val(c_ptr[n]);
    for (int i = 0; i < m; ++i)
        for (int p = M.rptr[i]; p < M.rptr[i + 1]; ++p) { const int j = M.rcol[p]; c_row[cfill[j]] = i; c_val[cfill[j]++] = M.rval[p]; }
    DC_TRY(dev_alloc(h, &h->r_ptr, M.rptr.size(), M.rptr.data()));
    DC_TRY(dev_alloc(h, &h->r_col, M.rcol.size(), M.rcol.data()));
    DC_TRY(dev_alloc(h, &h->r_val, M.rval.size(), M.rval.data()));
    DC_TRY(dev_alloc(h, &h->c_ptr, c_ptr.size(), c_ptr.data()));
    DC_TRY(dev_alloc(h, &h->c_row, c_row.size(), c_row.data()));
    DC_TRY(dev_alloc(h, &h->c_val, c_val.size(), c_val.data()));
    DC_TRY(dev_alloc(h, &h->Pd, M.P.size(), M.P.data()));
    DC_TRY(dev_alloc(h, &h->qd, M.q.size(), M.q.data()));
    DC_TRY(dev_alloc(h, &h->g_ptr, M.g_ptr.size(), M.g_ptr.data()));
    DC_TRY(dev_alloc(h, &h->g_row, M.g_row.size(), M.g_row.data()));
    DC_TRY(dev_alloc(h, &h->g_prod, M.g_prod.size(), M.g_prod.data()));
    DC_TRY(dev_alloc(h, &h->g_add, M.g_add.size(), M.g_add.data()));
    DC_TRY(dev_alloc(h, &h->g_dg, M.g_dg.size(), M.g_dg.data()));
    const size_t Mr = (size_t)m, N = (size_t)n, ld = (size_t)h->ld;
    DC_TRY(dev_alloc(h, &h->rhov, Mr, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->rinv, Mr, (const double*)nullptr, true));
    // K is symmetric positive definite (sigma > 0): the scalar factor on a static order without pivoting is safe
    BlockSymbolic S;
    if (analyze(n, M.kp.data(), M.kc.data(), DC_POLICY_NO_TOP, S) != 0) { h->error = "symbolic analysis of the pattern of K failed"; return 1; }
    DcFactor& F = h->fac;
    DC_TRY(factor_tables(h, F, n, S));
    DC_TRY(dev_alloc(h, &F.A, (size_t)h->nnz_k, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.X, (size_t)S.n_entries + 1, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.dinv, N, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.bad, (size_t)1, (const int*)nullptr, true));
    DC_TRY(probe_singular(h, M));
    DC_TRY(assemble_and_factor(h, h->sigma, false));
    DC_TRY(build_sweep(h, F, F.fwd, forward_levels(n, S), S.l_ptr, S.l_ent, S.l_col, false, true));
    DC_TRY(build_sweep(h, F, F.bwd, S.bwd_level, S.u_ptr, S.u_ent, S.u_col, true, true));
    h->chunks_r = (m + OPF_CHUNK - 1) / OPF_CHUNK;
    h->chunks_v = (n + OPF_CHUNK - 1) / OPF_CHUNK;
    DC_TRY(dev_alloc(h, &h->X, N * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->XT, N * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->B, N * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->W, (N + 1) * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->Z, Mr * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->Y, Mr * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->DY, Mr * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->L, Mr * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->U, Mr * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->done, ld, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->iters, ld, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->glist, ld / 64, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->part_r, (size_t)h->chunks_r * 5 * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->part_v, (size_t)h->chunks_v * 4 * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->rec, (size_t)OPF_REC * ld, (const double*)nullptr, true));
    h->h_done.assign(ld, 0); h->h_iters.assign(ld, 0); h->h_status.assign(ld, 0);
    return 0;
}

// the groups with a lane that still runs go to h->glist; returns how many
int upload_groups(DcopfHandle* h, int* groups) {
    std::vector<int> g;
    for (int k = 0; k < h->ld / 64; ++k)
        for (int s = k * 64; s < k * 64 + 64; ++s)
            if (!h->h_done[s]) { g.push_back(k); break; }
    *groups = (int)g.size();
    if (!g.empty()) DC_HIP(sync_copy(h->glist, g.data(), g.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

// the run loop: between checks nothing is waited for; at a check one verdict record comes back
int dcopf_run(DcopfHandle* h, double tol, long long max_iter, int check, int adapt_every) {
    const size_t ld = (size_t)h->ld;
    for (size_t s = 0; s < ld; ++s) { h->h_done[s] = s < (size_t)h->batch ? 0 : 1; h->h_iters[s] = 0; }     // padding lanes never run
    if (h->outages)                                                     // nor do lanes whose outage is a bridge
        for (size_t s = 0; s < (size_t)h->batch; ++s) if (h->h_ostate[s] == 3) h->h_done[s] = 3;
    h->solved = true;
    if (h->singular) { std::fill(h->h_status.begin(), h->h_status.end(), 3); return 0; }
    DC_HIP(sync_copy(h->done, h->h_done.data(), ld * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_fill(h->iters, 0, ld * sizeof(int), h->stream));
    DC_HIP(hipMemsetAsync(h->DY, 0, (size_t)h->m * ld * sizeof(double), h->stream));
    int groups = 0;
    DC_TRY(upload_groups(h, &groups));
    std::vector<double> rec((size_t)OPF_REC * ld), ratio;
    int blend = 0;
    for (long long k = 1; k <= max_iter && groups > 0; ++k) {
        const bool at_check = k % check == 0 || k == max_iter;
        launch_rhs(h, groups, blend, 1);
        launch_sweep(h, groups);
        launch_update(h, groups, at_check ? 1 : 0);
        blend = 1;
        if (!at_check) continue;
        launch_rhs(h, groups, 1, 0);                                    // x+ of this step, for the residuals
        blend = 0;
        launch_check(h, groups, tol, (int)k);
        DC_HIP(hipGetLastError());
        DC_HIP(sync_copy(rec.data(), h->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        bool changed = false;
        for (size_t s = 0; s < (size_t)h->batch; ++s)
            if (!h->h_done[s] && rec[s] != 0.0) { h->h_done[s] = (int)rec[s]; h->h_iters[s] = (int)k; changed = true; }
        if (changed) DC_TRY(upload_groups(h, &groups));
        if (adapt_every > 0 && k % adapt_every == 0 && groups > 0) {
            ratio.clear();
            for (size_t s = 0; s < (size_t)h->batch; ++s)
                if (!h->h_done[s]) {
                    const double p = rec[ld + s] / (rec[3 * ld + s] + 1e-10), d = rec[2 * ld + s] / (rec[4 * ld + s] + 1e-10);
                    if (std::isfinite(p) && std::isfinite(d) && d > 0.0) ratio.push_back(std::sqrt(p / d));
                }
            if (!ratio.empty()) {
                std::nth_element(ratio.begin(), ratio.begin() + ratio.size() / 2, ratio.end());
                const double r = ratio[ratio.size() / 2];
                const double rho = std::min(std::max(h->rho * r, OPF_RHO_MIN), OPF_RHO_MAX);
                if ((r < 0.2 || r > 5.0) && rho != h->rho) {
                    h->rho = rho;
                    DC_TRY(assemble_and_factor(h, h->sigma, true));
                    DC_TRY(build_outage(h));                          // K and a = A' (rho o p) changed: W and the lanes' 2 x 2 inverses with them
                    h->refactorisations++;
                }
            }
        }
    }
    DC_HIP(hipStreamSynchronize(h->stream));
    for (size_t s = 0; s < (size_t)h->batch; ++s) {
        h->h_status[s] = h->h_done[s] == 1 ? 0 : h->h_done[s] == 2 ? 2 : h->h_done[s] == 3 ? 3 : 5;
        if (!h->h_done[s]) h->h_iters[s] = (int)max_iter;
    }
    return 0;
}

void dcopf_destroy(DcopfHandle* h) {
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void* p : h->allocs) hipFree(p);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

// [batch][rows] on the host -> [rows][ld] on the device, scaled per row
int push_lanes(DcopfHandle* h, double* dev, size_t rows, const std::vector<double>& t) {
    DC_HIP(sync_copy(dev, t.data(), rows * (size_t)h->ld * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return 0;
}
int fetch_lanes(DcopfHandle* h, const double* dev, size_t rows, std::vector<double>& t) {
    t.resize(rows * (size_t)h->ld);
    DC_HIP(sync_copy(t.data(), dev, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace
}  // namespace jg

using jg::DcopfHandle;
using jg::api_fail;

#define OPF_ENTER(h) DC_API_ENTER(jg::DcopfHandle, "null DC optimal power flow handle", h)

extern "C" {

int jg_dcopf_create(int64_t* out, int64_t n, int64_t m, const double* P, const double* q, const int64_t* rowptr, const int64_t* col, const double* val,
                    const int32_t* equality, int64_t batch, double rho, double sigma, double alpha, int device) {
    if (!out || !P || !q || !rowptr || !col || !val || !equality || n < 1 || n > (1 << 24) || m < 1 || m > (1 << 26) || batch < 1 || batch > (1 << 20) ||
        !(rho >= jg::OPF_RHO_MIN && rho <= jg::OPF_RHO_MAX) || !(sigma > 0.0) || !(alpha > 0.0 && alpha < 2.0))
        return api_fail(1, "jg_dcopf_create: bad argument");
    jg::OpfModel M;
    std::string err;
    if (const int rc = jg::opf_model(M, err, n, m, rowptr, col, val, P, q, equality)) { *out = 0; return api_fail(rc, "jg_dcopf_create: " + err); }
    DcopfHandle* h = new DcopfHandle();
    h->h_P0.assign(P, P + n); h->h_q0.assign(q, q + n);
    const int rc = jg::dcopf_create(h, M, batch, rho, sigma, alpha, device);
    if (rc) { const std::string msg = h->error; jg::dcopf_destroy(h); *out = 0; return api_fail(rc, msg); }
    *out = (int64_t)reinterpret_cast<intptr_t>(h);
    return 0;
}

void jg_dcopf_destroy(int64_t h) {
    if (h) jg::dcopf_destroy(reinterpret_cast<DcopfHandle*>(static_cast<intptr_t>(h)));
}

// device-free: the host set-up alone.  K [n][n] dense from the term lists at (rho, sigma), the objective's scale and the rows' scales
int jg_dcopf_host_model(int64_t n, int64_t m, const double* P, const double* q, const int64_t* rowptr, const int64_t* col, const double* val,
                        const int32_t* equality, double rho, double sigma, double* K, double* cscale, double* E) {
    if (!P || !q || !rowptr || !col || !val || !equality || !K || !cscale || !E || n < 1 || n > 4096 || m < 1) return api_fail(1, "jg_dcopf_host_model: bad argument");
    jg::OpfModel M;
    std::string err;
    if (const int rc = jg::opf_model(M, err, n, m, rowptr, col, val, P, q, equality)) return api_fail(rc, "jg_dcopf_host_model: " + err);
    std::vector<double> rhov, rinv;
    jg::rho_rows(M.eq, rho, rhov, rinv);
    std::fill(K, K + n * n, 0.0);
    for (int r = 0; r < (int)n; ++r)
        for (int e = M.kp[r]; e < M.kp[r + 1]; ++e)
            K[(size_t)r * n + M.kc[e]] = jg::gain_entry(M.g_ptr.data(), M.g_row.data(), M.g_prod.data(), M.g_add.data(), M.g_dg.data(), rhov.data(), sigma, e);
    *cscale = M.cscale;
    std::copy(M.E.begin(), M.E.end(), E);
    return 0;
}

int jg_dcopf_dims(int64_t h, int64_t* dims) {
    OPF_ENTER(h);
    if (!dims) return api_fail(1, "jg_dcopf_dims: null pointer");
    dims[0] = d->n; dims[1] = d->m; dims[2] = d->batch; dims[3] = d->ld; dims[4] = d->nnz_k; dims[5] = d->fac.n_entries; dims[6] = d->fac.n_fact_levels;
    dims[7] = d->refactorisations; dims[8] = d->singular ? 1 : 0;
    return 0;
}

int jg_dcopf_get_rho(int64_t h, double* rho) {
    OPF_ENTER(h);
    if (!rho) return api_fail(1, "jg_dcopf_get_rho: null pointer");
    *rho = d->rho;
    return 0;
}

int jg_dcopf_set_bounds(int64_t h, const double* l, const double* u) {
    OPF_ENTER(h);
    if (!l || !u) return api_fail(1, "jg_dcopf_set_bounds: null pointer");
    const size_t m = (size_t)d->m, ld = (size_t)d->ld;
    std::vector<double> tl(m * ld, 0.0), tu(m * ld, 0.0);
    for (size_t s = 0; s < (size_t)d->batch; ++s)
        for (size_t i = 0; i < m; ++i) {
            const double lo = l[s * m + i], up = u[s * m + i];
            if (std::isnan(lo) || std::isnan(up) || lo > up) return api_fail(1, "jg_dcopf_set_bounds: a bound is NaN or lower > upper");
            tl[i * ld + s] = lo <= -jg::OPF_INF ? -1e30 : d->h_E[i] * lo;
            tu[i * ld + s] = up >= jg::OPF_INF ? 1e30 : d->h_E[i] * up;
        }
    DC_RET(jg::push_lanes(d, d->L, m, tl));
    DC_RET(jg::push_lanes(d, d->U, m, tu));
    d->have_bounds = true; d->solved = false;
    return 0;
}

// warm start: x and y as jg_dcopf_get returns them, z = A x
int jg_dcopf_set_start(int64_t h, const double* x, const double* y) {
    OPF_ENTER(h);
    if (!x || !y) return api_fail(1, "jg_dcopf_set_start: null pointer");
    const size_t m = (size_t)d->m, n = (size_t)d->n, ld = (size_t)d->ld;
    std::vector<double> tx(n * ld, 0.0), ty(m * ld, 0.0), tz(m * ld, 0.0);
    for (size_t s = 0; s < (size_t)d->batch; ++s) {
        for (size_t j = 0; j < n; ++j) tx[j * ld + s] = x[s * n + j];
        for (size_t i = 0; i < m; ++i) {
            ty[i * ld + s] = y[s * m + i] * d->cscale / d->h_E[i];
            double ax = 0.0;
            for (int p = d->h_rptr[i]; p < d->h_rptr[i + 1]; ++p) ax = std::fma(d->h_rval[p], x[s * n + d->h_rcol[p]], ax);
            tz[i * ld + s] = ax;
        }
        if (d->outages && d->h_ostate[s] == 1) {                        // z = A_s x
            const size_t nb = (size_t)d->batch;
            const double dx = x[s * n + d->h_ovar[s]] - x[s * n + d->h_ovar[nb + s]];
            for (int e = 0; e < 2; ++e) {
                const size_t r = (size_t)d->h_orow[e * nb + s];
                tz[r * ld + s] = std::fma((e ? d->h_oy[s] : -d->h_oy[s]) * d->h_E[r], dx, tz[r * ld + s]);
            }
        }
    }
    DC_RET(jg::push_lanes(d, d->X, n, tx));
    DC_RET(jg::push_lanes(d, d->Y, m, ty));
    DC_RET(jg::push_lanes(d, d->Z, m, tz));
    d->solved = false;
    return 0;
}

// one branch out per lane: from_variable, to_variable [batch] the variables of the branch's two buses, from_row, to_row [batch] their balance rows
// (1-based, equality rows), admittance [batch] y_k as it stands in A, state [batch] 0 none / 1 outage / 3 the outage is a bridge: the lane is not
// run (status 3).  A lane of state 0 or 3 is not read beyond its state.  state NULL clears the set.  x, y, z stay as they are
int jg_dcopf_set_branch_outages(int64_t h, const int64_t* from_variable, const int64_t* to_variable, const int64_t* from_row, const int64_t* to_row,
                                const double* admittance, const int32_t* state) {
    OPF_ENTER(h);
    const size_t nb = (size_t)d->batch, ld = (size_t)d->ld;
    d->solved = false;
    if (!state) { d->outages = false; return 0; }
    if (!from_variable || !to_variable || !from_row || !to_row || !admittance) return api_fail(1, "jg_dcopf_set_branch_outages: null pointer");
    std::vector<int> st(nb), var(2 * nb, -1), row(2 * nb, -1);
    std::vector<double> y(nb, 0.0);
    bool any = false;
    for (size_t s = 0; s < nb; ++s) {
        st[s] = state[s];
        if (st[s] != 0 && st[s] != 1 && st[s] != 3) return api_fail(1, "jg_dcopf_set_branch_outages: a state is not 0, 1 or 3");
        any = any || st[s] != 0;
        if (st[s] != 1) continue;
        const int64_t f = from_variable[s], t = to_variable[s], rf = from_row[s], rt = to_row[s];
        if (f < 1 || f > d->n || t < 1 || t > d->n || f == t || rf < 1 || rf > d->m || rt < 1 || rt > d->m || rf == rt || !std::isfinite(admittance[s]))
            return api_fail(1, "jg_dcopf_set_branch_outages: variables in 1..n and distinct, rows in 1..m and distinct, a finite admittance");
        if (!d->h_eq[rf - 1] || !d->h_eq[rt - 1]) return api_fail(1, "jg_dcopf_set_branch_outages: the two rows must be equality rows");
        var[s] = (int)f - 1; var[nb + s] = (int)t - 1; row[s] = (int)rf - 1; row[nb + s] = (int)rt - 1; y[s] = admittance[s];
    }
    if (!any) { d->outages = false; return 0; }
    if (!d->o_on) {
        const size_t N = (size_t)d->n;
        DC_RET(jg::dev_alloc(d, &d->o_on, ld, (const int*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->o_var, 2 * ld, (const int*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->o_row, 2 * ld, (const int*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->o_p, 2 * ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->o_s, ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->o_M, 4 * ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->o_g, 2 * ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->o_W, 2 * N * ld, (const double*)nullptr, true));
    }
    std::vector<int> on(ld, 0), tv(2 * ld, -1), tr(2 * ld, -1);
    std::vector<double> tp(2 * ld, 0.0);
    for (size_t s = 0; s < nb; ++s) {
        if (st[s] != 1) continue;
        on[s] = 1;
        for (int e = 0; e < 2; ++e) {
            tv[e * ld + s] = var[e * nb + s]; tr[e * ld + s] = row[e * nb + s];
            tp[e * ld + s] = (e ? y[s] : -y[s]) * d->h_E[row[e * nb + s]];
        }
    }
    DC_API_HIP(jg::sync_copy(d->o_on, on.data(), on.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(jg::sync_copy(d->o_var, tv.data(), tv.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(jg::sync_copy(d->o_row, tr.data(), tr.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(jg::sync_copy(d->o_p, tp.data(), tp.size() * sizeof(double), hipMemcpyHostToDevice, d->stream));
    d->h_ostate = st; d->h_ovar = var; d->h_orow = row; d->h_oy = y;
    d->outages = true;
    DC_RET(jg::build_outage(d));
    return 0;
}

int jg_dcopf_run(int64_t h, double tolerance, int64_t max_iteration, int64_t check, int64_t adapt_every, int32_t* iterations, int32_t* status,
                 int64_t* refactorisations) {
    OPF_ENTER(h);
    if (!(tolerance > 0.0) || max_iteration < 1 || max_iteration > (1 << 30) || check < 1 || check > (1 << 20) || adapt_every < 0 || (adapt_every % check) != 0)
        return api_fail(1, "jg_dcopf_run: bad argument (adapt_every is 0 or a multiple of check)");
    if (!d->have_bounds) return api_fail(4, "jg_dcopf_run: jg_dcopf_set_bounds first");
    DC_RET(jg::dcopf_run(d, tolerance, max_iteration, (int)check, (int)adapt_every));
    for (int s = 0; s < d->batch; ++s) {
        if (iterations) iterations[s] = d->h_iters[s];
        if (status) status[s] = d->h_status[s];
    }
    if (refactorisations) *refactorisations = d->refactorisations;
    return 0;
}

int jg_dcopf_get(int64_t h, double* x, double* y, double* z, double* objective) {
    OPF_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dcopf_get: jg_dcopf_run first");
    const size_t m = (size_t)d->m, n = (size_t)d->n, ld = (size_t)d->ld;
    const double nan = std::nan("");
    auto skipped = [&](size_t s) { return d->h_status[s] == 3; };       // a lane that never ran (a bridge outage): NaN
    std::vector<double> t;
    if (x || objective) {
        DC_RET(jg::fetch_lanes(d, d->X, n, t));
        for (size_t s = 0; s < (size_t)d->batch; ++s) {
            double obj = 0.0;
            for (size_t j = 0; j < n; ++j) {
                const double v = skipped(s) ? nan : t[j * ld + s];
                if (x) x[s * n + j] = v;
                obj += (0.5 * d->h_P0[j] * v + d->h_q0[j]) * v;
            }
            if (objective) objective[s] = obj;
        }
    }
    if (y) {
        DC_RET(jg::fetch_lanes(d, d->Y, m, t));
        for (size_t s = 0; s < (size_t)d->batch; ++s)
            for (size_t i = 0; i < m; ++i) y[s * m + i] = skipped(s) ? nan : t[i * ld + s] * d->h_E[i] / d->cscale;
    }
    if (z) {
        DC_RET(jg::fetch_lanes(d, d->Z, m, t));
        for (size_t s = 0; s < (size_t)d->batch; ++s)
            for (size_t i = 0; i < m; ++i) z[s * m + i] = skipped(s) ? nan : t[i * ld + s] / d->h_E[i];
    }
    return 0;
}

// kernel: 0 one whole iteration, 1 right-hand side, 2 sweep pair, 3 projection step, 4 residual pass and verdict, 5 assembly of K and refactorisation,
// 6 the outaged lanes' correction of x~ (the gather and the pass over x~), 7 the build of W and the 2 x 2 inverses; 6 and 7 need a set of outages.
// The timed launches advance the lanes' iterates: set the start and run again for results
int jg_dcopf_time(int64_t h, int kernel, int reps, double* ms) {
    OPF_ENTER(h);
    if (!ms || reps < 1 || kernel < 0 || kernel > 7) return api_fail(1, "jg_dcopf_time: bad argument");
    if (kernel >= 6 && !d->outages) return api_fail(4, "jg_dcopf_time: jg_dcopf_set_branch_outages first");
    if (!d->have_bounds) return api_fail(4, "jg_dcopf_time: jg_dcopf_set_bounds first");
    std::fill(d->h_done.begin(), d->h_done.end(), 0);
    int groups = 0;
    DC_RET(jg::upload_groups(d, &groups));
    DC_API_HIP(jg::sync_fill(d->done, 0, (size_t)d->ld * sizeof(int), d->stream));
    const int rc = jg::time_events(d->stream, reps, ms, d->error, [&]() -> int {
        if (kernel == 0 || kernel == 1) jg::launch_rhs(d, groups, 1, 1);
        if (kernel == 0) jg::launch_sweep(d, groups);
        if (kernel == 2) jg::sweep_pair(d->fac, d->stream, 0, d->B, nullptr, nullptr, d->W, d->XT, d->ld, groups, d->glist);
        if (kernel == 6) jg::launch_correct(d, groups);
        if (kernel == 7) return jg::build_outage(d);
        if (kernel == 0 || kernel == 3) jg::launch_update(d, groups, 0);
        if (kernel == 4) jg::launch_check(d, groups, 1e-300, 0);
        if (kernel == 5) return jg::assemble_and_factor(d, d->sigma, true);
        return 0;
    });
    d->solved = false;
    return rc ? api_fail(rc, d->error) : 0;
}

}  // extern "C"
