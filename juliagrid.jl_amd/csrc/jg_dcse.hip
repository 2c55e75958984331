// jg_dcse.hip -- DC state estimation with batched bad-data removal on one shared scalar factor of the gain matrix (jg_dcse.hpp has the algebra and the
// reference lines it stands for).  The factorisation and the sweeps are jg_dc_sweep.hip's, on the pattern of G = H' W H; here: the gain assembly, the
// right-hand side H' W z, the residual pass (objective, normalised residuals, their arg-max), the Omega diagonal, the removal by compensation, the C ABI.
// Coefficient values, weights and indices are wave-uniform and go through scalar loads; every store is a vector store.
//
// Two residuals of the reference differ from z - H theta when the slack's angle a is not 0, and are restated as they are: residualTest! multiplies the
// coefficient WITHOUT its slack column by voltage.angle = theta + a (badData.jl:66-73), chiTest the full coefficient (:971).  So row i of the test
// subtracts roff_t[i] = a sum_{j != slack} H_ij and the objective roff_c[i] = a sum_j H_ij on top of r_i.  Both are 0 for a = 0.
#include "jg_dcse.hpp"
#include "jg_dc_abi.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/jgrid.h"
#include "jg_engine.hpp"

namespace jg {

namespace {

constexpr int K = DCSE_MAX_REMOVED;

// ---- gain assembly: G entries from products of H values x status x precision ----------------------------------------------------------------
__global__ void k_dcse_gain(const int* g_ptr, const int* g_row, const double* g_prod, const double* g_add, const double* ws, double* A, int nnz) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    double s = g_add[e];                                               // 1 on the slack's diagonal; the slack's row and column have no terms
    for (int t = g_ptr[e]; t < g_ptr[e + 1]; ++t) s = fma(g_prod[t], ws[g_row[t]], s);
    A[e] = s;
}

// ---- right-hand side b = H' W z: a wavefront = one state row x 64 lanes ---------------------------------------------------------------------
struct DcseRhsArgs { const int* c_ptr; const int* c_row; const double* c_val; const double* ws; const double* Z; double* B; int n, ld; };
__global__ __launch_bounds__(256) void k_dcse_rhs(DcseRhsArgs a) {
    const int j = blockIdx.x * 4 + uniform(threadIdx.y);
    if (j >= a.n) return;
    const size_t ld = (size_t)a.ld, bl = (size_t)blockIdx.y * 64 + threadIdx.x;
    double acc = 0.0;
    for (int p = ((CInt)a.c_ptr)[j]; p < ((CInt)a.c_ptr)[j + 1]; ++p) {
        const int i = ((CInt)a.c_row)[p];
        acc = fma(((CDbl)a.c_val)[p] * ((CDbl)a.ws)[i], a.Z[(size_t)i * ld + bl], acc);
    }
    a.B[(size_t)j * ld + bl] = acc;
}
__global__ void k_dcse_add(double* X, const double* D, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) X[i] += D[i];
}

// ---- residual pass: r = z - H theta, objective, normalised residuals and their arg-max, DCSE_ROWS rows per wavefront --------------------------
struct DcseResArgs {
    const int* r_ptr; const int* r_col; const double* r_val; const int* st; const double* ws; const double* wi;
    const double* Z; const double* TH;
    double* R;                                   // nullable: the residuals z - H theta, [m][ld]
    const double* omega; const double* roff_t; const double* roff_c;
    const int* rem; const int* cnt; const int* lstat; const double* U; const double* LD;       // REM
    double* NRM;                                 // nullable: every normalised residual, [m][ld]
    double* part;                                // [chunks][3][ld]
    int m, n, ld;
};
template <bool NORM, bool REM>
__global__ __launch_bounds__(256) void k_dcse_residual(DcseResArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * DCSE_ROWS;
    if (i0 >= a.m) return;
    const size_t ld = (size_t)a.ld, bl = (size_t)blockIdx.y * 64 + threadIdx.x, n = (size_t)a.n;
    int cnt = 0, rem[K];
    double LDv[K * K];
    if (REM) {
        cnt = a.lstat[bl] ? 0 : a.cnt[bl];
        for (int q = 0; q < K; ++q) rem[q] = q < cnt ? a.rem[(size_t)q * ld + bl] : -1;
        if (NORM)
            for (int q = 0; q < K * K; ++q) LDv[q] = a.LD[(size_t)q * ld + bl];
    }
    double obj = 0.0, mx = 0.0, arg = 0.0;
    for (int i = i0; i < min(i0 + DCSE_ROWS, a.m); ++i) {
        const int s = ((CInt)a.st)[i];
        double ht = 0.0, q[K];
        for (int b = 0; b < K; ++b) q[b] = 0.0;
        for (int p = ((CInt)a.r_ptr)[i]; p < ((CInt)a.r_ptr)[i + 1]; ++p) {
            const int c = ((CInt)a.r_col)[p];
            const double v = ((CDbl)a.r_val)[p];
            ht = fma(v, a.TH[(size_t)c * ld + bl], ht);
            if (REM && NORM)
                for (int b = 0; b < K; ++b)
                    if (b < cnt) q[b] = fma(v, a.U[((size_t)b * n + c) * ld + bl], q[b]);
        }
        bool gone = s == 0;
        if (REM)
            for (int b = 0; b < K; ++b) gone = gone || rem[b] == i;
        const double r = s ? a.Z[(size_t)i * ld + bl] - ht : 0.0;
        if (a.R) a.R[(size_t)i * ld + bl] = r;
        const double rc = gone ? 0.0 : r - ((CDbl)a.roff_c)[i];
        obj = fma(((CDbl)a.ws)[i] * rc, rc, obj);
        if (NORM) {
            const double rt = gone ? 0.0 : r - ((CDbl)a.roff_t)[i];
            double om = ((CDbl)a.omega)[i];
            if (REM) {                                                  // Omega'_ii = Omega_ii - q' (L D L')^-1 q: y = L^-1 q, sum y^2 / D
                double y[K];
                for (int b = 0; b < K; ++b) {
                    double t = q[b];
                    for (int c = 0; c < b; ++c) t -= LDv[b * K + c] * y[c];
                    y[b] = t;
                    if (b < cnt) om -= t * t / LDv[b * K + b];
                }
            }
            const double nr = rt != 0.0 ? fabs(rt) / sqrt(fabs(om)) : 0.0;      // badData.jl:73-82; first on ties (strict comparison, rows ascending)
            if (nr > mx) { mx = nr; arg = (double)(i + 1); }
            if (a.NRM) a.NRM[(size_t)i * ld + bl] = nr;
        }
    }
    double* o = a.part + (size_t)chunk * 3 * ld + bl;
    o[0] = obj; o[ld] = mx; o[2 * ld] = arg;
}
// chunks in ascending order: the objective's sum has a fixed order, ties of the maximum go to the lowest row
__global__ __launch_bounds__(64) void k_dcse_finish(const double* part, double* res, int chunks, int ld) {
    const size_t bl = (size_t)blockIdx.x * 64 + threadIdx.x, l = (size_t)ld;
    double obj = 0.0, mx = 0.0, arg = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const double* o = part + (size_t)c * 3 * l + bl;
        obj += o[0];
        if (o[l] > mx) { mx = o[l]; arg = o[2 * l]; }
    }
    res[bl] = obj; res[l + bl] = mx; res[2 * l + bl] = arg;
}

// ---- rows of H as right-hand sides (the Omega diagonal; the new columns of U) ------------------------------------------------------------------
// lane bl gets h_i' with i = rowid[bl] (-1: none), the slack's entry dropped; B [n][ld] is zero on entry
__global__ void k_dcse_row_rhs(const int* rowid, const int* r_ptr, const int* r_col, const double* r_val, const int* st, double* B, int ld, int slack) {
    const int bl = blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= ld) return;
    const int i = rowid[bl];
    if (i < 0 || !st[i]) return;
    for (int p = r_ptr[i]; p < r_ptr[i + 1]; ++p)
        if (r_col[p] != slack) B[(size_t)r_col[p] * ld + bl] = r_val[p];
}
__global__ void k_dcse_omega(const int* rowid, const int* r_ptr, const int* r_col, const double* r_val, const int* st, const double* wi, const double* Uo,
                             double* omega, int ld, int slack) {
    const int bl = blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= ld) return;
    const int i = rowid[bl];
    if (i < 0) return;
    double dot = 0.0;
    if (st[i])
        for (int p = r_ptr[i]; p < r_ptr[i + 1]; ++p)
            if (r_col[p] != slack) dot = fma(r_val[p], Uo[(size_t)r_col[p] * ld + bl], dot);
    omega[i] = wi[i] - dot;
}
// the new column of a lane goes to its slot cnt of U
__global__ void k_dcse_keep_column(const int* newrow, const int* cnt, const double* T, double* U, int n, int ld) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * ld) return;
    const size_t bl = i % ld, j = i / ld;
    if (newrow[bl] >= 0 && cnt[bl] < K) U[((size_t)cnt[bl] * n + j) * ld + bl] = T[i];      // (a full lane: k_dcse_extend gives it status 2)
}
// Omega_SS gains the row of the lane's new measurement: Omega_kb = delta_kb / w - h_k u_b, then one more row of L D L'.  A pivot at or below
// DCSE_SINGULAR / w_k: the measurement is critical in the lane's reduced set, status 1.
__global__ void k_dcse_extend(const int* newrow, int* rem, int* cnt, int* lstat, const double* U, double* LD, const double* wi,
                              const int* r_ptr, const int* r_col, const double* r_val, int n, int ld, int slack) {
    const int bl = blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= ld) return;
    const int i = newrow[bl];
    if (i < 0) return;
    const int k = cnt[bl];
    if (k >= K) { lstat[bl] = 2; return; }
    const size_t l = (size_t)ld;
    double om[K], Lk[K], D[K];
    for (int b = 0; b <= k; ++b) {
        double dot = 0.0;
        for (int p = r_ptr[i]; p < r_ptr[i + 1]; ++p)
            if (r_col[p] != slack) dot = fma(r_val[p], U[((size_t)b * n + r_col[p]) * l + bl], dot);
        om[b] = (b == k ? wi[i] : 0.0) - dot;
    }
    double d = om[k];
    for (int b = 0; b < k; ++b) {
        D[b] = LD[(size_t)(b * K + b) * l + bl];
        double t = om[b];
        for (int c = 0; c < b; ++c) t -= Lk[c] * D[c] * LD[(size_t)(b * K + c) * l + bl];
        Lk[b] = t / D[b];
        d -= Lk[b] * Lk[b] * D[b];
    }
    if (!(d > DCSE_SINGULAR * wi[i])) { lstat[bl] = 1; return; }
    for (int b = 0; b < k; ++b) LD[(size_t)(k * K + b) * l + bl] = Lk[b];
    LD[(size_t)(k * K + k) * l + bl] = d;
    rem[(size_t)k * l + bl] = i;
    cnt[bl] = k + 1;
}
// theta' = x - U Omega_SS^-1 r_S (NaN for a lane with a status), 8 state rows per wavefront
constexpr int DCSE_APPLY_ROWS = 8;
struct DcseApplyArgs { const double* X0; const double* U; const double* R; const double* LD; const int* rem; const int* cnt; const int* lstat; double* TH; int n, ld; };
__global__ __launch_bounds__(256) void k_dcse_apply(DcseApplyArgs a) {
    const size_t ld = (size_t)a.ld, bl = (size_t)blockIdx.y * 64 + threadIdx.x, n = (size_t)a.n;
    const int bad = a.lstat[bl], cnt = bad ? 0 : a.cnt[bl];
    double c[K];
    for (int b = 0; b < K; ++b) {                                       // L y = r_S
        double t = b < cnt ? a.R[(size_t)a.rem[(size_t)b * ld + bl] * ld + bl] : 0.0;
        for (int q = 0; q < b; ++q)
            if (b < cnt) t -= a.LD[(size_t)(b * K + q) * ld + bl] * c[q];
        c[b] = t;
    }
    for (int b = 0; b < K; ++b) c[b] = b < cnt ? c[b] / a.LD[(size_t)(b * K + b) * ld + bl] : 0.0;
    for (int b = K - 1; b >= 0; --b)                                    // L' c = y
        for (int q = b + 1; q < K; ++q)
            if (q < cnt) c[b] -= a.LD[(size_t)(q * K + b) * ld + bl] * c[q];
    const int j0 = (blockIdx.x * 4 + uniform(threadIdx.y)) * DCSE_APPLY_ROWS;
    for (int j = j0; j < min(j0 + DCSE_APPLY_ROWS, a.n); ++j) {
        double th = a.X0[(size_t)j * ld + bl];
        for (int b = 0; b < K; ++b)
            if (b < cnt) th = fma(-c[b], a.U[((size_t)b * n + j) * ld + bl], th);
        if (bad) th = __longlong_as_double(0x7ff8000000000000LL);
        a.TH[(size_t)j * ld + bl] = th;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
void launch_rhs(DcseHandle* h, const double* Z) {
    DcseRhsArgs a{h->c_ptr, h->c_row, h->c_val, h->ws, Z, h->B, h->n, h->ld};
    hipLaunchKernelGGL(k_dcse_rhs, dim3((h->n + 3) / 4, h->ld / 64), dim3(64, 4), 0, h->stream, a);
}
void sweep(DcseHandle* h, double* out) { sweep_pair(h->fac, h->stream, 0, h->B, nullptr, nullptr, h->W, out, h->ld, h->ld / 64, nullptr); }

template <bool NORM, bool REM>
void launch_residual(DcseHandle* h, const double* TH, double* R, double* NRM) {
    DcseResArgs a{};
    a.r_ptr = h->r_ptr; a.r_col = h->r_col; a.r_val = h->r_val; a.st = h->st; a.ws = h->ws; a.wi = h->wi; a.Z = h->Z; a.TH = TH; a.R = R;
    a.omega = h->omega; a.roff_t = h->roff_t; a.roff_c = h->roff_c; a.rem = h->rem; a.cnt = h->cnt; a.lstat = h->lstat; a.U = h->U; a.LD = h->LD;
    a.NRM = NRM; a.part = h->part; a.m = h->m; a.n = h->n; a.ld = h->ld;
    hipLaunchKernelGGL((k_dcse_residual<NORM, REM>), dim3((h->n_chunks + 3) / 4, h->ld / 64), dim3(64, 4), 0, h->stream, a);
    hipLaunchKernelGGL(k_dcse_finish, dim3(h->ld / 64), dim3(64), 0, h->stream, h->part, h->res, h->n_chunks, h->ld);
}
void launch_apply(DcseHandle* h) {
    DcseApplyArgs a{h->X0, h->U, h->R, h->LD, h->rem, h->cnt, h->lstat, h->TH, h->n, h->ld};
    const int per = 4 * DCSE_APPLY_ROWS;
    hipLaunchKernelGGL(k_dcse_apply, dim3((h->n + per - 1) / per, h->ld / 64), dim3(64, 4), 0, h->stream, a);
}

// the launch chain of a batch: right-hand side, sweep pair, residual pass; `correct`: one step theta += G^-1 H' W (z - H theta) on the same factor
// (the Orthogonal / PetersWilkinson tags); lanes with removed rows: the compensation and a second residual pass on the reduced set
int solve_chain(DcseHandle* h, int correct) {
    launch_rhs(h, h->Z);
    sweep(h, h->X0);
    launch_residual<false, false>(h, h->X0, h->R, nullptr);
    if (correct) {
        launch_rhs(h, h->R);
        sweep(h, h->TH);
        const size_t count = (size_t)h->n * h->ld;
        hipLaunchKernelGGL(k_dcse_add, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, h->X0, h->TH, count);
        launch_residual<false, false>(h, h->X0, h->R, nullptr);
    }
    h->cur = h->X0;
    if (h->any_removed) {
        launch_apply(h);
        launch_residual<false, true>(h, h->TH, nullptr, nullptr);
        h->cur = h->TH;
    }
    DC_HIP(hipGetLastError());
    return 0;
}

// the per-row constants that follow status and precision, then G and its factor
int assemble_and_factor(DcseHandle* h) {
    const int m = h->m;
    std::vector<double> ws(m), wi(m), rt(m), rc(m);
    for (int i = 0; i < m; ++i) {
        ws[i] = h->h_st[i] ? h->h_prec[i] : 0.0;
        wi[i] = 1.0 / h->h_prec[i];
        double all = 0.0, noslack = 0.0;
        for (int p = h->h_rptr[i]; p < h->h_rptr[i + 1]; ++p) { all += h->h_rval[p]; if (h->h_rcol[p] != h->slack) noslack += h->h_rval[p]; }
        rt[i] = h->h_st[i] ? h->slack_angle * noslack : 0.0;
        rc[i] = h->h_st[i] ? h->slack_angle * all : 0.0;
    }
    DC_HIP(sync_copy(h->st, h->h_st.data(), m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->ws, ws.data(), m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->wi, wi.data(), m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->roff_t, rt.data(), m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->roff_c, rc.data(), m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_fill(h->fac.bad, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_dcse_gain, dim3((h->nnz_gain + 255) / 256), dim3(256), 0, h->stream, h->g_ptr, h->g_row, h->g_prod, h->g_add, h->ws, h->fac.A, h->nnz_gain);
    factor_numeric(h->fac, h->stream);
    DC_HIP(hipGetLastError());
    return 0;
}
int check_pivots(DcseHandle* h) {
    int bad = 0;
    DC_HIP(sync_copy(&bad, h->fac.bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (bad) { h->error = "zero or non-finite pivot in the gain matrix: the measurement set does not make the grid observable"; return 3; }
    return 0;
}
int reset_removed(DcseHandle* h) {
    std::fill(h->h_cnt.begin(), h->h_cnt.end(), 0);
    std::fill(h->h_stat.begin(), h->h_stat.end(), 0);
    std::fill(h->h_rem.begin(), h->h_rem.end(), -1);
    h->any_removed = false;
    DC_HIP(sync_fill(h->cnt, 0, (size_t)h->ld * sizeof(int), h->stream));
    DC_HIP(sync_fill(h->lstat, 0, (size_t)h->ld * sizeof(int), h->stream));
    DC_HIP(sync_fill(h->rem, 0xff, (size_t)K * h->ld * sizeof(int), h->stream));
    return 0;
}

int dcse_create(DcseHandle* h, int64_t n64, int64_t m64, const int64_t* rowptr, const int64_t* col, const double* val, const double* precision,
                const int32_t* status, int64_t slack1, double slack_angle, int64_t batch, int device) {
    const int n = (int)n64, m = (int)m64;
    h->n = n; h->m = m; h->batch = (int)batch; h->ld = (int)((batch + 63) / 64 * 64); h->device = device; h->slack = (int)slack1 - 1; h->slack_angle = slack_angle;
    if (rowptr[0] != 0) { h->error = "rowptr is not 0-based"; return 1; }
    const int64_t nnz = rowptr[m];
    if (nnz < 1 || nnz > (1 << 28)) { h->error = "the coefficient matrix is empty or too large"; return 1; }
    h->h_rptr.resize(m + 1); h->h_rcol.resize(nnz); h->h_rval.assign(val, val + nnz); h->h_prec.assign(precision, precision + m); h->h_st.resize(m);
    for (int i = 0; i <= m; ++i) h->h_rptr[i] = (int)rowptr[i];
    for (int i = 0; i < m; ++i) {
        if (rowptr[i + 1] < rowptr[i] || rowptr[i + 1] > nnz) { h->error = "rowptr is not monotone"; return 1; }
        if (!(precision[i] > 0.0) || !std::isfinite(precision[i])) { h->error = "precision must be positive and finite"; return 1; }
        if (status[i] != 0 && status[i] != 1) { h->error = "status must be 0 or 1"; return 1; }
        h->h_st[i] = status[i];
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            if (col[p] < 1 || col[p] > n || (p > rowptr[i] && col[p] <= col[p - 1])) { h->error = "col: columns of a row must be ascending, unique and in 1..n"; return 1; }
            h->h_rcol[p] = (int)col[p] - 1;
        }
    }
    const int slack = h->slack;
    // pattern of G: the union over rows of H of all column pairs, plus the whole diagonal (a state no row touches is then a zero pivot: unobservable)
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
    // per entry of G its (row of H, coefficient product) terms, rows ascending; the slack's row and column carry none (G[slack, slack] = 1, :346-353)
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
        else {
            DC_HIP(hipSetDevice(device));
            DC_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
            DC_TRY(dev_alloc(h, &h->g_row, g_row.size(), g_row.data()));
            DC_TRY(dev_alloc(h, &h->g_prod, g_prod.size(), g_prod.data()));
        }
    }
    std::vector<double> g_add(nnzg, 0.0);
    g_add[entry(slack, slack)] = 1.0;
    DC_TRY(dev_alloc(h, &h->g_ptr, g_ptr.size(), g_ptr.data()));
    DC_TRY(dev_alloc(h, &h->g_add, g_add.size(), g_add.data()));
    // H' by state columns (rows ascending), the slack's list empty
    std::vector<int> c_ptr(n + 1, 0);
    for (int64_t p = 0; p < nnz; ++p) if (h->h_rcol[p] != slack) c_ptr[h->h_rcol[p] + 1]++;
    for (int j = 0; j < n; ++j) c_ptr[j + 1] += c_ptr[j];
    std::vector<int> c_row(c_ptr[n]), cfill(c_ptr.begin(), c_ptr.end() - 1);
    std::vector<double> c_val(c_ptr[n]);
    for (int i = 0; i < m; ++i)
        for (int p = h->h_rptr[i]; p < h->h_rptr[i + 1]; ++p) {
            const int j = h->h_rcol[p];
            if (j != slack) { c_row[cfill[j]] = i; c_val[cfill[j]++] = h->h_rval[p]; }
        }
    DC_TRY(dev_alloc(h, &h->c_ptr, c_ptr.size(), c_ptr.data()));
    DC_TRY(dev_alloc(h, &h->c_row, c_row.size(), c_row.data()));
    DC_TRY(dev_alloc(h, &h->c_val, c_val.size(), c_val.data()));
    DC_TRY(dev_alloc(h, &h->r_ptr, h->h_rptr.size(), h->h_rptr.data()));
    DC_TRY(dev_alloc(h, &h->r_col, h->h_rcol.size(), h->h_rcol.data()));
    DC_TRY(dev_alloc(h, &h->r_val, h->h_rval.size(), h->h_rval.data()));
    // symbolic analysis of G's pattern, no top tasks (DC_POLICY_NO_TOP); G is symmetric positive definite when the set is observable, so the
    // scalar factor without pivoting is safe
    BlockSymbolic S;
    if (analyze(n, rp.data(), ci.data(), DC_POLICY_NO_TOP, S) != 0) { h->error = "symbolic analysis of the gain pattern failed"; return 1; }
    DcFactor& F = h->fac;
    DC_TRY(factor_tables(h, F, n, S));
    const size_t M = (size_t)m, ld = (size_t)h->ld, N = (size_t)n;
    DC_TRY(dev_alloc(h, &F.A, (size_t)nnzg, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.X, (size_t)S.n_entries + 1, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.dinv, N, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.bad, (size_t)1, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->st, M, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->ws, M, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->wi, M, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->roff_t, M, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->roff_c, M, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->omega, M, (const double*)nullptr, true));
    DC_TRY(assemble_and_factor(h));
    DC_TRY(build_sweep(h, F, F.fwd, forward_levels(n, S), S.l_ptr, S.l_ent, S.l_col, false, true));
    DC_TRY(build_sweep(h, F, F.bwd, S.bwd_level, S.u_ptr, S.u_ent, S.u_col, true, true));
    DC_TRY(check_pivots(h));
    h->n_chunks = (m + DCSE_ROWS - 1) / DCSE_ROWS;
    DC_TRY(dev_alloc(h, &h->Z, M * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->R, M * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->B, N * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->W, (N + 1) * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->X0, N * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->TH, N * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->part, (size_t)h->n_chunks * 3 * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->res, 3 * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->rem, (size_t)K * ld, (const int*)nullptr, false));
    DC_TRY(dev_alloc(h, &h->cnt, ld, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->lstat, ld, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->newrow, std::max<size_t>(ld, DCSE_OMEGA_LD), (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->glist, ld / 64, (const int*)nullptr, true));
    h->h_cnt.assign(ld, 0); h->h_stat.assign(ld, 0); h->h_rem.assign((size_t)K * ld, -1);
    DC_TRY(reset_removed(h));
    h->cur = h->X0;
    return 0;
}

}  // namespace

// (jg_dcse_critical.hip fills its right-hand sides with the same kernel)
void launch_row_rhs(DcseHandle* h, const int* rowid, double* B, int ld) {
    hipLaunchKernelGGL(k_dcse_row_rhs, dim3((ld + 255) / 256), dim3(256), 0, h->stream, rowid, h->r_ptr, h->r_col, h->r_val, h->st, B, ld, h->slack);
}

// Omega_ii = 1 / w_i - h_i G^-1 h_i' for every row, rows of H as the lanes of the shared sweep pair, DCSE_OMEGA_LD rows per pair
int compute_omega(DcseHandle* h) {
    const int ldo = DCSE_OMEGA_LD;
    const size_t N = (size_t)h->n;
    double* Bo = nullptr; double* Wo = nullptr; double* Uo = nullptr;
    DC_TRY(dev_alloc(h, &Bo, N * ldo, (const double*)nullptr, false));
    DC_TRY(dev_alloc(h, &Wo, (N + 1) * ldo, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &Uo, N * ldo, (const double*)nullptr, false));
    std::vector<int> ids(ldo);
    int rc = 0;
    for (int i0 = 0; i0 < h->m && !rc; i0 += ldo) {
        for (int s = 0; s < ldo; ++s) ids[s] = i0 + s < h->m ? i0 + s : -1;
        hipError_t e = hipMemcpyAsync(h->newrow, ids.data(), ldo * sizeof(int), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);                    // ids is reused
        if (e == hipSuccess) e = hipMemsetAsync(Bo, 0, N * ldo * sizeof(double), h->stream);
        if (e != hipSuccess) { h->error = std::string("Omega diagonal: ") + hipGetErrorString(e); rc = 2; break; }
        hipLaunchKernelGGL(k_dcse_row_rhs, dim3(ldo / 256), dim3(256), 0, h->stream, h->newrow, h->r_ptr, h->r_col, h->r_val, h->st, Bo, ldo, h->slack);
        sweep_pair(h->fac, h->stream, 0, Bo, nullptr, nullptr, Wo, Uo, ldo, ldo / 64, nullptr);
        hipLaunchKernelGGL(k_dcse_omega, dim3(ldo / 256), dim3(256), 0, h->stream, h->newrow, h->r_ptr, h->r_col, h->r_val, h->st, h->wi, Uo, h->omega, ldo, h->slack);
    }
    hipError_t e = hipStreamSynchronize(h->stream);
    if (!rc && e == hipSuccess) e = hipGetLastError();
    dev_release(h, Bo); dev_release(h, Wo); dev_release(h, Uo);
    if (rc) return rc;
    if (e != hipSuccess) { h->error = std::string("Omega diagonal: ") + hipGetErrorString(e); return 2; }
    h->omega_valid = true;
    h->omega_runs++;
    return 0;
}

namespace {

int run_test_pass(DcseHandle* h, double* NRM) {
    if (!h->omega_valid) DC_TRY(compute_omega(h));
    if (h->any_removed) launch_residual<true, true>(h, h->cur, nullptr, NRM);
    else launch_residual<true, false>(h, h->cur, nullptr, NRM);
    DC_HIP(hipGetLastError());
    return 0;
}

// the lanes in `rows` (>= 0: the row that leaves the lane's set) get one more column of U and one more row of Omega_SS
int remove_rows(DcseHandle* h, const std::vector<int>& rows) {
    const size_t N = (size_t)h->n, ld = (size_t)h->ld;
    if (!h->U) {
        DC_TRY(dev_alloc(h, &h->U, (size_t)K * N * ld, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &h->TMP, N * ld, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &h->LD, (size_t)K * K * ld, (const double*)nullptr, true));
    }
    std::vector<int> groups;
    for (size_t g = 0; g < ld / 64; ++g)
        for (size_t s = g * 64; s < g * 64 + 64; ++s)
            if (rows[s] >= 0) { groups.push_back((int)g); break; }
    if (groups.empty()) return 0;
    DC_HIP(sync_copy(h->newrow, rows.data(), ld * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->glist, groups.data(), groups.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DC_HIP(hipMemsetAsync(h->B, 0, N * ld * sizeof(double), h->stream));
    const int tb = (int)((ld + 255) / 256);
    hipLaunchKernelGGL(k_dcse_row_rhs, dim3(tb), dim3(256), 0, h->stream, h->newrow, h->r_ptr, h->r_col, h->r_val, h->st, h->B, h->ld, h->slack);
    sweep_pair(h->fac, h->stream, 0, h->B, nullptr, nullptr, h->W, h->TMP, h->ld, (int)groups.size(), h->glist);
    hipLaunchKernelGGL(k_dcse_keep_column, dim3((unsigned)((N * ld + 255) / 256)), dim3(256), 0, h->stream, h->newrow, h->cnt, h->TMP, h->U, h->n, h->ld);
    hipLaunchKernelGGL(k_dcse_extend, dim3(tb), dim3(256), 0, h->stream, h->newrow, h->rem, h->cnt, h->lstat, h->U, h->LD, h->wi, h->r_ptr, h->r_col, h->r_val,
                       h->n, h->ld, h->slack);
    DC_HIP(hipGetLastError());
    DC_HIP(sync_copy(h->h_cnt.data(), h->cnt, ld * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(sync_copy(h->h_stat.data(), h->lstat, ld * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(sync_copy(h->h_rem.data(), h->rem, (size_t)K * ld * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    h->any_removed = true;
    h->solved = false;
    return 0;
}

void dcse_destroy(DcseHandle* h) {
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void* p : h->allocs) hipFree(p);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

}  // namespace
}  // namespace jg

using jg::DcseHandle;

using jg::api_fail;

namespace {
// [rows][ld] on the device -> [batch][rows] on the host
int fetch_lanes(DcseHandle* d, const double* dev, size_t rows, double* out, double add) {
    const size_t ld = (size_t)d->ld;
    std::vector<double> t(rows * ld);
    if (jg::sync_copy(t.data(), dev, rows * ld * sizeof(double), hipMemcpyDeviceToHost, d->stream) != hipSuccess) { d->error = "device to host copy failed"; return 2; }
    for (size_t s = 0; s < (size_t)d->batch; ++s)
        for (size_t i = 0; i < rows; ++i) out[s * rows + i] = t[i * ld + s] + add;
    return 0;
}
}  // namespace

extern "C" {

int jg_dcse_create(int64_t* out, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* col, const double* val, const double* precision,
                   const int32_t* status, int64_t slack, double slack_angle, int64_t batch, int device) {
    if (!out || !rowptr || !col || !val || !precision || !status || n < 1 || n > (1 << 24) || m < 1 || m > (1 << 26) || slack < 1 || slack > n || batch < 1 ||
        batch > (1 << 20))
        return api_fail(1, "jg_dcse_create: bad argument");
    DcseHandle* h = new DcseHandle();
    const int rc = jg::dcse_create(h, n, m, rowptr, col, val, precision, status, slack, slack_angle, batch, device);
    if (rc) { const std::string msg = h->error; jg::dcse_destroy(h); *out = 0; return api_fail(rc, msg); }
    *out = (int64_t)reinterpret_cast<intptr_t>(h);
    return 0;
}

void jg_dcse_destroy(int64_t h) {
    if (h) jg::dcse_destroy(reinterpret_cast<DcseHandle*>(static_cast<intptr_t>(h)));
}

int jg_dcse_dims(int64_t h, int64_t* dims) {
    SE_ENTER(h);
    if (!dims) return api_fail(1, "jg_dcse_dims: null pointer");
    dims[0] = d->n; dims[1] = d->m; dims[2] = d->batch; dims[3] = d->ld; dims[4] = d->nnz_gain; dims[5] = d->fac.n_entries; dims[6] = d->fac.n_fact_levels;
    dims[7] = (int64_t)d->fac.fwd.h_lev.size() - 1; dims[8] = (int64_t)d->fac.bwd.h_lev.size() - 1;
    dims[9] = (int64_t)(d->fac.fwd.launches.size() + d->fac.bwd.launches.size()); dims[10] = d->fac.fwd.terms + d->fac.bwd.terms;
    dims[11] = d->refactorisations; dims[12] = d->omega_runs; dims[13] = jg::DCSE_MAX_REMOVED;
    return 0;
}

int jg_dcse_set_weights(int64_t h, const double* precision, const int32_t* status) {
    SE_ENTER(h);
    if (!precision || !status) return api_fail(1, "jg_dcse_set_weights: null pointer");
    for (int i = 0; i < d->m; ++i)
        if (!(precision[i] > 0.0) || !std::isfinite(precision[i]) || (status[i] != 0 && status[i] != 1)) return api_fail(1, "jg_dcse_set_weights: precision must be positive, status 0 or 1");
    d->h_prec.assign(precision, precision + d->m);
    for (int i = 0; i < d->m; ++i) d->h_st[i] = status[i];
    d->solved = false; d->omega_valid = false;
    DC_RET(jg::assemble_and_factor(d));
    jg::compact_sweep(d->fac, d->fac.fwd, d->stream);
    jg::compact_sweep(d->fac, d->fac.bwd, d->stream);
    DC_API_HIP(hipGetLastError());
    d->refactorisations++;
    DC_RET(jg::reset_removed(d));
    DC_RET(jg::check_pivots(d));
    return 0;
}

int jg_dcse_set_readings(int64_t h, int64_t lane0, int64_t count, const double* z) {
    SE_ENTER(h);
    if (lane0 < 0 || count < 1 || lane0 + count > d->batch || !z) return api_fail(1, "jg_dcse_set_readings: lanes out of range");
    const size_t m = (size_t)d->m, ld = (size_t)d->ld;
    std::vector<double> t(m * (size_t)count);
    for (size_t s = 0; s < (size_t)count; ++s)
        for (size_t i = 0; i < m; ++i) t[i * count + s] = z[s * m + i];
    DC_API_HIP(hipMemcpy2DAsync(d->Z + lane0, ld * sizeof(double), t.data(), (size_t)count * sizeof(double), (size_t)count * sizeof(double), m, hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    d->have_z = true; d->solved = false;
    return 0;
}

int jg_dcse_solve(int64_t h, int correct) {
    SE_ENTER(h);
    if (!d->have_z) return api_fail(4, "jg_dcse_solve: jg_dcse_set_readings first");
    DC_RET(jg::solve_chain(d, correct));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    d->solved = true;
    return 0;
}

int jg_dcse_get_angle(int64_t h, double* theta, int32_t* status, double* objective) {
    SE_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dcse_get_angle: jg_dcse_solve first");
    if (theta) {
        DC_RET(fetch_lanes(d, d->cur, (size_t)d->n, theta, d->slack_angle));
        for (size_t s = 0; s < (size_t)d->batch; ++s)
            if (!d->h_stat[s]) theta[s * d->n + d->slack] = d->slack_angle;
    }
    if (status) for (int s = 0; s < d->batch; ++s) status[s] = d->h_stat[s];
    if (objective) {
        DC_RET(fetch_lanes(d, d->res, 1, objective, 0.0));
        for (int s = 0; s < d->batch; ++s) if (d->h_stat[s]) objective[s] = std::nan("");
    }
    return 0;
}

int jg_dcse_residual_test(int64_t h, double threshold, int remove, double* maximum, int32_t* index) {
    SE_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dcse_residual_test: jg_dcse_solve first");
    if (!maximum || !index) return api_fail(1, "jg_dcse_residual_test: null pointer");
    DC_RET(jg::run_test_pass(d, nullptr));
    const size_t ld = (size_t)d->ld;
    std::vector<double> res(3 * ld);
    DC_API_HIP(jg::sync_copy(res.data(), d->res, 3 * ld * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    std::vector<int> rows(ld, -1);
    bool any = false;
    for (int s = 0; s < d->batch; ++s) {
        maximum[s] = d->h_stat[s] ? std::nan("") : res[ld + s];
        index[s] = d->h_stat[s] ? 0 : (int32_t)res[2 * ld + s];
        if (remove && !d->h_stat[s] && index[s] > 0 && maximum[s] > threshold) { rows[s] = index[s] - 1; any = true; }
    }
    if (any) DC_RET(jg::remove_rows(d, rows));
    return 0;
}

int jg_dcse_remove_rows(int64_t h, const int32_t* rows) {
    SE_ENTER(h);
    if (!rows) return api_fail(1, "jg_dcse_remove_rows: null pointer");
    std::vector<int> r(d->ld, -1);
    for (int s = 0; s < d->batch; ++s) {
        if (rows[s] < 0 || rows[s] > d->m) return api_fail(1, "jg_dcse_remove_rows: row out of range");
        if (rows[s] == 0 || d->h_stat[s]) continue;
        for (int q = 0; q < d->h_cnt[s]; ++q)
            if (d->h_rem[(size_t)q * d->ld + s] == rows[s] - 1) return api_fail(1, "jg_dcse_remove_rows: the lane has removed that row already");
        if (!d->h_st[rows[s] - 1]) return api_fail(1, "jg_dcse_remove_rows: the row is out of service");
        r[s] = rows[s] - 1;
    }
    DC_RET(jg::remove_rows(d, r));
    return 0;
}

int jg_dcse_get_normalized_residual(int64_t h, double* r) {
    SE_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dcse_get_normalized_residual: jg_dcse_solve first");
    if (!r) return api_fail(1, "jg_dcse_get_normalized_residual: null pointer");
    if (!d->NRM) DC_RET(jg::dev_alloc(d, &d->NRM, (size_t)d->m * d->ld, (const double*)nullptr, true));
    DC_RET(jg::run_test_pass(d, d->NRM));
    DC_RET(fetch_lanes(d, d->NRM, (size_t)d->m, r, 0.0));
    return 0;
}

int jg_dcse_get_removed(int64_t h, int32_t* rows, int32_t* count) {
    SE_ENTER(h);
    if (!rows || !count) return api_fail(1, "jg_dcse_get_removed: null pointer");
    for (int s = 0; s < d->batch; ++s) {
        count[s] = d->h_cnt[s];
        for (int q = 0; q < jg::DCSE_MAX_REMOVED; ++q) rows[s * jg::DCSE_MAX_REMOVED + q] = q < d->h_cnt[s] ? d->h_rem[(size_t)q * d->ld + s] + 1 : 0;
    }
    return 0;
}

int jg_dcse_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, const double* shift) {
    SE_ENTER(h);
    if (nbr < 1 || !from || !to || !admittance || !shift) return api_fail(1, "jg_dcse_set_branches: bad argument");
    if (d->nbr) return api_fail(1, "jg_dcse_set_branches: the branch table is already set");
    std::vector<int> f(nbr), t(nbr);
    for (int64_t k = 0; k < nbr; ++k) {
        if (from[k] < 1 || from[k] > d->n || to[k] < 1 || to[k] > d->n) return api_fail(1, "jg_dcse_set_branches: bus index out of range");
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

int jg_dcse_get_flows(int64_t h, double* from) {
    SE_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dcse_get_flows: jg_dcse_solve first");
    if (!d->nbr) return api_fail(1, "jg_dcse_get_flows: jg_dcse_set_branches first");
    if (!from) return api_fail(1, "jg_dcse_get_flows: null pointer");
    jg::DcFlowArgs f{};
    f.TH = d->cur; f.bf = d->b_from; f.bt = d->b_to; f.by = d->b_y; f.bs = d->b_shift; f.rating = nullptr; f.obr = d->o_none;
    f.flows = d->flows; f.part = d->fpart; f.nbr = d->nbr; f.ld = d->ld;
    jg::launch_dc_flows(f, false, dim3((d->n_fchunks + 3) / 4, d->ld / 64), d->stream);
    DC_API_HIP(hipGetLastError());
    DC_RET(fetch_lanes(d, d->flows, (size_t)d->nbr, from, 0.0));
    return 0;
}

int jg_dcse_time_kernel(int64_t h, int kernel, int reps, double* ms) {
    SE_ENTER(h);
    if (!ms || reps < 1 || kernel < 0 || kernel > 5) return api_fail(1, "jg_dcse_time_kernel: bad argument");
    if (!d->solved) return api_fail(4, "jg_dcse_time_kernel: jg_dcse_solve first");
    int rc = jg::time_events(d->stream, reps, ms, d->error, [&]() -> int {
        if (kernel == 5) d->omega_valid = false;
        if (kernel == 0) return jg::solve_chain(d, 0);
        if (kernel == 1) jg::launch_rhs(d, d->Z);
        else if (kernel == 2) jg::sweep(d, d->X0);
        else if (kernel == 3) jg::launch_residual<false, false>(d, d->X0, d->R, nullptr);
        else return jg::run_test_pass(d, nullptr);                          // 4: the normalised pass; 5: the Omega diagonal before it
        return 0;
    });
    if (!rc && kernel != 0) {                                               // leave the handle as a solve left it
        rc = jg::solve_chain(d, 0);
        if (!rc && hipStreamSynchronize(d->stream) != hipSuccess) { rc = 2; d->error = "hipStreamSynchronize failed"; }
    }
    return rc ? api_fail(rc, d->error) : 0;
}

}  // extern "C"
