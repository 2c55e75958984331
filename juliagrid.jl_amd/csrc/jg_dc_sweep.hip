// jg_dc_sweep.hip -- the one compiled copy of what every DC handle runs on (jg_dc_sweep.hpp declares it): the scalar factorisation kernels, the
// level-scheduled sweep kernels with scenarios as lanes, the branch-flow kernel and their launchers.  Nothing here keeps state of its own: every call
// works on the DcFactor and the stream it is given.
#include "jg_dc_sweep.hpp"

namespace jg {

namespace {

#ifndef JG_DC_CHAIN_SPLIT
#define JG_DC_CHAIN_SPLIT 1             // probe builds: -DJG_DC_CHAIN_SPLIT=0 gives every row of a chain level to ONE wave (the A/B of DESIGN.md 3.7)
#endif
static_assert(DC_T == 4, "a step of a sweep row is one 16-byte index load and one 32-byte value load");

// ---- factorisation of the base matrix: A = Lh D^-1 U on the static pivot order, scalars ---------------------------------------------------
__global__ void k_dc_init(const int* e_src, const double* A, double* X, int n_entries) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_entries) X[e] = e_src[e] >= 0 ? A[e_src[e]] : 0.0;
}
// one dependency level: entry e -= sum Lh(i,k) U(k,j) / D(k) over its update terms (all final at lower levels)
__global__ void k_dc_fact_level(const int* f_ent, const int* t_ptr, const int* t_a, const int* t_d, const int* t_b, double* X, int i0, int i1) {
    const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= i1) return;
    const int e = f_ent[i];
    double s = X[e];
    for (int t = t_ptr[e]; t < t_ptr[e + 1]; ++t) s -= X[t_a[t]] * X[t_b[t]] / X[t_d[t]];
    X[e] = s;
}
__global__ void k_dc_dinv(const int* diag, const double* X, double* dinv, int* bad, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double d = X[diag[k]];
    if (d == 0.0 || !isfinite(d)) atomicOr(bad, 1);
    dinv[k] = 1.0 / d;
}
// the sweeps' values in list order: Lh(k,c) / D(c) below the diagonal, U(k,c) / D(k) above it; 0 for the padding of a list
__global__ void k_dc_compact(const int* ent, const int* dpiv, const double* X, const double* dinv, double* val, int terms, int n_entries) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= terms) return;
    const int e = ent[p];
    val[p] = e < n_entries ? X[e] * dinv[dpiv[p]] : 0.0;
}

// ---- sweeps on the shared factor, scenarios as lanes --------------------------------------------------------------------------------------
// share `sub` of `wpi` of row k: MODE 0 / 1 forward (y_k = r_k - sum M(k,c) y_c), MODE 2 backward (x_k = y_k / D_k - sum M(k,c) x_c)
template <int MODE>
__device__ __forceinline__ double dc_row(const DcSweepArgs& a, int k, int sub, int wpi, size_t bl) {
    const size_t ld = (size_t)a.ld;
    double acc = 0.0;
    if (sub == 0) {
        if (MODE == 2) acc = a.W[(size_t)k * ld + bl] * ((CDbl)a.dinv)[k];
        else {
            const int bus = ((CInt)a.perm)[k];
            if (MODE == 0) acc = a.rhs[(size_t)bus * ld + bl];
            else acc = (a.of[bl] == bus ? 1.0 : 0.0) - (a.ot[bl] == bus ? 1.0 : 0.0);
        }
    }
    const int p0 = ((CInt)a.ptr)[k], p1 = ((CInt)a.ptr)[k + 1];
    for (int p = p0 + DC_T * sub; p < p1; p += DC_T * wpi) {
        const I4 c = *(CI4)(a.col + p);
        const D4 v = *(CD4)(a.val + p);
        const double w0 = a.W[(size_t)c[0] * ld + bl], w1 = a.W[(size_t)c[1] * ld + bl];
        const double w2 = a.W[(size_t)c[2] * ld + bl], w3 = a.W[(size_t)c[3] * ld + bl];
        acc = fma(-v[0], w0, acc); acc = fma(-v[1], w1, acc); acc = fma(-v[2], w2, acc); acc = fma(-v[3], w3, acc);
    }
    return acc;
}
template <int MODE>
__device__ __forceinline__ void dc_store(const DcSweepArgs& a, int k, size_t bl, double acc) {
    a.W[(size_t)k * a.ld + bl] = acc;
    if (MODE == 2) a.out[(size_t)((CInt)a.perm)[k] * a.ld + bl] = acc;
}

// one wide level: a wave = one row
template <int MODE>
__global__ __launch_bounds__(256) void k_dc_sweep(DcSweepArgs a) {
    const int wave = uniform(threadIdx.y);
    const int r0 = ((CInt)a.lev)[a.l0], r1 = ((CInt)a.lev)[a.l0 + 1];
    const int item = r0 + blockIdx.x * 4 + wave;
    if (item >= r1) return;
    const int grp = a.groups ? ((CInt)a.groups)[blockIdx.y] : (int)blockIdx.y;
    const size_t bl = (size_t)grp * 64 + threadIdx.x;
    const int k = ((CInt)a.rows)[item];
    dc_store<MODE>(a, k, bl, dc_row<MODE>(a, k, 0, 1, bl));
}
// a run of narrow levels (at most DC_CHAIN_WAVES rows each): ONE workgroup per lane group walks them, a workgroup barrier between levels; the waves
// left over by a level of few rows share its rows' lists (partial sums meet in LDS, fixed order)
template <int MODE>
__global__ __launch_bounds__(64 * DC_CHAIN_WAVES) void k_dc_chain(DcSweepArgs a) {
    __shared__ double red[DC_CHAIN_WAVES * 64];
    const int wave = uniform(threadIdx.y), lane = threadIdx.x;
    const int grp = a.groups ? ((CInt)a.groups)[blockIdx.y] : (int)blockIdx.y;
    const size_t bl = (size_t)grp * 64 + lane;
    for (int l = a.l0; l < a.l1; ++l) {
        const int r0 = ((CInt)a.lev)[l], cnt = ((CInt)a.lev)[l + 1] - r0;
        int wpi = JG_DC_CHAIN_SPLIT ? DC_CHAIN_WAVES : 1;
        while (cnt * wpi > DC_CHAIN_WAVES) wpi >>= 1;               // cnt <= DC_CHAIN_WAVES: ends at wpi >= 1
        const int row = wave / wpi, sub = wave & (wpi - 1);
        const bool have = row < cnt;
        int k = 0; double acc = 0.0;
        if (have) {
            k = ((CInt)a.rows)[r0 + row];
            acc = dc_row<MODE>(a, k, sub, wpi, bl);
            if (sub != 0) red[wave * 64 + lane] = acc;
        }
        if (wpi > 1) __syncthreads();
        if (have && sub == 0) {
            for (int w = 1; w < wpi; ++w) acc += red[(wave + w) * 64 + lane];
            dc_store<MODE>(a, k, bl, acc);
        }
        __syncthreads();
    }
}

// ---- branch flows and the screen summary ---------------------------------------------------------------------------------------------------
// ISL: a lane whose outage sheds the buses with preorder numbers lo .. hi (their angles are NaN) carries 0 on every branch with an end among them
template <bool ISL>
__global__ __launch_bounds__(256) void k_dc_flows(DcFlowArgs a) {
    const int wave = uniform(threadIdx.y);
    const int chunk = blockIdx.x * 4 + wave;
    const int k0 = chunk * DC_FLOW_BRANCHES;
    if (k0 >= a.nbr) return;
    const size_t ld = (size_t)a.ld, bl = (size_t)blockIdx.y * 64 + threadIdx.x;
    const int out = a.obr[bl], out2 = a.obr2 ? a.obr2[bl] : -1;
    int lo = 1, hi = 0;
    if (ISL) { const I4 q = a.isl[bl]; lo = q[1]; hi = q[2]; }
    double wl = 0.0, wf = 0.0, il = 0.0, jf = 0.0;
    for (int k = k0; k < min(k0 + DC_FLOW_BRANCHES, a.nbr); ++k) {
        const int f = ((CInt)a.bf)[k], t = ((CInt)a.bt)[k];
        const double y = ((CDbl)a.by)[k], s = ((CDbl)a.bs)[k];
        double p = y * (a.TH[(size_t)f * ld + bl] - a.TH[(size_t)t * ld + bl] - s);
        if (k == out || k == out2) p = 0.0;
        if (ISL) {
            const int pf = ((CInt)a.preorder)[f], pt = ((CInt)a.preorder)[t];
            if ((pf >= lo && pf <= hi) || (pt >= lo && pt <= hi)) p = 0.0;
        }
        if (a.flows) a.flows[(size_t)k * ld + bl] = p;
        const double m = fabs(p);
        if (m > wf) { wf = m; jf = (double)(k + 1); }
        if (a.rating) {
            const double r = ((CDbl)a.rating)[k];
            if (r > 0.0 && m / r > wl) { wl = m / r; il = (double)(k + 1); }
        }
    }
    double* q = a.part + (size_t)chunk * 4 * ld + bl;
    q[0] = wl; q[ld] = il; q[2 * ld] = wf; q[3 * ld] = jf;
}

template <int MODE>
void launch_sweep(const DcFactor& F, hipStream_t stream, const DcSweepTables& T, DcSweepArgs a, int groups) {
    a.rows = T.rows; a.lev = T.lev; a.ptr = T.ptr; a.col = T.col; a.val = T.val; a.perm = F.perm; a.dinv = F.dinv;
    for (const auto& L : T.launches) {
        a.l0 = L.l0; a.l1 = L.l1;
        if (L.chain) hipLaunchKernelGGL((k_dc_chain<MODE>), dim3(1, groups), dim3(64, DC_CHAIN_WAVES), 0, stream, a);
        else {
            const int cnt = T.h_lev[L.l0 + 1] - T.h_lev[L.l0];
            hipLaunchKernelGGL((k_dc_sweep<MODE>), dim3((cnt + 3) / 4, groups), dim3(64, 4), 0, stream, a);
        }
    }
}

}  // namespace

void compact_sweep(const DcFactor& F, const DcSweepTables& T, hipStream_t stream) {
    if (T.terms) hipLaunchKernelGGL(k_dc_compact, dim3((unsigned)((T.terms + 255) / 256)), dim3(256), 0, stream, T.ent, T.dpiv, F.X, F.dinv, T.val, (int)T.terms, F.n_entries);
}

int build_sweep(DcDevice* h, const DcFactor& F, DcSweepTables& T, const std::vector<int>& level, const std::vector<int>& lptr, const std::vector<int>& lent,
                const std::vector<int>& lcol, bool upper, bool keep) {
    const int n = F.n;
    int nlev = 0;
    for (int k = 0; k < n; ++k) nlev = std::max(nlev, level[k]);
    T.h_lev.assign(nlev + 1, 0);
    for (int k = 0; k < n; ++k) T.h_lev[level[k]]++;                 // level is 1-based
    for (int l = 0; l < nlev; ++l) T.h_lev[l + 1] += T.h_lev[l];
    std::vector<int> rows(n), fill(T.h_lev.begin(), T.h_lev.end() - 1);
    for (int k = 0; k < n; ++k) rows[fill[level[k] - 1]++] = k;
    std::vector<int> ptr(n + 1, 0);
    for (int k = 0; k < n; ++k) ptr[k + 1] = ptr[k] + (lptr[k + 1] - lptr[k] + DC_T - 1) / DC_T * DC_T;
    T.terms = ptr[n];
    std::vector<int> col(ptr[n], n), ent(ptr[n], F.n_entries), dpiv(ptr[n], 0);
    for (int k = 0; k < n; ++k)
        for (int p = lptr[k], q = ptr[k]; p < lptr[k + 1]; ++p, ++q) { col[q] = lcol[p]; ent[q] = lent[p]; dpiv[q] = upper ? k : lcol[p]; }
    DC_TRY(dev_alloc(h, &T.rows, (size_t)n, rows.data()));
    DC_TRY(dev_alloc(h, &T.lev, T.h_lev.size(), T.h_lev.data()));
    DC_TRY(dev_alloc(h, &T.ptr, (size_t)n + 1, ptr.data()));
    DC_TRY(dev_alloc(h, &T.col, col.size(), col.data()));
    DC_TRY(dev_alloc(h, &T.ent, ent.size(), ent.data()));
    DC_TRY(dev_alloc(h, &T.dpiv, dpiv.size(), dpiv.data()));
    DC_TRY(dev_alloc(h, &T.val, col.size(), (const double*)nullptr, true));
    compact_sweep(F, T, h->stream);
    DC_HIP(hipGetLastError());
    DC_HIP(hipStreamSynchronize(h->stream));
    if (!keep) { dev_release(h, T.ent); dev_release(h, T.dpiv); }
    T.launches.clear();
    for (int l = 0; l < nlev;) {
        const bool narrow = T.h_lev[l + 1] - T.h_lev[l] <= DC_CHAIN_WAVES;
        int e = l + 1;
        if (narrow) while (e < nlev && T.h_lev[e + 1] - T.h_lev[e] <= DC_CHAIN_WAVES) ++e;
        T.launches.push_back({l, e, narrow ? 1 : 0});
        l = e;
    }
    return 0;
}

void sweep_pair(const DcFactor& F, hipStream_t stream, int mode_f, const double* rhs, const int* of, const int* ot, double* W, double* out, int ld, int groups,
                const int* glist) {
    DcSweepArgs a{};
    a.rhs = rhs; a.of = of; a.ot = ot; a.W = W; a.out = out; a.groups = glist; a.ld = ld;
    if (mode_f == 0) launch_sweep<0>(F, stream, F.fwd, a, groups);
    else launch_sweep<1>(F, stream, F.fwd, a, groups);
    launch_sweep<2>(F, stream, F.bwd, a, groups);
}

void launch_dc_flows(const DcFlowArgs& a, bool isl, dim3 grid, hipStream_t stream) {
    if (isl) hipLaunchKernelGGL(k_dc_flows<true>, grid, dim3(64, 4), 0, stream, a);
    else hipLaunchKernelGGL(k_dc_flows<false>, grid, dim3(64, 4), 0, stream, a);
}

int factor_tables(DcDevice* h, DcFactor& F, int n, const BlockSymbolic& S) {
    F.n = n;
    F.n_entries = S.n_entries;
    int nlev = 0;
    for (int e = 0; e < S.n_entries; ++e) nlev = std::max(nlev, S.e_level[e]);
    F.n_fact_levels = nlev;
    F.f_lev.assign(nlev + 2, 0);
    for (int e = 0; e < S.n_entries; ++e) F.f_lev[S.e_level[e] + 1]++;
    for (int l = 0; l <= nlev; ++l) F.f_lev[l + 1] += F.f_lev[l];
    std::vector<int> f_ent(S.n_entries), fill(F.f_lev.begin(), F.f_lev.end() - 1);
    for (int e = 0; e < S.n_entries; ++e) f_ent[fill[S.e_level[e]]++] = e;
    DC_TRY(dev_alloc(h, &F.perm, (size_t)n, S.perm.data()));
    DC_TRY(dev_alloc(h, &F.f_ent, f_ent.size(), f_ent.data()));
    DC_TRY(dev_alloc(h, &F.t_ptr, S.t_ptr.size(), S.t_ptr.data()));
    DC_TRY(dev_alloc(h, &F.t_a, S.t_a.size(), S.t_a.data()));
    DC_TRY(dev_alloc(h, &F.t_d, S.t_d.size(), S.t_d.data()));
    DC_TRY(dev_alloc(h, &F.t_b, S.t_b.size(), S.t_b.data()));
    DC_TRY(dev_alloc(h, &F.e_src, S.e_src.size(), S.e_src.data()));
    DC_TRY(dev_alloc(h, &F.diag, (size_t)n, S.diag.data()));
    return 0;
}
void factor_numeric(const DcFactor& F, hipStream_t stream) {
    hipLaunchKernelGGL(k_dc_init, dim3((F.n_entries + 255) / 256), dim3(256), 0, stream, F.e_src, F.A, F.X, F.n_entries);
    for (int l = 0; l <= F.n_fact_levels; ++l) {
        const int i0 = F.f_lev[l], i1 = F.f_lev[l + 1];
        if (i1 > i0) hipLaunchKernelGGL(k_dc_fact_level, dim3((i1 - i0 + 255) / 256), dim3(256), 0, stream, F.f_ent, F.t_ptr, F.t_a, F.t_d, F.t_b, F.X, i0, i1);
    }
    hipLaunchKernelGGL(k_dc_dinv, dim3((F.n + 255) / 256), dim3(256), 0, stream, F.diag, F.X, F.dinv, F.bad, F.n);
}
std::vector<int> forward_levels(int n, const BlockSymbolic& S) {
    std::vector<int> flev(n, 1);
    for (int r = 0; r < n; ++r)
        for (int p = S.l_ptr[r]; p < S.l_ptr[r + 1]; ++p) flev[r] = std::max(flev[r], flev[S.l_col[p]] + 1);
    return flev;
}

}  // namespace jg
