// jg_dc_lanefactor.hip -- the lane-valued scalar factorisation and its sweeps (jg_dc_lanefactor.hpp declares them and says what is held where).  The
// symbolic side is jg_dc_sweep.hip's; the kernels here are its factorisation and sweep kernels with every VALUE read per lane.
#include "jg_dc_lanefactor.hpp"

namespace jg {

namespace {

// ---- factorisation: a wavefront = one entry x 64 lanes ----------------------------------------------------------------------------------------
struct LaneFactArgs {
    const int* f_ent; const int* t_ptr; const int* t_a; const int* t_d; const int* t_b; const int* e_src; const int* diag;
    const double* A; double* X; double* dinv; int* bad;
    const int* groups;
    int ld, i0, i1;
};
// X = the matrix's entries, 0 on fill; i1 = n_entries
__global__ __launch_bounds__(256) void k_lf_init(LaneFactArgs a) {
    const int e = blockIdx.x * 4 + uniform(threadIdx.y);
    if (e >= a.i1) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    const int src = ((CInt)a.e_src)[e];
    a.X[(size_t)e * ld + bl] = src >= 0 ? a.A[(size_t)src * ld + bl] : 0.0;
    if (e == 0) a.bad[bl] = 0;
}
// one dependency level: entry e -= sum Lh(i,k) U(k,j) / D(k) over its update terms (all final at lower levels)
__global__ __launch_bounds__(256) void k_lf_level(LaneFactArgs a) {
    const int i = a.i0 + blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.i1) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    const int e = ((CInt)a.f_ent)[i];
    const int t0 = ((CInt)a.t_ptr)[e], t1 = ((CInt)a.t_ptr)[e + 1];
    if (t0 == t1) return;
    double s = a.X[(size_t)e * ld + bl];
    for (int t = t0; t < t1; ++t) {
        const int ta = ((CInt)a.t_a)[t], tb = ((CInt)a.t_b)[t], td = ((CInt)a.t_d)[t];
        s -= a.X[(size_t)ta * ld + bl] * a.X[(size_t)tb * ld + bl] / a.X[(size_t)td * ld + bl];
    }
    a.X[(size_t)e * ld + bl] = s;
}
// i1 = n; a lane with a bad pivot writes its own flag (every writer stores the same 1)
__global__ __launch_bounds__(256) void k_lf_dinv(LaneFactArgs a) {
    const int k = blockIdx.x * 4 + uniform(threadIdx.y);
    if (k >= a.i1) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(a.groups);
    const double d = a.X[(size_t)((CInt)a.diag)[k] * ld + bl];
    if (dc_bad_pivot(d)) a.bad[bl] = 1;
    a.dinv[(size_t)k * ld + bl] = 1.0 / d;
}

// ---- sweeps: a wavefront = one row x 64 lanes, the factor value of a term is X[ent] * dinv[dpiv] of the lane -------------------------------------
struct LaneSweepArgs {
    const int* rows; const int* lev; const int* ptr; const int* col; const int* ent; const int* dpiv; const int* perm;
    const double* X; const double* dinv;
    const double* rhs;                  // forward: [n][ld], the matrix's own order
    double* W;                          // [n + 1][ld], pivot order; row n stays zero
    double* out;                        // backward: [n][ld], the matrix's own order
    const int* groups;
    int ld, l0, l1;
};
// share `sub` of `wpi` of row k: forward y_k = r_k - sum M(k,c) y_c, backward x_k = y_k / D_k - sum M(k,c) x_c
template <bool BWD>
__device__ __forceinline__ double lane_row(const LaneSweepArgs& a, int k, int sub, int wpi, size_t bl) {
    const size_t ld = (size_t)a.ld;
    double acc = 0.0;
    if (sub == 0) {
        if (BWD) acc = a.W[(size_t)k * ld + bl] * a.dinv[(size_t)k * ld + bl];
        else acc = a.rhs[(size_t)((CInt)a.perm)[k] * ld + bl];
    }
    const int p0 = ((CInt)a.ptr)[k], p1 = ((CInt)a.ptr)[k + 1];
    for (int p = p0 + DC_T * sub; p < p1; p += DC_T * wpi) {
        const I4 c = *(CI4)(a.col + p), e = *(CI4)(a.ent + p), d = *(CI4)(a.dpiv + p);
#pragma unroll
        for (int q = 0; q < DC_T; ++q) {
            const double v = a.X[(size_t)e[q] * ld + bl] * a.dinv[(size_t)d[q] * ld + bl];
            acc = fma(-v, a.W[(size_t)c[q] * ld + bl], acc);
        }
    }
    return acc;
}
template <bool BWD>
__device__ __forceinline__ void lane_store(const LaneSweepArgs& a, int k, size_t bl, double acc) {
    a.W[(size_t)k * a.ld + bl] = acc;
    if (BWD) a.out[(size_t)((CInt)a.perm)[k] * a.ld + bl] = acc;
}
template <bool BWD>
__global__ __launch_bounds__(256) void k_lf_sweep(LaneSweepArgs a) {
    const int wave = uniform(threadIdx.y);
    const int r0 = ((CInt)a.lev)[a.l0], r1 = ((CInt)a.lev)[a.l0 + 1];
    const int item = r0 + blockIdx.x * 4 + wave;
    if (item >= r1) return;
    const size_t bl = lane_of(a.groups);
    const int k = ((CInt)a.rows)[item];
    lane_store<BWD>(a, k, bl, lane_row<BWD>(a, k, 0, 1, bl));
}
// a run of narrow levels: ONE workgroup per lane group walks them, a workgroup barrier between levels; the waves a level of few rows leaves over share
// its rows' lists (partial sums meet in LDS, fixed order) -- k_dc_chain of jg_dc_sweep.hip with lane values
template <bool BWD>
__global__ __launch_bounds__(64 * DC_CHAIN_WAVES) void k_lf_chain(LaneSweepArgs a) {
    __shared__ double red[DC_CHAIN_WAVES * 64];
    const int wave = uniform(threadIdx.y), lane = threadIdx.x;
    const size_t bl = lane_of(a.groups);
    for (int l = a.l0; l < a.l1; ++l) {
        const int r0 = ((CInt)a.lev)[l], cnt = ((CInt)a.lev)[l + 1] - r0;
        int wpi = DC_CHAIN_WAVES;
        while (cnt * wpi > DC_CHAIN_WAVES) wpi >>= 1;               // cnt <= DC_CHAIN_WAVES: ends at wpi >= 1
        const int row = wave / wpi, sub = wave & (wpi - 1);
        const bool have = row < cnt;
        int k = 0; double acc = 0.0;
        if (have) {
            k = ((CInt)a.rows)[r0 + row];
            acc = lane_row<BWD>(a, k, sub, wpi, bl);
            if (sub != 0) red[wave * 64 + lane] = acc;
        }
        if (wpi > 1) __syncthreads();
        if (have && sub == 0) {
            for (int w = 1; w < wpi; ++w) acc += red[(wave + w) * 64 + lane];
            lane_store<BWD>(a, k, bl, acc);
        }
        __syncthreads();
    }
}

template <bool BWD>
void launch_lane_sweep(const DcLaneFactor& F, hipStream_t stream, const DcSweepTables& T, LaneSweepArgs a, int groups) {
    a.rows = T.rows; a.lev = T.lev; a.ptr = T.ptr; a.col = T.col; a.ent = T.ent; a.dpiv = T.dpiv; a.perm = F.sym.perm; a.X = F.X; a.dinv = F.dinv; a.ld = F.ld;
    for (const auto& L : T.launches) {
        a.l0 = L.l0; a.l1 = L.l1;
        if (L.chain) hipLaunchKernelGGL((k_lf_chain<BWD>), dim3(1, groups), dim3(64, DC_CHAIN_WAVES), 0, stream, a);
        else {
            const int cnt = T.h_lev[L.l0 + 1] - T.h_lev[L.l0];
            hipLaunchKernelGGL((k_lf_sweep<BWD>), dim3((cnt + 3) / 4, groups), dim3(64, 4), 0, stream, a);
        }
    }
}

}  // namespace

int lane_factor_create(DcDevice* h, DcLaneFactor& F, int n, int nnz, const BlockSymbolic& S, int ld) {
    DcFactor& Y = F.sym;
    F.ld = ld; F.nnz = nnz;
    DC_TRY(factor_tables(h, Y, n, S));
    // build_sweep fills its premultiplied list values from Y.X and Y.dinv: one lane of zeros serves it and leaves again
    DC_TRY(dev_alloc(h, &Y.X, (size_t)S.n_entries + 1, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &Y.dinv, (size_t)n, (const double*)nullptr, true));
    DC_TRY(build_sweep(h, Y, Y.fwd, forward_levels(n, S), S.l_ptr, S.l_ent, S.l_col, false, true));
    DC_TRY(build_sweep(h, Y, Y.bwd, S.bwd_level, S.u_ptr, S.u_ent, S.u_col, true, true));
    dev_release(h, Y.X); dev_release(h, Y.dinv);
    dev_release(h, Y.fwd.val); dev_release(h, Y.bwd.val);
    const size_t l = (size_t)ld;
    DC_TRY(dev_alloc(h, &F.A, (size_t)nnz * l, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.X, ((size_t)S.n_entries + 1) * l, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.dinv, (size_t)n * l, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.bad, l, (const int*)nullptr, true));
    return 0;
}

void lane_factor_numeric(const DcLaneFactor& F, hipStream_t stream, int groups, const int* glist) {
    const DcFactor& Y = F.sym;
    LaneFactArgs a{Y.f_ent, Y.t_ptr, Y.t_a, Y.t_d, Y.t_b, Y.e_src, Y.diag, F.A, F.X, F.dinv, F.bad, glist, F.ld, 0, Y.n_entries};
    hipLaunchKernelGGL(k_lf_init, dim3((Y.n_entries + 3) / 4, groups), dim3(64, 4), 0, stream, a);
    for (int l = 0; l <= Y.n_fact_levels; ++l) {                     // (an entry without update terms is final after k_lf_init: its wave leaves at once)
        a.i0 = Y.f_lev[l]; a.i1 = Y.f_lev[l + 1];
        if (a.i1 > a.i0) hipLaunchKernelGGL(k_lf_level, dim3((a.i1 - a.i0 + 3) / 4, groups), dim3(64, 4), 0, stream, a);
    }
    a.i0 = 0; a.i1 = Y.n;
    hipLaunchKernelGGL(k_lf_dinv, dim3((Y.n + 3) / 4, groups), dim3(64, 4), 0, stream, a);
}

void lane_sweep_pair(const DcLaneFactor& F, hipStream_t stream, const double* rhs, double* W, double* out, int groups, const int* glist) {
    LaneSweepArgs a{};
    a.rhs = rhs; a.W = W; a.out = out; a.groups = glist;
    launch_lane_sweep<false>(F, stream, F.sym.fwd, a, groups);
    launch_lane_sweep<true>(F, stream, F.sym.bwd, a, groups);
}

}  // namespace jg
