// jg_dc_series.hip -- the DC N-1 screen over a series of injection profiles (jg_dc_series.hpp has the algebra and the reference loop it stands for).
//
// Build: Phi by the build the three screens share (dc_phi_build, jg_dc_phi.hip), into a state of the series' own; then F0, the row flows of the profiles'
// right-hand sides (dc_phi_row_flows: the sweep pair of jg_dc_sweep.hip, DC_PAIR_LANES profiles at a time).  Screen of a row block [k0, k1):
// k_series_screen walks the rows once (a wave = DC_SERIES_TILE candidates k in registers x 64 consecutive profiles; Phi[m, k..], 1 / rating_m and the
// row's candidate position through scalar loads, F0[m, t..t+63] one coalesced vector load reused for every k of the tile; nothing is written per m); the
// records come out of the block's dense result by k_dc_rows and dc_block_records (jg_dc_records.hpp has the protocol) under the policy SeriesRows, sorted
// by (k, t).  Every store is a vector store.
#include "jg_dc_series.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/jgrid.h"

namespace jg {

namespace {

// ---- the screen kernel -------------------------------------------------------------------------------------------------------------------
struct SeriesScreenArgs {
    const double* Phi; const double* F0; const double* rinv; const int* pos; const int* rbranch;
    const int* crow; const double* cdiag;
    double* load; int* branch; int* count;                      // [k1 - k0][ldt]
    double thr; int rows, ldk, ldt, T, k0, k1, kbase;           // kbase: k0 rounded down to a multiple of the tile (the scalar loads of a tile are 32-byte aligned)
    const int* cisl; const int* rpre;                            // SHED: the candidates' (side, lo, hi, 0) and the rows' preorder[from]
};
// SHED (a screen built in shed mode): a bridge candidate's column of Phi holds Z[:,k], its coefficient is s_k F0[k,t] without a denominator, and a row whose
// from end lies in its preorder interval left with it and carries 0.  The interval and the row's number are wave-uniform: scalar loads, scalar compares.
template <bool SHED>
__global__ __launch_bounds__(64 * DC_PAIR_WAVES) void k_series_screen(SeriesScreenArgs a) {
    constexpr int K = DC_SERIES_TILE;
    const int wave = uniform(threadIdx.y);
    const int kt = a.kbase + (blockIdx.y * DC_PAIR_WAVES + wave) * K;
    if (kt >= a.k1) return;
    const int t = blockIdx.x * 64 + threadIdx.x;                // < ldt: F0 is [rows][ldt], 0 behind T
    const size_t ldk = (size_t)a.ldk, ldt = (size_t)a.ldt;
    const double* fcol = a.F0 + t;
    double c[K], wl[K];
    int il[K], cnt[K];
    bool sing[K];
    int lo[K], hi[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int k = kt + i;                                    // < ldk: the per-candidate arrays are [ldk], 0 behind nk
        const double dk = 1.0 - ((CDbl)a.cdiag)[k];
        const int rk = ((CInt)a.crow)[k];
        sing[i] = fabs(dk) < DC_SINGULAR;
        c[i] = sing[i] ? 0.0 : fcol[(size_t)rk * ldt] / dk;
        wl[i] = 0.0; il[i] = -1; cnt[i] = 0;
        lo[i] = 1; hi[i] = 0;
        if constexpr (SHED) {
            const I4 q = ((CI4)a.cisl)[k];
            lo[i] = q[1]; hi[i] = q[2];
            if (q[0] != 0) { sing[i] = false; c[i] = (q[0] > 0 ? 1.0 : -1.0) * fcol[(size_t)rk * ldt]; }     // what left m over the bridge before the outage
        }
    }
    const double thr = a.thr;
    auto row = [&](int r, int pk, auto hit_c) {
        constexpr bool HIT = decltype(hit_c)::value;
        const double ri = ((CDbl)a.rinv)[r];
        const double* prow = a.Phi + (size_t)r * ldk;
        double pt[K];
        const D4 q0 = *(CD4)(prow + kt);
        pt[0] = q0[0]; pt[1] = q0[1]; pt[2] = q0[2]; pt[3] = q0[3];
        if constexpr (K == 8) {
            const D4 q1 = *(CD4)(prow + kt + 4);
            pt[4] = q1[0]; pt[5] = q1[1]; pt[6] = q1[2]; pt[7] = q1[3];
        }
        const double f = fcol[(size_t)r * ldt];
        int pr = 0;
        if constexpr (SHED) pr = ((CInt)a.rpre)[r];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double v = fma(pt[i], c[i], f);
            if (HIT && pk == kt + i) v = 0.0;                    // the outaged branch carries nothing
            if (SHED && pr >= lo[i] && pr <= hi[i]) v = 0.0;     // nor does a branch that left with the bridge
            const double ld = fabs(v) * ri;
            if (ld > wl[i]) { wl[i] = ld; il[i] = r; }           // rows ascend by branch index, strict comparison: ties go to the lowest branch (k_dc_flows)
            cnt[i] += ld > thr ? 1 : 0;
        }
    };
    for (int r = 0; r < a.rows; ++r) {
        const int pk = ((CInt)a.pos)[r];
        // only a row whose branch is one of this wave's own candidates (at most K of the rows) needs the test
        if ((unsigned)(pk - kt) < (unsigned)K) row(r, pk, std::true_type{});
        else row(r, pk, std::false_type{});
    }
    if (t >= a.T) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int k = kt + i;
        if (k < a.k0 || k >= a.k1) continue;
        const size_t o = (size_t)(k - a.k0) * ldt + t;
        a.load[o] = sing[i] ? nan : wl[i];
        a.branch[o] = (sing[i] || il[i] < 0) ? 0 : a.rbranch[il[i]] + 1;
        a.count[o] = sing[i] ? 0 : cnt[i];
    }
}

// ---- summaries out of the block's dense result: the series' policy of k_dc_rows (jg_dc_records.hpp) ------------------------------------------------
// Row k's columns are the profiles 0 .. T; one list, the violators v > thr (a NaN, the loading of a bridge candidate, compares false); the row's maximum from 0.
struct SeriesRows {
    static constexpr int LISTS = 1;
    const double* load; const int* branch; const int* count; const int* clabel;
    DcRecords list[1]; double* r_red;
    double thr; int ldt, T, k0, k1;
    __device__ int first(int) const { return 0; }
    __device__ int cols() const { return T; }
    __device__ bool valid(int, int t) const { return t < T; }
    __device__ double value(int i, int t) const { return load[(size_t)i * ldt + t]; }
    __device__ bool hit(int, double v, int) const { return v > thr; }
    __device__ void write(int, long long at, int klab, int i, int, int t, double v) const {
        double* e = (double*)list[0].rec + at * 5;
        e[0] = (double)klab; e[1] = (double)t; e[2] = (double)branch[(size_t)i * ldt + t]; e[3] = v; e[4] = (double)count[(size_t)i * ldt + t];
    }
    static __device__ double identity() { return 0.0; }
    static __device__ bool better(double v, double m) { return v > m; }
    static __device__ double combine(double x, double y) { return fmax(x, y); }
};
// per profile over the block's candidates: the worst loading (bridges aside) and the number of candidates whose outage violates
__global__ void k_series_cols(const double* load, double* c_max, int* c_viol, double thr, int ldt, int T, int rb) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ldt) return;
    double mx = 0.0;
    int nv = 0;
    if (t < T)
        for (int i = 0; i < rb; ++i) {
            const double v = load[(size_t)i * ldt + t];
            if (v > mx) mx = v;
            nv += v > thr ? 1 : 0;
        }
    c_max[t] = mx; c_viol[t] = nv;
}
// the base case of every profile (no outage): worst loading, its branch (1-based, 0: none), branches above the threshold
__global__ void k_series_base(const double* F0, const double* rinv, const int* rbranch, double* base, double thr, int rows, int ldt, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    double wl = 0.0;
    int il = -1, cnt = 0;
    for (int r = 0; r < rows; ++r) {
        const double ld = fabs(F0[(size_t)r * ldt + t]) * ((CDbl)rinv)[r];
        if (ld > wl) { wl = ld; il = r; }
        cnt += ld > thr ? 1 : 0;
    }
    double* q = base + (size_t)t * 3;
    q[0] = wl; q[1] = il < 0 ? 0.0 : (double)(rbranch[il] + 1); q[2] = (double)cnt;
}

// rhs [T][n]: the lane right-hand sides as jg_dc_set_injections takes them
int series_build(DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, int T, const double* rhs, int64_t budget, double* info) {
    dc_state_release(h, h->series);
    const bool shed = h->series_shed == 1;
    h->series_shed = 0;
    const int ldt = (T + 63) / 64 * 64;
    const int nr = (int)dc_phi_row_labels(h, cand, mon, ldt, info).size();
    const size_t f0_bytes = (size_t)info[8], scratch = dc_phi_flows_scratch(h, ldt);
    DcSeriesState* s = h->series = new DcSeriesState();
    s->T = T; s->ldt = ldt;
    const std::string extra = "; F0 needs " + dc_bytes_text(f0_bytes) + " (" + std::to_string(nr) + " rows x " + std::to_string(ldt) + " profiles x 8) and " +
                              dc_bytes_text(scratch) + " of scratch";
    int rc = 0;
    auto step = [&](int r) { if (r && !rc) rc = r; return rc == 0; };
    double ms[2] = {0.0, 0.0};
    step(dc_phi_build(h, &s->phi, "jg_dc_series_build", cand, mon, budget, f0_bytes + scratch, extra, info, shed)) &&
        step(dev_alloc(h, s->mem, &s->F0, (size_t)nr * ldt, (const double*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->c_max, (size_t)ldt, (const double*)nullptr, true)) &&
        step(dev_alloc(h, s->mem, &s->c_viol, (size_t)ldt, (const int*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->base, (size_t)ldt * 3, (const double*)nullptr, true)) &&
        step(dc_phi_row_flows(h, &s->phi, T, rhs, true, s->F0, ldt, ms)) && step(dc_phi_bridges(h, &s->phi, s->h_bridge));
    if (rc) return dc_build_failed(h, h->series, rc);
    dc_phi_flows_ms(ms, s->build_ms, info);
    return 0;
}

// the block's buffers for `rb` rows; grown, never shrunk
int series_block(DcHandle* h, int rb, long long rec_cap) {
    DcSeriesState* s = h->series;
    if (rb > s->blk_rows) {
        const size_t cells = (size_t)rb * s->ldt, r = (size_t)rb;
        DC_TRY(dc_block_grow(h, s->mem, "jg_dc_series_screen", rb, s->blk_rows, cells * 16, {&s->viol}, dc_blk(s->b_load, cells), dc_blk(s->b_branch, cells), dc_blk(s->b_count, cells),
                             dc_blk(s->r_max, r)));
    }
    return dc_list_grow(h, s->mem, s->viol, rec_cap);
}

SeriesScreenArgs screen_args(const DcSeriesBlock& b, int k0, int k1, double thr) {
    const DcPhi* p = b.phi;
    SeriesScreenArgs a{};
    a.Phi = p->Phi; a.F0 = b.F0; a.rinv = p->row_rinv; a.pos = p->row_pos; a.rbranch = p->row_branch; a.crow = p->cand_row; a.cdiag = p->cand_diag;
    a.load = b.load; a.branch = b.branch; a.count = b.count;
    a.thr = thr; a.rows = p->rows; a.ldk = p->ldk; a.ldt = b.ldt; a.T = b.T; a.k0 = k0; a.k1 = k1; a.kbase = k0 / DC_SERIES_TILE * DC_SERIES_TILE;
    a.cisl = p->shed ? p->cand_isl : nullptr; a.rpre = p->shed ? p->row_pre : nullptr;
    return a;
}
DcSeriesBlock series_blk(DcHandle* h) {
    DcSeriesState* s = h->series;
    return DcSeriesBlock{&s->phi, s->F0, s->ldt, s->T, s->b_load, s->b_branch, s->b_count};
}
void launch_screen(DcHandle* h, const SeriesScreenArgs& a) {
    const int tiles = (a.k1 - a.kbase + DC_SERIES_TILE - 1) / DC_SERIES_TILE;
    const dim3 grid(a.ldt / 64, (tiles + DC_PAIR_WAVES - 1) / DC_PAIR_WAVES), block(64, DC_PAIR_WAVES);
    if (a.cisl) hipLaunchKernelGGL(k_series_screen<true>, grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL(k_series_screen<false>, grid, block, 0, h->stream, a);
}
SeriesRows list_args(DcHandle* h, int k0, int k1, double thr, long long rec_cap) {
    DcSeriesState* s = h->series;
    SeriesRows a{};
    a.load = s->b_load; a.branch = s->b_branch; a.count = s->b_count; a.clabel = s->phi.cand_label;
    a.list[0] = s->viol.limited(rec_cap); a.r_red = s->r_max;
    a.thr = thr; a.ldt = s->ldt; a.T = s->T; a.k0 = k0; a.k1 = k1;
    return a;
}
void launch_stats(DcHandle* h, const SeriesRows& a) {
    DcSeriesState* s = h->series;
    dc_launch_rows<false>(h, a);
    dc_series_launch_cols(h, series_blk(h), s->c_max, s->c_viol, a.thr, a.k1 - a.k0);
}

struct SeriesOut {
    double* records; int64_t* islanding; int64_t* totals; double* worst; double* worst_profile; int64_t* viol_profile; double* base;
    double* d_load; int32_t* d_branch; int32_t* d_count;
};
int series_screen(DcHandle* h, int k0, int k1, double thr, long long rec_cap, const SeriesOut& o) {
    DcSeriesState* s = h->series;
    DcPhi* p = &s->phi;
    const int rb = k1 - k0, T = s->T, ldt = s->ldt;
    DC_TRY(series_block(h, rb, rec_cap));
    dc_phi_rinv(h, p);
    launch_screen(h, screen_args(series_blk(h), k0, k1, thr));
    const SeriesRows la = list_args(h, k0, k1, thr, rec_cap);
    launch_stats(h, la);
    if (o.base) dc_series_launch_base(h, series_blk(h), s->base, thr);
    std::vector<int> cviol(ldt);
    std::vector<double> rmax(rb), cmax(ldt);
    DcListCall viol{&s->viol, rec_cap, o.records};
    DC_TRY(dc_block_records(h, rb, {&viol}, [&] {
        DC_HIP(hipMemcpyAsync(rmax.data(), s->r_max, rb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(hipMemcpyAsync(cviol.data(), s->c_viol, ldt * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (o.base) DC_HIP(hipMemcpyAsync(o.base, s->base, (size_t)T * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(sync_copy(cmax.data(), s->c_max, ldt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        return 0;
    }, [&] { dc_launch_rows<true>(h, la); }));
    o.totals[0] = (long long)rb * T; o.totals[1] = viol.total; o.totals[2] = dc_bridge_list(*p, s->h_bridge, k0, k1, o.islanding); o.totals[3] = viol.kept;
    o.totals[4] = viol.total > rec_cap ? 1 : 0;
    if (o.worst) for (int i = 0; i < rb; ++i) o.worst[k0 + i] = rmax[i];
    if (o.worst_profile) for (int t = 0; t < T; ++t) o.worst_profile[t] = std::max(o.worst_profile[t], cmax[t]);
    if (o.viol_profile) for (int t = 0; t < T; ++t) o.viol_profile[t] += cviol[t];
    auto same = [](int, int, auto v) { return v; };
    if (o.d_load) DC_TRY(dc_dense(h, o.d_load, (const double*)s->b_load, rb, ldt, T, same));
    if (o.d_branch) DC_TRY(dc_dense(h, o.d_branch, (const int*)s->b_branch, rb, ldt, T, same));
    if (o.d_count) DC_TRY(dc_dense(h, o.d_count, (const int*)s->b_count, rb, ldt, T, same));
    return 0;
}

}  // namespace

void dc_series_free(DcHandle* h) { dc_state_release(h, h->series); }

void dc_series_launch_screen(DcHandle* h, const DcSeriesBlock& b, int k0, int k1, double thr) { launch_screen(h, screen_args(b, k0, k1, thr)); }
void dc_series_launch_cols(DcHandle* h, const DcSeriesBlock& b, double* c_max, int* c_viol, double thr, int rb) {
    hipLaunchKernelGGL(k_series_cols, dim3((b.ldt + 255) / 256), dim3(256), 0, h->stream, b.load, c_max, c_viol, thr, b.ldt, b.T, rb);
}
void dc_series_launch_base(DcHandle* h, const DcSeriesBlock& b, double* base, double thr) {
    hipLaunchKernelGGL(k_series_base, dim3((b.T + 63) / 64), dim3(64), 0, h->stream, b.F0, b.phi->row_rinv, b.phi->row_branch, base, thr, b.phi->rows, b.ldt, b.T);
}

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_series_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t profiles, const double* rhs,
                       int64_t budget_bytes, double* info) {
    DC_ENTER(h);
    if (!d->nbr) return api_fail(1, "jg_dc_series_build: jg_dc_set_branches first");
    if (d->h_rhs.empty()) return api_fail(1, "jg_dc_series_build: jg_dc_set_rhs first");
    if (nk < 1 || !candidates || !info || nm < 0 || (nm && !monitored)) return api_fail(1, "jg_dc_series_build: one or more candidates, and info, are needed");
    if (profiles < 1 || profiles > (1 << 24) || !rhs) return api_fail(1, "jg_dc_series_build: one or more profiles are needed");
    std::vector<int> cand, mon;
    DC_RET(jg::dc_phi_lists(d, "jg_dc_series_build", nk, candidates, nm, monitored, cand, mon));
    DC_RET(jg::series_build(d, cand, mon, (int)profiles, rhs, budget_bytes, info));
    return 0;
}

int jg_dc_series_screen(int64_t h, int64_t k0, int64_t k1, double threshold, int64_t capacity, double* records, int64_t* islanding, int64_t* totals,
                        double* worst, double* worst_profile, int64_t* violating_profile, double* base, double* dense_load, int32_t* dense_branch,
                        int32_t* dense_count) {
    DC_ENTER(h);
    if (!d->series) return api_fail(4, "jg_dc_series_screen: jg_dc_series_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_series_screen: jg_dc_set_rating first (the loadings are |from| / rating)");
    if (k0 < 0 || k1 <= k0 || k1 > d->series->phi.nk) return api_fail(1, "jg_dc_series_screen: rows [k0, k1) out of range");
    if (!(threshold >= 0.0) || capacity < 0 || (capacity && !records) || !totals) return api_fail(1, "jg_dc_series_screen: bad argument");
    jg::SeriesOut o{records, islanding, totals, worst, worst_profile, violating_profile, base, dense_load, dense_branch, dense_count};
    DC_RET(jg::series_screen(d, (int)k0, (int)k1, threshold, capacity, o));
    return 0;
}

int jg_dc_series_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms) {
    DC_ENTER(h);
    jg::DcSeriesState* s = d->series;
    return jg::dc_phi_time_kernel(d, "series", s ? &s->phi : nullptr, s ? s->blk_rows : 0, kernel, k0, k1, reps, ms,
                                  [&] {
        return [d, sa = jg::screen_args(jg::series_blk(d), (int)k0, (int)k1, 1.0), la = jg::list_args(d, (int)k0, (int)k1, 1.0, 0)](int which) {
            if (which == 0) jg::launch_screen(d, sa);
            else jg::launch_stats(d, la);
        };
    });
}

int jg_dc_series_set_island_mode(int64_t h, int mode) {
    DC_ENTER(h);
    return jg::dc_phi_set_island_mode(d, "series", mode, d->series_shed);
}

int jg_dc_series_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* labels, int64_t* buses, int64_t* m, int64_t* side) {
    DC_ENTER(h);
    return jg::dc_phi_get_shed_table(d, "series", d->series ? &d->series->phi : nullptr, k0, k1, count, labels, buses, m, side);
}

int jg_dc_series_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow) {
    DC_ENTER(h);
    if (!d->series) return api_fail(4, "jg_dc_series_get_shed: jg_dc_series_build first");
    if (!flow || k0 < 0 || k1 < k0 || k1 > d->series->phi.nk) return api_fail(1, "jg_dc_series_get_shed: bad argument");
    DC_RET(jg::dc_phi_shed_gather(d, &d->series->phi, (int)k0, (int)k1, d->series->F0, d->series->ldt, d->series->T, flow));
    return 0;
}

int jg_dc_series_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_series_free(d);
    return 0;
}

}  // extern "C"
