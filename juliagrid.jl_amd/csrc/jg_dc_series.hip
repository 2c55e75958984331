// jg_dc_series.hip -- the DC N-1 screen over a series of injection profiles (jg_dc_series.hpp has the algebra and the reference loop it stands for).
//
// Build: Phi by the build the three screens share (dc_phi_build, jg_dc_phi.hip), into a state of the series' own; then F0, the row flows of the profiles'
// right-hand sides (dc_phi_row_flows: the sweep pair of jg_dc_sweep.hip, DC_PAIR_LANES profiles at a time).  Screen of a row block [k0, k1):
// k_series_screen walks the rows once (a wave = DC_SERIES_TILE candidates k in registers x 64 consecutive profiles; Phi[m, k..], 1 / rating_m and the
// row's candidate position through scalar loads, F0[m, t..t+63] one coalesced vector load reused for every k of the tile; nothing is written per m); the
// records come out of the block's dense result by count (k_series_rows<false>) / prefix sum over the rows (host) / ordered scatter
// (k_series_rows<true>: ballot ranks, no atomics), so the list is sorted by (k, t) and a list that overflows keeps the first.  Every store is a vector store.
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

// ---- summaries out of the block's dense result: count, (prefix sum on the host), ordered scatter ---------------------------------------------
struct SeriesListArgs {
    const double* load; const int* branch; const int* count; const int* clabel;
    int* r_viol; double* r_max;                                  // per row of the block
    const long long* r_off;                                      // scatter: the row's first record
    double* rec; long long rec_cap;
    double thr; int ldt, T, k0, k1;
};
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_series_rows(SeriesListArgs a) {
    const int wave = uniform(threadIdx.y), lane = threadIdx.x;
    const int i = blockIdx.x * 4 + wave;
    const int k = a.k0 + i;
    if (k >= a.k1) return;
    const size_t ldt = (size_t)a.ldt;
    int nv = 0;
    double mx = 0.0;
    long long vb = SCATTER ? a.r_off[i] : 0;
    const int klab = ((CInt)a.clabel)[k];
    for (int t0 = 0; t0 < a.T; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < a.T;
        const double v = valid ? a.load[(size_t)i * ldt + t] : 0.0;
        const bool viol = valid && v > a.thr;                    // (a NaN, the loading of a bridge candidate, compares false)
        const unsigned long long mv = __ballot(viol);
        if (SCATTER) {
            if (viol) {
                const long long at = vb + __popcll(mv & ((1ull << lane) - 1ull));
                if (at < a.rec_cap) {
                    double* q = a.rec + at * 5;
                    q[0] = (double)klab; q[1] = (double)t; q[2] = (double)a.branch[(size_t)i * ldt + t]; q[3] = v; q[4] = (double)a.count[(size_t)i * ldt + t];
                }
            }
            vb += __popcll(mv);
        } else {
            nv += __popcll(mv);
            if (valid && v > mx) mx = v;
        }
    }
    if (!SCATTER) {
        for (int s = 32; s; s >>= 1) mx = fmax(mx, __shfl_xor(mx, s, 64));
        if (lane == 0) { a.r_viol[i] = nv; a.r_max[i] = mx; }
    }
}
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
    int nr = 0;
    {
        std::vector<char> in(h->nbr, 0);
        for (int m : mon) in[m] = 1;
        for (int m : cand) in[m] = 1;
        for (char c : in) nr += c;
    }
    const size_t f0_bytes = (size_t)nr * ldt * sizeof(double), scratch = dc_phi_flows_scratch(h, ldt);
    for (int j = 8; j < 12; ++j) info[j] = 0.0;
    info[8] = (double)f0_bytes;
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
    s->build_ms[0] = ms[0] + ms[1]; s->build_ms[1] = ms[0]; s->build_ms[2] = ms[1];
    info[9] = s->build_ms[0]; info[10] = ms[0]; info[11] = ms[1];
    return 0;
}

// the block's buffers for `rb` rows; grown, never shrunk
int series_block(DcHandle* h, int rb, long long rec_cap) {
    DcSeriesState* s = h->series;
    if (rb > s->blk_rows) {
        const size_t cells = (size_t)rb * s->ldt, r = (size_t)rb;
        DC_TRY(dc_block_grow(h, s->mem, "jg_dc_series_screen", rb, s->blk_rows, cells * 16, dc_blk(s->b_load, cells), dc_blk(s->b_branch, cells), dc_blk(s->b_count, cells),
                             dc_blk(s->r_viol, r), dc_blk(s->r_max, r), dc_blk(s->r_off, r)));
    }
    return dc_list_grow(h, s->mem, s->rec, s->rec_cap, rec_cap, 5);
}

SeriesScreenArgs screen_args(DcHandle* h, int k0, int k1, double thr) {
    DcSeriesState* s = h->series;
    const DcPhi* p = &s->phi;
    SeriesScreenArgs a{};
    a.Phi = p->Phi; a.F0 = s->F0; a.rinv = p->row_rinv; a.pos = p->row_pos; a.rbranch = p->row_branch; a.crow = p->cand_row; a.cdiag = p->cand_diag;
    a.load = s->b_load; a.branch = s->b_branch; a.count = s->b_count;
    a.thr = thr; a.rows = p->rows; a.ldk = p->ldk; a.ldt = s->ldt; a.T = s->T; a.k0 = k0; a.k1 = k1; a.kbase = k0 / DC_SERIES_TILE * DC_SERIES_TILE;
    a.cisl = p->shed ? p->cand_isl : nullptr; a.rpre = p->shed ? p->row_pre : nullptr;
    return a;
}
void launch_screen(DcHandle* h, const SeriesScreenArgs& a) {
    const int tiles = (a.k1 - a.kbase + DC_SERIES_TILE - 1) / DC_SERIES_TILE;
    const dim3 grid(a.ldt / 64, (tiles + DC_PAIR_WAVES - 1) / DC_PAIR_WAVES), block(64, DC_PAIR_WAVES);
    if (a.cisl) hipLaunchKernelGGL(k_series_screen<true>, grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL(k_series_screen<false>, grid, block, 0, h->stream, a);
}
SeriesListArgs list_args(DcHandle* h, int k0, int k1, double thr, long long rec_cap) {
    DcSeriesState* s = h->series;
    SeriesListArgs a{};
    a.load = s->b_load; a.branch = s->b_branch; a.count = s->b_count; a.clabel = s->phi.cand_label;
    a.r_viol = s->r_viol; a.r_max = s->r_max; a.r_off = s->r_off; a.rec = s->rec; a.rec_cap = rec_cap;
    a.thr = thr; a.ldt = s->ldt; a.T = s->T; a.k0 = k0; a.k1 = k1;
    return a;
}
void launch_stats(DcHandle* h, const SeriesListArgs& a) {
    DcSeriesState* s = h->series;
    hipLaunchKernelGGL((k_series_rows<false>), dim3((a.k1 - a.k0 + 3) / 4), dim3(64, 4), 0, h->stream, a);
    hipLaunchKernelGGL(k_series_cols, dim3((s->ldt + 255) / 256), dim3(256), 0, h->stream, s->b_load, s->c_max, s->c_viol, a.thr, s->ldt, s->T, a.k1 - a.k0);
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
    launch_screen(h, screen_args(h, k0, k1, thr));
    SeriesListArgs la = list_args(h, k0, k1, thr, rec_cap);
    launch_stats(h, la);
    if (o.base) hipLaunchKernelGGL(k_series_base, dim3((T + 63) / 64), dim3(64), 0, h->stream, s->F0, p->row_rinv, p->row_branch, s->base, thr, p->rows, ldt, T);
    DC_HIP(hipGetLastError());
    std::vector<int> nv(rb), cviol(ldt);
    std::vector<double> rmax(rb), cmax(ldt);
    DC_HIP(hipMemcpyAsync(nv.data(), s->r_viol, rb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipMemcpyAsync(rmax.data(), s->r_max, rb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipMemcpyAsync(cviol.data(), s->c_viol, ldt * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (o.base) DC_HIP(hipMemcpyAsync(o.base, s->base, (size_t)T * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(sync_copy(cmax.data(), s->c_max, ldt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    std::vector<long long> off;
    const long long viol = dc_prefix(nv, off);
    long long isl = 0;
    for (int i = 0; i < rb; ++i)
        if (s->h_bridge[k0 + i]) { if (o.islanding) o.islanding[isl] = p->h_cand[k0 + i] + 1; ++isl; }
    const long long nrec = std::min(viol, rec_cap);
    if (nrec) {
        DC_HIP(hipMemcpyAsync(s->r_off, off.data(), rb * sizeof(long long), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL((k_series_rows<true>), dim3((rb + 3) / 4), dim3(64, 4), 0, h->stream, la);
        DC_HIP(hipGetLastError());
        DC_HIP(hipMemcpyAsync(o.records, s->rec, (size_t)nrec * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(hipStreamSynchronize(h->stream));                // (off goes out of scope behind it)
    }
    o.totals[0] = (long long)rb * T; o.totals[1] = viol; o.totals[2] = isl; o.totals[3] = nrec; o.totals[4] = viol > rec_cap ? 1 : 0;
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
        return [d, sa = jg::screen_args(d, (int)k0, (int)k1, 1.0), la = jg::list_args(d, (int)k0, (int)k1, 1.0, 0)](int which) {
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
