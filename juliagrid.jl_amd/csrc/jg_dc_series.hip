// jg_dc_series.hip -- the DC N-1 screen over a series of injection profiles (jg_dc_series.hpp has the algebra and the reference loop it stands for).
//
// Build: Phi by the build the pair screen shares (jg_dc_pair.hip), into a state of the series' own; then the sweep pair of jg_dc_sweep.hip over the
// profiles' right-hand sides, DC_PAIR_LANES at a time on scratch of the build's own, and k_series_f0 after each batch (k_pair_phi's shape: a wave is 8 rows
// x 64 profiles, y_m ((theta[from_m] + slack angle) - (theta[to_m] + slack angle) - shiftAngle_m), coalesced stores).  Screen of a row block [k0, k1):
// k_series_screen walks the rows once (a wave = DC_SERIES_TILE candidates k in registers x 64 consecutive profiles; Phi[m, k..], 1 / rating_m and the
// row's candidate position through scalar loads, F0[m, t..t+63] one coalesced vector load reused for every k of the tile; nothing is written per m); the
// records come out of the block's dense result by count (k_series_rows<false>) / prefix sum over the rows (host) / ordered scatter
// (k_series_rows<true>: ballot ranks, no atomics), so the list is sorted by (k, t) and a list that overflows keeps the first.  Every store is a vector store.
#include "jg_dc_series.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/jgrid.h"
#include "jg_dc.hpp"
#include "jg_dc_abi.hpp"

namespace jg {

namespace {

constexpr int SERIES_F0_ROWS = 8;       // rows of F0 per wave of k_series_f0

// F0[r, col0 + lane] = y_m ((theta[from_m] + slack angle) - (theta[to_m] + slack angle) - shiftAngle_m) for the profiles of one lane batch, formed as
// k_dc_flows forms a flow; columns behind the last profile stay 0.  SHIFT false: y_m (theta[from_m] - theta[to_m]), what the flow gains per unit of the
// right-hand side (the transfer screen's G), formed as k_pair_phi forms Phi
struct SeriesF0Args { const double* TH; const int* rbranch; const int* bf; const int* bt; const double* by; const double* bs; double slack_angle;
                      double* F0; int rows, ldb, ldt, col0, T; };
template <bool SHIFT>
__global__ __launch_bounds__(256) void k_series_f0(SeriesF0Args a) {
    const int wave = uniform(threadIdx.y);
    const int r0 = (blockIdx.x * 4 + wave) * SERIES_F0_ROWS;
    const size_t ldb = (size_t)a.ldb, bl = (size_t)blockIdx.y * 64 + threadIdx.x;
    const size_t col = (size_t)a.col0 + bl;
    if (col >= (size_t)a.T) return;
    for (int r = r0; r < min(r0 + SERIES_F0_ROWS, a.rows); ++r) {
        const int m = ((CInt)a.rbranch)[r];
        const int f = ((CInt)a.bf)[m], t = ((CInt)a.bt)[m];
        const double y = ((CDbl)a.by)[m], s = ((CDbl)a.bs)[m];
        if constexpr (SHIFT) a.F0[(size_t)r * a.ldt + col] = y * ((a.TH[(size_t)f * ldb + bl] + a.slack_angle) - (a.TH[(size_t)t * ldb + bl] + a.slack_angle) - s);
        else a.F0[(size_t)r * a.ldt + col] = y * (a.TH[(size_t)f * ldb + bl] - a.TH[(size_t)t * ldb + bl]);
    }
}

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

// what left m over the bridge before the outage, for the bridge candidates `list` of a block: out[j][t] = s_k F[row of k][t]
__global__ void k_shed_gather(const double* F, const int* crow, const int* cisl, const int* list, double* out, int nb, int ldt, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    for (int j = blockIdx.y; j < nb; j += gridDim.y) {
        const int k = list[j];
        out[(size_t)j * T + t] = (cisl[4 * k] > 0 ? 1.0 : -1.0) * F[(size_t)crow[k] * ldt + t];
    }
}

void series_release(DcHandle* h) {
    DcSeriesState* s = h->series;
    if (!s) return;
    hipStreamSynchronize(h->stream);
    dc_pair_state_free(h, s->phi);
    dev_release(h, s->F0); dev_release(h, s->b_load); dev_release(h, s->b_branch); dev_release(h, s->b_count);
    dev_release(h, s->r_viol); dev_release(h, s->r_max); dev_release(h, s->r_off); dev_release(h, s->c_max); dev_release(h, s->c_viol);
    dev_release(h, s->base); dev_release(h, s->rec);
    delete s;
    h->series = nullptr;
}

// the lane-batch loop of a build (dc_series_row_flows of jg_dc_series.hpp): F0 of the series screen with the shift angle, G of the transfer screen without
int row_flows(DcHandle* h, const DcPairState* p, int T, const double* rhs, bool shift, double* F, int ldt, double* ms) {
    const int n = h->n, nr = p->rows, ldb = std::min(ldt, DC_PAIR_LANES);
    int rc = 0;
    double* R = nullptr; double* W = nullptr; double* TH = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) { rc = 2; h->error = std::string(what) + ": " + hipGetErrorString(e); } return e == hipSuccess; };
    auto alloc = [&](int r) { if (r && !rc) rc = r; return r == 0; };
    double sweep_ms = 0.0, f0_ms = 0.0;
    // scratch: one lane batch of right-hand sides and of the sweeps (row n of W stays zero)
    if (alloc(dev_alloc(h, &R, (size_t)n * ldb, (const double*)nullptr, true)) && alloc(dev_alloc(h, &W, ((size_t)n + 1) * ldb, (const double*)nullptr, true)) &&
        alloc(dev_alloc(h, &TH, (size_t)n * ldb, (const double*)nullptr, true))) {
        for (auto& e : ev) hip(hipEventCreate(&e), "hipEventCreate");
        std::vector<double> tb;
        for (int c0 = 0; c0 < T && !rc; c0 += ldb) {
            const int cnt = std::min(ldb, T - c0), groups = (cnt + 63) / 64, w = groups * 64;
            tb.assign((size_t)n * w, 0.0);                      // bus-major, lanes behind the last profile carry a zero right-hand side
            for (int q = 0; q < cnt; ++q) {
                const double* src = rhs + (size_t)(c0 + q) * n;
                for (int i = 0; i < n; ++i) tb[(size_t)i * w + q] = src[i];
            }
            for (int q = 0; q < cnt; ++q) tb[(size_t)h->slack * w + q] = 0.0;
            if (!hip(hipMemcpy2DAsync(R, (size_t)ldb * sizeof(double), tb.data(), (size_t)w * sizeof(double), (size_t)w * sizeof(double), (size_t)n, hipMemcpyHostToDevice, h->stream), "upload") ||
                !hip(hipStreamSynchronize(h->stream), "hipStreamSynchronize")) break;
            hip(hipEventRecord(ev[0], h->stream), "hipEventRecord");
            sweep_pair(h->fac, h->stream, 0, R, nullptr, nullptr, W, TH, ldb, groups, nullptr);
            hip(hipEventRecord(ev[1], h->stream), "hipEventRecord");
            SeriesF0Args a{TH, p->row_branch, h->b_from, h->b_to, h->b_y, h->b_shift, h->slack_angle, F, nr, ldb, ldt, c0, T};
            const dim3 grid((nr + 4 * SERIES_F0_ROWS - 1) / (4 * SERIES_F0_ROWS), groups);
            if (shift) hipLaunchKernelGGL(k_series_f0<true>, grid, dim3(64, 4), 0, h->stream, a);
            else hipLaunchKernelGGL(k_series_f0<false>, grid, dim3(64, 4), 0, h->stream, a);
            hip(hipEventRecord(ev[2], h->stream), "hipEventRecord");
            hip(hipGetLastError(), "launch");
            if (!hip(hipEventSynchronize(ev[2]), "hipEventSynchronize")) break;
            float t1 = 0.f, t2 = 0.f;
            hip(hipEventElapsedTime(&t1, ev[0], ev[1]), "hipEventElapsedTime");
            hip(hipEventElapsedTime(&t2, ev[1], ev[2]), "hipEventElapsedTime");
            sweep_ms += t1; f0_ms += t2;
        }
    }
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    dev_release(h, R); dev_release(h, W); dev_release(h, TH);
    ms[0] += sweep_ms; ms[1] += f0_ms;
    return rc;
}
int bridges(DcHandle* h, const DcPairState* p, std::vector<char>& bridge) {
    std::vector<double> diag(p->ldk);
    DC_HIP(sync_copy(diag.data(), p->cand_diag, diag.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    bridge.assign(p->nk, 0);
    for (int k = 0; k < p->nk; ++k) bridge[k] = !(p->shed && p->h_side[k] != 0) && std::fabs(1.0 - diag[k]) < DC_SINGULAR;
    return 0;
}

// rhs [T][n]: the lane right-hand sides as jg_dc_set_injections takes them
int series_build(DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, int T, const double* rhs, int64_t budget, double* info) {
    series_release(h);
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
    const size_t f0_bytes = (size_t)nr * ldt * sizeof(double), scratch = dc_series_flows_scratch(h, ldt);
    for (int j = 8; j < 12; ++j) info[j] = 0.0;
    info[8] = (double)f0_bytes;
    DcSeriesState* s = new DcSeriesState();
    h->series = s;
    s->T = T; s->ldt = ldt;
    const std::string extra = "; F0 needs " + dc_pair_bytes_text(f0_bytes) + " (" + std::to_string(nr) + " rows x " + std::to_string(ldt) + " profiles x 8) and " +
                              dc_pair_bytes_text(scratch) + " of scratch";
    int rc = dc_pair_state_build(h, s->phi, "jg_dc_series_build", cand, mon, budget, f0_bytes + scratch, extra, info, shed);
    if (rc) { const std::string msg = h->error; series_release(h); h->error = msg; return rc; }
    DcPairState* p = s->phi;
    auto step = [&](int r) { if (r && !rc) rc = r; return r == 0; };
    double ms[2] = {0.0, 0.0};
    step(dev_alloc(h, &s->F0, (size_t)nr * ldt, (const double*)nullptr, true)) && step(dev_alloc(h, &s->c_max, (size_t)ldt, (const double*)nullptr, true)) &&
        step(dev_alloc(h, &s->c_viol, (size_t)ldt, (const int*)nullptr, true)) && step(dev_alloc(h, &s->base, (size_t)ldt * 3, (const double*)nullptr, true)) &&
        step(row_flows(h, p, T, rhs, true, s->F0, ldt, ms)) && step(bridges(h, p, s->h_bridge));
    if (rc) { const std::string msg = h->error; series_release(h); h->error = msg; return rc; }
    s->build_ms[0] = ms[0] + ms[1]; s->build_ms[1] = ms[0]; s->build_ms[2] = ms[1];
    info[9] = s->build_ms[0]; info[10] = ms[0]; info[11] = ms[1];
    return 0;
}

// the block's buffers for `rb` rows; grown, never shrunk
int series_block(DcHandle* h, int rb, long long rec_cap) {
    DcSeriesState* s = h->series;
    if (rb > s->blk_rows) {
        const size_t cells = (size_t)rb * s->ldt, need = cells * 16;
        dev_release(h, s->b_load); dev_release(h, s->b_branch); dev_release(h, s->b_count);
        dev_release(h, s->r_viol); dev_release(h, s->r_max); dev_release(h, s->r_off);
        s->blk_rows = 0;
        size_t free_b = 0, total_b = 0;
        DC_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b) {
            h->error = "jg_dc_series_screen: a block of " + std::to_string(rb) + " rows needs " + dc_pair_bytes_text(need) + ", " + dc_pair_bytes_text(free_b) +
                       " are free: screen fewer rows per call";
            return 5;
        }
        DC_TRY(dev_alloc(h, &s->b_load, cells, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &s->b_branch, cells, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &s->b_count, cells, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &s->r_viol, (size_t)rb, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &s->r_max, (size_t)rb, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &s->r_off, (size_t)rb, (const long long*)nullptr, true));
        s->blk_rows = rb;
    }
    if (rec_cap > s->rec_cap) { dev_release(h, s->rec); s->rec_cap = 0; DC_TRY(dev_alloc(h, &s->rec, (size_t)rec_cap * 5, (const double*)nullptr, true)); s->rec_cap = rec_cap; }
    return 0;
}

SeriesScreenArgs screen_args(DcHandle* h, int k0, int k1, double thr) {
    DcSeriesState* s = h->series;
    DcPairState* p = s->phi;
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
    a.load = s->b_load; a.branch = s->b_branch; a.count = s->b_count; a.clabel = s->phi->cand_label;
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
// the block's dense result of one quantity on the host: [k1 - k0][T]
template <typename V, typename D>
int series_dense(DcHandle* h, D* dst, const V* src, int rb) {
    const int T = h->series->T, ldt = h->series->ldt;
    std::vector<V> t((size_t)rb * ldt);
    DC_HIP(sync_copy(t.data(), src, t.size() * sizeof(V), hipMemcpyDeviceToHost, h->stream));
    for (int i = 0; i < rb; ++i)
        for (int q = 0; q < T; ++q) dst[(size_t)i * T + q] = (D)t[(size_t)i * ldt + q];
    return 0;
}
int series_screen(DcHandle* h, int k0, int k1, double thr, long long rec_cap, const SeriesOut& o) {
    DcSeriesState* s = h->series;
    DcPairState* p = s->phi;
    const int rb = k1 - k0, T = s->T, ldt = s->ldt;
    DC_TRY(series_block(h, rb, rec_cap));
    dc_pair_state_rinv(h, p);
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
    std::vector<long long> off(rb);
    long long viol = 0, isl = 0;
    for (int i = 0; i < rb; ++i) {
        off[i] = viol; viol += nv[i];
        if (s->h_bridge[k0 + i]) { if (o.islanding) o.islanding[isl] = p->h_cand[k0 + i] + 1; ++isl; }
    }
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
    if (o.d_load) DC_TRY(series_dense(h, o.d_load, (const double*)s->b_load, rb));
    if (o.d_branch) DC_TRY(series_dense(h, o.d_branch, (const int*)s->b_branch, rb));
    if (o.d_count) DC_TRY(series_dense(h, o.d_count, (const int*)s->b_count, rb));
    return 0;
}

}  // namespace

void dc_series_free(DcHandle* h) { series_release(h); }
size_t dc_series_flows_scratch(const DcHandle* h, int ldt) { return ((size_t)3 * h->n + 1) * std::min(ldt, DC_PAIR_LANES) * sizeof(double); }
int dc_series_row_flows(DcHandle* h, const DcPairState* p, int T, const double* rhs, bool shift, double* F, int ldt, double* ms) {
    return row_flows(h, p, T, rhs, shift, F, ldt, ms);
}
int dc_series_bridges(DcHandle* h, const DcPairState* p, std::vector<char>& bridge) { return bridges(h, p, bridge); }
int dc_series_shed_table(const DcHandle* h, const DcPairState* p, int k0, int k1, int64_t* labels, int64_t* buses, int64_t* m, int64_t* side) {
    int nb = 0;
    if (!p->shed) return 0;
    for (int k = k0; k < k1; ++k) {
        if (p->h_side[k] == 0) continue;
        const int br = p->h_cand[k];
        if (labels) labels[nb] = br + 1;
        if (buses) buses[nb] = p->h_hi[k] - p->h_lo[k] + 1;
        if (m) m[nb] = (p->h_side[k] > 0 ? h->h_from[br] : h->h_to[br]) + 1;
        if (side) side[nb] = p->h_side[k];
        ++nb;
    }
    return nb;
}
int dc_series_shed_gather(DcHandle* h, const DcPairState* p, int k0, int k1, const double* F, int ldt, int T, double* out) {
    std::vector<int> list;
    if (p->shed)
        for (int k = k0; k < k1; ++k) if (p->h_side[k] != 0) list.push_back(k);
    const int nb = (int)list.size();
    if (!nb) return 0;
    int* d_list = nullptr; double* d_out = nullptr;
    int rc = dev_alloc(h, &d_list, (size_t)nb, list.data());
    if (!rc) rc = dev_alloc(h, &d_out, (size_t)nb * T, (const double*)nullptr, false);
    if (!rc) {
        hipLaunchKernelGGL(k_shed_gather, dim3((T + 255) / 256, std::min(nb, 4096)), dim3(256), 0, h->stream, F, p->cand_row, p->cand_isl, d_list, d_out, nb, ldt, T);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = sync_copy(out, d_out, (size_t)nb * T * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) { h->error = std::string("shed gather: ") + hipGetErrorString(e); rc = 2; }
    }
    dev_release(h, d_list); dev_release(h, d_out);
    return rc;
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
    DC_RET(jg::dc_pair_lists(d, "jg_dc_series_build", nk, candidates, nm, monitored, cand, mon));
    DC_RET(jg::series_build(d, cand, mon, (int)profiles, rhs, budget_bytes, info));
    return 0;
}

int jg_dc_series_screen(int64_t h, int64_t k0, int64_t k1, double threshold, int64_t capacity, double* records, int64_t* islanding, int64_t* totals,
                        double* worst, double* worst_profile, int64_t* violating_profile, double* base, double* dense_load, int32_t* dense_branch,
                        int32_t* dense_count) {
    DC_ENTER(h);
    if (!d->series) return api_fail(4, "jg_dc_series_screen: jg_dc_series_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_series_screen: jg_dc_set_rating first (the loadings are |from| / rating)");
    if (k0 < 0 || k1 <= k0 || k1 > d->series->phi->nk) return api_fail(1, "jg_dc_series_screen: rows [k0, k1) out of range");
    if (!(threshold >= 0.0) || capacity < 0 || (capacity && !records) || !totals) return api_fail(1, "jg_dc_series_screen: bad argument");
    jg::SeriesOut o{records, islanding, totals, worst, worst_profile, violating_profile, base, dense_load, dense_branch, dense_count};
    DC_RET(jg::series_screen(d, (int)k0, (int)k1, threshold, capacity, o));
    return 0;
}

int jg_dc_series_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms) {
    DC_ENTER(h);
    if (!d->series) return api_fail(4, "jg_dc_series_time_kernel: jg_dc_series_build first");
    if (!ms || reps < 1 || kernel < 0 || kernel > 1 || k0 < 0 || k1 <= k0 || k1 > d->series->phi->nk) return api_fail(1, "jg_dc_series_time_kernel: bad argument");
    if (k1 - k0 > d->series->blk_rows) return api_fail(4, "jg_dc_series_time_kernel: jg_dc_series_screen with a block of at least these rows first");
    const jg::SeriesScreenArgs sa = jg::screen_args(d, (int)k0, (int)k1, 1.0);
    const jg::SeriesListArgs la = jg::list_args(d, (int)k0, (int)k1, 1.0, 0);
    DC_RET(jg::time_events(d->stream, reps, ms, d->error, [&]() -> int {
        if (kernel == 0) jg::launch_screen(d, sa);
        else jg::launch_stats(d, la);
        return 0;
    }));
    return 0;
}

int jg_dc_series_set_island_mode(int64_t h, int mode) {
    DC_ENTER(h);
    if (mode != 0 && mode != 1) return api_fail(1, "jg_dc_series_set_island_mode: mode is 0 (a bridge candidate is skipped: status 3) or 1 (screened on the slack's island)");
    if (mode == 1 && !d->nbr) return api_fail(1, "jg_dc_series_set_island_mode: jg_dc_set_branches first");
    d->series_shed = mode;
    return 0;
}

int jg_dc_series_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* labels, int64_t* buses, int64_t* m, int64_t* side) {
    DC_ENTER(h);
    if (!d->series) return api_fail(4, "jg_dc_series_get_shed_table: jg_dc_series_build first");
    if (!count || k0 < 0 || k1 < k0 || k1 > d->series->phi->nk) return api_fail(1, "jg_dc_series_get_shed_table: bad argument");
    *count = jg::dc_series_shed_table(d, d->series->phi, (int)k0, (int)k1, labels, buses, m, side);
    return 0;
}

int jg_dc_series_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow) {
    DC_ENTER(h);
    if (!d->series) return api_fail(4, "jg_dc_series_get_shed: jg_dc_series_build first");
    if (!flow || k0 < 0 || k1 < k0 || k1 > d->series->phi->nk) return api_fail(1, "jg_dc_series_get_shed: bad argument");
    DC_RET(jg::dc_series_shed_gather(d, d->series->phi, (int)k0, (int)k1, d->series->F0, d->series->ldt, d->series->T, flow));
    return 0;
}

int jg_dc_series_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_series_free(d);
    return 0;
}

}  // extern "C"
