// jg_dcse_critical.hip -- the critical-measurement and critical-pair screen of a DC measurement set (jg_dcse_critical.hpp has the algebra).  The handle,
// the factor and the sweep pair are the estimator's (jg_dcse.hpp, jg_dc_sweep.hip); here: the cross pass over all rows of H against one block of
// U = G^-1 H_J', its finishing kernel, the host loop over the blocks, the records, the C ABI.
// Coefficients, column indices and the per-row constants of row i are wave-uniform and go through scalar loads; every store is a vector store.
#include "jg_dcse_critical.hpp"
#include "jg_dc_abi.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>

#include "../../include/jgrid.h"
#include "jg_engine.hpp"

namespace jg {

namespace {

constexpr int LDO = DCSE_OMEGA_LD;
constexpr int GROUPS = LDO / 64;            // column groups (waves) of a block

// live[i] = 1: in service and not critical; single[i] = 1: in service and critical (w_i Omega_ii <= DCSE_SINGULAR, the rule of k_dcse_extend's first pivot)
__global__ void k_dcse_live(const int* st, const double* omega, const double* wi, int* live, int* single, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const bool crit = st[i] && !(omega[i] > DCSE_SINGULAR * wi[i]);
    live[i] = st[i] && !crit;
    single[i] = crit;
}

struct DcseCrossArgs {
    const int* r_ptr; const int* r_col; const double* r_val; const int* live; const double* omega; const double* wi;
    const double* U;                             // [n][LDO]: G^-1 h_j' of the block's columns j = j0 + lane
    double* part;                                // [chunks][3][LDO]: the chunk's largest |gamma|, that gamma, its row
    int* count;                                  // [chunks][groups][2]: records, critical pairs among them
    const long long* off;                        // WRITE [chunks][groups]: the first record of the wave
    double* rec; long long cap;                  // WRITE [cap][3]: i, j (1-based), gamma
    double corr;                                 // < 0: critical pairs only
    int m, j0, groups, g0, slack;                // groups of the whole set, the block's first
};
// grid (chunks of DCSE_ROWS rows, LDO / 256): the four waves of a workgroup share the chunk (its rows of H come through the scalar cache once) and take
// 64 columns each
template <bool WRITE>
__global__ __launch_bounds__(256) void k_dcse_cross(DcseCrossArgs a) {
    const int chunk = blockIdx.x, gl = blockIdx.y * 4 + uniform(threadIdx.y), lane = threadIdx.x;
    const int bl = gl * 64 + lane, j = a.j0 + bl, i0 = chunk * DCSE_ROWS;
    const size_t slot = (size_t)chunk * a.groups + a.g0 + gl;
    long long at = 0;
    if (WRITE) {
        if (((CInt)a.count)[2 * slot] == 0) return;
        at = a.off[slot];
        if (at >= a.cap) return;
    }
    const bool jl = j < a.m && a.live[j];
    const double oj = jl ? a.omega[j] : 1.0, wj = jl ? a.wi[j] : 1.0;
    double mx = 0.0, mg = 0.0, mrow = -1.0;
    int nrec = 0, ncrit = 0;
    for (int i = i0; i < min(i0 + DCSE_ROWS, a.m); ++i) {
        if (!((CInt)a.live)[i]) continue;
        const double oi = ((CDbl)a.omega)[i], wii = ((CDbl)a.wi)[i];
        double dot = 0.0;
        for (int p = ((CInt)a.r_ptr)[i]; p < ((CInt)a.r_ptr)[i + 1]; ++p) {
            const int c = ((CInt)a.r_col)[p];
            if (c != a.slack) dot = fma(((CDbl)a.r_val)[p], a.U[(size_t)c * LDO + bl], dot);
        }
        const double oij = -dot;
        const bool valid = jl && i != j, lo = i < j;
        // the pivot of a lane that removes the lower row, then the higher one (k_dcse_extend: d = Omega_hh - L^2 D, L = Omega_lh / D, D = Omega_ll)
        const double ol = lo ? oi : oj, oh = lo ? oj : oi, wh = lo ? wj : wii;
        const double L = oij / ol;
        const double d = oh - L * L * ol;
        const bool crit = valid && !(d > DCSE_SINGULAR * wh);
        const double g = crit ? copysign(1.0, oij) : oij / sqrt(oi * oj);
        const double ag = fabs(g);
        if (!WRITE && valid && ag > mx) { mx = ag; mg = g; mrow = (double)i; }       // first on ties: strict comparison, rows ascending
        const bool hit = valid && lo && (crit || (a.corr >= 0.0 && ag >= a.corr));
        const unsigned long long b = __ballot(hit);
        if (WRITE) {
            const long long pos = at + __popcll(b & ((1ull << lane) - 1ull));
            if (hit && pos < a.cap) { double* r = a.rec + 3 * pos; r[0] = (double)(i + 1); r[1] = (double)(j + 1); r[2] = g; }
            at += __popcll(b);
        } else {
            nrec += __popcll(b);
            ncrit += __popcll(__ballot(hit && crit));
        }
    }
    if (!WRITE) {
        double* o = a.part + (size_t)chunk * 3 * LDO + bl;
        o[0] = mx; o[LDO] = mg; o[2 * LDO] = mrow;
        if (lane == 0) { a.count[2 * slot] = nrec; a.count[2 * slot + 1] = ncrit; }
    }
}
// chunks in ascending order: ties of the maximum go to the lowest row
__global__ __launch_bounds__(256) void k_dcse_cross_finish(const double* part, const int* live, int* partner, double* pgamma, int chunks, int j0, int m) {
    const int bl = blockIdx.x * blockDim.x + threadIdx.x, j = j0 + bl;
    if (bl >= LDO || j >= m) return;
    double mx = 0.0, mg = 0.0, mrow = -1.0;
    for (int c = 0; c < chunks; ++c) {
        const double* o = part + (size_t)c * 3 * LDO + bl;
        if (o[0] > mx) { mx = o[0]; mg = o[LDO]; mrow = o[2 * LDO]; }
    }
    const bool has = live[j] && mrow >= 0.0;
    partner[j] = has ? (int)mrow + 1 : 0;
    pgamma[j] = has ? mg : __longlong_as_double(0x7ff8000000000000LL);
}

// what a screen call holds on the device beside the handle; released when the call ends
struct CriticalPass {
    DcseHandle* h;
    int blocks = 0, groups = 0;
    int* rowid = nullptr; int* live = nullptr; int* single = nullptr; int* partner = nullptr; int* count = nullptr;
    double* Bo = nullptr; double* Wo = nullptr; double* Uo = nullptr; double* part = nullptr; double* pgamma = nullptr; double* rec = nullptr;
    long long* off = nullptr;
    explicit CriticalPass(DcseHandle* handle) : h(handle) {}
    CriticalPass(const CriticalPass&) = delete;
    ~CriticalPass() {
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        dev_release(h, rowid); dev_release(h, live); dev_release(h, single); dev_release(h, partner); dev_release(h, count); dev_release(h, Bo);
        dev_release(h, Wo); dev_release(h, Uo); dev_release(h, part); dev_release(h, pgamma); dev_release(h, rec); dev_release(h, off);
    }
    int setup() {
        const size_t N = (size_t)h->n, M = (size_t)h->m;
        blocks = (h->m + LDO - 1) / LDO;
        groups = blocks * GROUPS;
        if (!h->omega_valid) DC_TRY(compute_omega(h));
        std::vector<int> ids((size_t)blocks * LDO);
        for (size_t s = 0; s < ids.size(); ++s) ids[s] = s < M ? (int)s : -1;
        DC_TRY(dev_alloc(h, &rowid, ids.size(), ids.data()));
        DC_TRY(dev_alloc(h, &live, M, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &single, M, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &partner, M, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &pgamma, M, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &count, (size_t)h->n_chunks * groups * 2, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &Bo, N * LDO, (const double*)nullptr, false));
        DC_TRY(dev_alloc(h, &Wo, (N + 1) * LDO, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &Uo, N * LDO, (const double*)nullptr, false));
        DC_TRY(dev_alloc(h, &part, (size_t)h->n_chunks * 3 * LDO, (const double*)nullptr, true));
        hipLaunchKernelGGL(k_dcse_live, dim3((h->m + 255) / 256), dim3(256), 0, h->stream, h->st, h->omega, h->wi, live, single, h->m);
        DC_HIP(hipGetLastError());
        return 0;
    }
    // U = G^-1 h_j' for the columns of block b: the right-hand sides and the sweep pair of compute_omega
    int solve_block(int b) {
        DC_HIP(hipMemsetAsync(Bo, 0, (size_t)h->n * LDO * sizeof(double), h->stream));
        launch_row_rhs(h, rowid + (size_t)b * LDO, Bo, LDO);
        sweep_pair(h->fac, h->stream, 0, Bo, nullptr, nullptr, Wo, Uo, LDO, GROUPS, nullptr);
        return 0;
    }
    template <bool WRITE>
    void cross(int b, double corr, long long cap) {
        DcseCrossArgs a{};
        a.r_ptr = h->r_ptr; a.r_col = h->r_col; a.r_val = h->r_val; a.live = live; a.omega = h->omega; a.wi = h->wi; a.U = Uo; a.part = part; a.count = count;
        a.off = off; a.rec = rec; a.cap = cap; a.corr = corr; a.m = h->m; a.j0 = b * LDO; a.groups = groups; a.g0 = b * GROUPS; a.slack = h->slack;
        hipLaunchKernelGGL((k_dcse_cross<WRITE>), dim3(h->n_chunks, GROUPS / 4), dim3(64, 4), 0, h->stream, a);
        if (!WRITE) hipLaunchKernelGGL(k_dcse_cross_finish, dim3(LDO / 256), dim3(256), 0, h->stream, part, live, partner, pgamma, h->n_chunks, b * LDO, h->m);
    }
};

}  // namespace

int dcse_critical_screen(DcseHandle* h, double corr, long long capacity, double* records, long long* totals, int* single, int* partner, double* partner_gamma) {
    if (h->any_removed) {
        h->error = "jg_dcse_critical_screen: lanes of this handle have removed rows; the screen is a property of the full set (jg_dcse_set_weights forgets them)";
        return 4;
    }
    CriticalPass P(h);
    DC_TRY(P.setup());
    const size_t M = (size_t)h->m, slots = (size_t)h->n_chunks * P.groups;
    for (int b = 0; b < P.blocks; ++b) {
        DC_TRY(P.solve_block(b));
        P.cross<false>(b, corr, 0);
    }
    DC_HIP(hipGetLastError());
    std::vector<int> cnt(slots * 2), sg(M);
    DC_HIP(hipMemcpyAsync(cnt.data(), P.count, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (partner) DC_HIP(hipMemcpyAsync(partner, P.partner, M * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (partner_gamma) DC_HIP(hipMemcpyAsync(partner_gamma, P.pgamma, M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(sync_copy(sg.data(), P.single, M * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (single) std::copy(sg.begin(), sg.end(), single);
    // offsets in (chunk, group) order; the cut: through the end of the chunk where the running total reaches the capacity
    std::vector<long long> off(slots);
    long long total = 0, pairs = 0, cut = 0;
    for (int c = 0; c < h->n_chunks; ++c) {
        for (int g = 0; g < P.groups; ++g) {
            const size_t s = (size_t)c * P.groups + g;
            off[s] = total; total += cnt[2 * s]; pairs += cnt[2 * s + 1];
        }
        if (cut < capacity) cut = total;
    }
    totals[0] = std::accumulate(sg.begin(), sg.end(), 0LL);
    totals[1] = pairs;
    totals[2] = total - pairs;
    const long long kept = std::min(total, capacity);
    if (!kept || !records) return 0;
    DC_TRY(dev_alloc(h, &P.off, slots, off.data()));
    DC_TRY(dev_alloc(h, &P.rec, (size_t)cut * 3, (const double*)nullptr, true));
    for (int b = 0; b < P.blocks; ++b) {
        bool any = false;
        for (int c = 0; c < h->n_chunks && !any; ++c)
            for (int g = b * GROUPS; g < (b + 1) * GROUPS && !any; ++g) {
                const size_t s = (size_t)c * P.groups + g;
                any = cnt[2 * s] && off[s] < cut;
            }
        if (!any) continue;
        DC_TRY(P.solve_block(b));
        P.cross<true>(b, corr, cut);
    }
    DC_HIP(hipGetLastError());
    std::vector<double> rec((size_t)cut * 3);
    DC_HIP(sync_copy(rec.data(), P.rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    std::vector<long long> order(cut);
    std::iota(order.begin(), order.end(), 0LL);
    std::sort(order.begin(), order.end(), [&](long long x, long long y) {
        return rec[3 * x] != rec[3 * y] ? rec[3 * x] < rec[3 * y] : rec[3 * x + 1] < rec[3 * y + 1];
    });
    for (long long k = 0; k < kept; ++k) std::copy(&rec[3 * order[k]], &rec[3 * order[k]] + 3, records + 3 * k);
    return 0;
}

int dcse_critical_time(DcseHandle* h, int reps, double* ms) {
    CriticalPass P(h);
    DC_TRY(P.setup());
    DC_TRY(P.solve_block(0));
    return time_events(h->stream, reps, ms, h->error, [&]() -> int { P.cross<false>(0, -1.0, 0); return 0; });
}

}  // namespace jg

using jg::DcseHandle;
using jg::api_fail;

extern "C" {

int jg_dcse_critical_screen(int64_t h, double correlation, int64_t capacity, double* records, int64_t* totals, int32_t* single, int32_t* partner,
                            double* partner_gamma) {
    SE_ENTER(h);
    if (!totals || capacity < 0 || (capacity > 0 && !records) || std::isnan(correlation)) return api_fail(1, "jg_dcse_critical_screen: bad argument");
    long long t[3] = {0, 0, 0};
    DC_RET(jg::dcse_critical_screen(d, correlation, capacity, records, t, single, partner, partner_gamma));
    for (int k = 0; k < 3; ++k) totals[k] = t[k];
    return 0;
}

int jg_dcse_get_variance(int64_t h, double* omega) {
    SE_ENTER(h);
    if (!omega) return api_fail(1, "jg_dcse_get_variance: null pointer");
    if (!d->omega_valid) DC_RET(jg::compute_omega(d));
    DC_API_HIP(jg::sync_copy(omega, d->omega, (size_t)d->m * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    return 0;
}

int jg_dcse_critical_time_kernel(int64_t h, int reps, double* ms) {
    SE_ENTER(h);
    if (!ms || reps < 1) return api_fail(1, "jg_dcse_critical_time_kernel: bad argument");
    DC_RET(jg::dcse_critical_time(d, reps, ms));
    return 0;
}

}  // extern "C"
