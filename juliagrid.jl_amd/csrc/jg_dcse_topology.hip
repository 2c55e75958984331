// jg_dcse_topology.hip -- branch status tests of a DC measurement set (jg_dcse_topology.hpp has the algebra).  The handle, the factor and the sweep pair
// are the estimator's (jg_dcse.hpp, jg_dc_sweep.hip); here: the right-hand sides H' W m_k, the denominators, the statistic of every (candidate, lane), the
// records, the corrected angles, the C ABI.
// In k_topo_stat the candidates' denominators, row ids, signs and weights are wave-uniform and go through scalar loads; every store is a vector store.
#include "jg_dcse_topology.hpp"
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
constexpr int GROUPS = LDO / 64;
constexpr long long QNAN = 0x7ff8000000000000LL;

struct TopoCols { const int* ptr; const int* row; const double* sgn; };                                  // the candidates' meter columns
struct TopoRows { const int* r_ptr; const int* r_col; const double* r_val; const double* ws; int slack; };     // H by rows, status x precision

// lane bl of B [n][ld] (zero on entry) gets g_k = H' W m_k of its candidate k = cand[bl] (-1: none), the slack's entry dropped.  One lane owns one column
// of B; a bus hit by several rows is summed in the column's stored order
__global__ void k_topo_rhs(const int* cand, TopoCols t, TopoRows H, double* B, int ld) {
    const int bl = blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= ld) return;
    const int k = cand[bl];
    if (k < 0) return;
    for (int q = t.ptr[k]; q < t.ptr[k + 1]; ++q) {
        const int i = t.row[q];
        const double s = t.sgn[q] * H.ws[i];
        if (s == 0.0) continue;                                          // out of service
        for (int p = H.r_ptr[i]; p < H.r_ptr[i + 1]; ++p)
            if (H.r_col[p] != H.slack) B[(size_t)H.r_col[p] * ld + bl] += s * H.r_val[p];
    }
}
// the same entries against the swept column U = G^-1 g_k: N_k = m_k' W m_k, D_k = N_k - g_k . x_k, the status
__global__ void k_topo_denominator(const int* cand, TopoCols t, TopoRows H, const double* U, double* D, double* norm, int* stat, int ld) {
    const int bl = blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= ld) return;
    const int k = cand[bl];
    if (k < 0) return;
    double nrm = 0.0, dot = 0.0;
    for (int q = t.ptr[k]; q < t.ptr[k + 1]; ++q) {
        const int i = t.row[q];
        const double w = H.ws[i], s = t.sgn[q] * w;
        if (w == 0.0) continue;
        nrm += w;
        for (int p = H.r_ptr[i]; p < H.r_ptr[i + 1]; ++p)
            if (H.r_col[p] != H.slack) dot = fma(s * H.r_val[p], U[(size_t)H.r_col[p] * ld + bl], dot);
    }
    const double d = nrm - dot;
    D[k] = d; norm[k] = nrm;
    stat[k] = nrm == 0.0 ? 2 : (d > DCSE_SINGULAR * nrm ? 0 : 1);
}

struct TopoStatArgs {
    TopoCols t; const double* ws; const double* R; const double* D; const int* stat;
    double* part;                                // [chunks][4][ld]: the chunk's largest |t|, that t, its phi^, its candidate
    int* lcount;                                 // [chunks][ld]: the lane's candidates with |t| >= threshold
    int* count;                                  // [chunks][groups]: records of the wave
    const long long* off;                        // WRITE [groups][chunks]: the first record of the wave
    double* rec; long long cap;                  // WRITE [cap][4]: lane, candidate (1-based), t, phi^
    double* dense;                               // nullable [count][ld]
    double threshold;
    int count_k, batch, ld, groups, chunks;
};
// grid (chunks of TOPO_CHUNK candidates, groups / 4): the four waves of a workgroup share the chunk (its columns come through the scalar cache once) and
// take 64 lanes of the batch each.  Padding lanes batch <= l < ld produce nothing
template <bool WRITE>
__global__ __launch_bounds__(256) void k_topo_stat(TopoStatArgs a) {
    const int chunk = blockIdx.x, gl = blockIdx.y * 4 + uniform(threadIdx.y), lane = threadIdx.x;
    if (gl >= a.groups) return;
    const int l = gl * 64 + lane, k0 = chunk * TOPO_CHUNK;
    const bool mine = l < a.batch;
    long long at = 0;
    if (WRITE) {
        if (((CInt)a.count)[(size_t)chunk * a.groups + gl] == 0) return;
        at = a.off[(size_t)gl * a.chunks + chunk];
        if (at >= a.cap) return;
    }
    double mx = 0.0, mt = 0.0, mphi = 0.0, mk = -1.0;
    int nrec = 0, nlane = 0;
    for (int k = k0; k < min(k0 + TOPO_CHUNK, a.count_k); ++k) {
        if (((CInt)a.stat)[k] != 0) {
            if (!WRITE && a.dense && mine) a.dense[(size_t)k * a.ld + l] = __longlong_as_double(QNAN);
            continue;
        }
        const double d = ((CDbl)a.D)[k];
        double c = 0.0;
        for (int q = ((CInt)a.t.ptr)[k]; q < ((CInt)a.t.ptr)[k + 1]; ++q) {
            const int i = ((CInt)a.t.row)[q];
            c = fma(((CDbl)a.t.sgn)[q] * ((CDbl)a.ws)[i], a.R[(size_t)i * a.ld + l], c);
        }
        const double tt = c / sqrt(d), phi = c / d, ab = fabs(tt);
        const bool hit = mine && ab >= a.threshold;
        const unsigned long long b = __ballot(hit);
        if (WRITE) {
            const long long pos = at + __popcll(b & ((1ull << lane) - 1ull));
            if (hit && pos < a.cap) { double* r = a.rec + 4 * pos; r[0] = (double)(l + 1); r[1] = (double)(k + 1); r[2] = tt; r[3] = phi; }
            at += __popcll(b);
        } else {
            if (a.dense && mine) a.dense[(size_t)k * a.ld + l] = tt;
            if (mk < 0.0 || ab > mx) { mx = ab; mt = tt; mphi = phi; mk = (double)k; }      // first on ties: strict comparison, candidates ascending
            nrec += __popcll(b);
            nlane += hit;
        }
    }
    if (!WRITE) {
        double* o = a.part + (size_t)chunk * 4 * a.ld + l;
        o[0] = mx; o[a.ld] = mt; o[2 * (size_t)a.ld] = mphi; o[3 * (size_t)a.ld] = mk;
        a.lcount[(size_t)chunk * a.ld + l] = nlane;
        if (lane == 0) a.count[(size_t)chunk * a.groups + gl] = nrec;
    }
}
// chunks in ascending order: ties of the maximum go to the lowest candidate
__global__ __launch_bounds__(64) void k_topo_stat_finish(const double* part, const int* lcount, int* best, double* bt, double* bphi, int* cnt, int chunks, int ld) {
    const size_t l = (size_t)blockIdx.x * 64 + threadIdx.x, L = (size_t)ld;
    double mx = 0.0, mt = 0.0, mphi = 0.0, mk = -1.0;
    int n = 0;
    for (int c = 0; c < chunks; ++c) {
        const double* o = part + (size_t)c * 4 * L + l;
        if (o[3 * L] >= 0.0 && (mk < 0.0 || o[0] > mx)) { mx = o[0]; mt = o[L]; mphi = o[2 * L]; mk = o[3 * L]; }
        n += lcount[(size_t)c * L + l];
    }
    best[l] = (int)mk + 1;
    bt[l] = mk < 0.0 ? __longlong_as_double(QNAN) : mt;
    bphi[l] = mk < 0.0 ? __longlong_as_double(QNAN) : mphi;
    cnt[l] = n;
}

// theta' = theta^ - x phi^ of the lane's candidate (cand < 0: theta^ as it is), in place of x; TOPO_APPLY_ROWS state rows per wavefront
constexpr int TOPO_APPLY_ROWS = 8;
struct TopoApplyArgs { const int* cand; TopoCols t; const double* ws; const double* R; const double* D; const double* TH; double* X; int n, ld; };
__global__ __launch_bounds__(256) void k_topo_apply(TopoApplyArgs a) {
    const size_t ld = (size_t)a.ld, bl = (size_t)blockIdx.y * 64 + threadIdx.x;
    const int k = a.cand[bl];
    double phi = 0.0;
    if (k >= 0) {
        double c = 0.0;
        for (int q = a.t.ptr[k]; q < a.t.ptr[k + 1]; ++q) {
            const int i = a.t.row[q];
            c = fma(a.t.sgn[q] * a.ws[i], a.R[(size_t)i * ld + bl], c);
        }
        phi = c / a.D[k];
    }
    const int j0 = (blockIdx.x * 4 + uniform(threadIdx.y)) * TOPO_APPLY_ROWS;
    for (int j = j0; j < min(j0 + TOPO_APPLY_ROWS, a.n); ++j) {
        const double th = a.TH[(size_t)j * ld + bl];
        a.X[(size_t)j * ld + bl] = k >= 0 ? fma(-phi, a.X[(size_t)j * ld + bl], th) : th;
    }
}

TopoCols cols_of(const DcseHandle* h) { return TopoCols{h->t_ptr, h->t_row, h->t_sgn}; }
TopoRows rows_of(const DcseHandle* h) { return TopoRows{h->r_ptr, h->r_col, h->r_val, h->ws, h->slack}; }

bool cache_current(const DcseHandle* h) { return h->topo_valid && h->topo_factor == h->refactorisations; }

// the denominators' device scratch: DCSE_OMEGA_LD candidates per sweep pair; released when the call ends
struct DenominatorPass {
    DcseHandle* h;
    int blocks = 0;
    int* ids = nullptr; double* Bo = nullptr; double* Wo = nullptr; double* Uo = nullptr;
    explicit DenominatorPass(DcseHandle* handle) : h(handle) {}
    DenominatorPass(const DenominatorPass&) = delete;
    ~DenominatorPass() {
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        dev_release(h, ids); dev_release(h, Bo); dev_release(h, Wo); dev_release(h, Uo);
    }
    int setup() {
        const size_t N = (size_t)h->n;
        blocks = (h->t_count + LDO - 1) / LDO;
        std::vector<int> v((size_t)blocks * LDO);
        for (size_t s = 0; s < v.size(); ++s) v[s] = s < (size_t)h->t_count ? (int)s : -1;
        DC_TRY(dev_alloc(h, &ids, v.size(), v.data()));
        DC_TRY(dev_alloc(h, &Bo, N * LDO, (const double*)nullptr, false));
        DC_TRY(dev_alloc(h, &Wo, (N + 1) * LDO, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &Uo, N * LDO, (const double*)nullptr, false));
        return 0;
    }
    int rhs(int b) {
        DC_HIP(hipMemsetAsync(Bo, 0, (size_t)h->n * LDO * sizeof(double), h->stream));
        hipLaunchKernelGGL(k_topo_rhs, dim3(LDO / 256), dim3(256), 0, h->stream, ids + (size_t)b * LDO, cols_of(h), rows_of(h), Bo, LDO);
        return 0;
    }
    void sweep() { sweep_pair(h->fac, h->stream, 0, Bo, nullptr, nullptr, Wo, Uo, LDO, GROUPS, nullptr); }
    void finish(int b) {
        hipLaunchKernelGGL(k_topo_denominator, dim3(LDO / 256), dim3(256), 0, h->stream, ids + (size_t)b * LDO, cols_of(h), rows_of(h), Uo, h->t_D, h->t_norm,
                           h->t_stat, LDO);
    }
    int all() {
        for (int b = 0; b < blocks; ++b) { DC_TRY(rhs(b)); sweep(); finish(b); }
        DC_HIP(hipGetLastError());
        return 0;
    }
};

int need_candidates(DcseHandle* h, const char* who) {
    if (h->t_count) return 0;
    h->error = std::string(who) + ": jg_dcse_topology_set first";
    return 4;
}
// a solved handle whose lanes removed nothing: R is the residual of the full set's estimate
int need_full_set_estimate(DcseHandle* h, const char* who) {
    if (!h->solved) { h->error = std::string(who) + ": the handle is not solved (jg_dcse_solve first)"; return 1; }
    if (h->any_removed) {
        h->error = std::string(who) + ": lanes of this handle have removed rows; the test reads the residuals of the full set (jg_dcse_set_weights forgets them)";
        return 1;
    }
    return 0;
}

// what a screen call holds on the device beside the handle; released when the call ends
struct StatPass {
    DcseHandle* h;
    int chunks = 0, groups = 0;
    double* part = nullptr; int* lcount = nullptr; int* count = nullptr; long long* off = nullptr; double* rec = nullptr; double* dense = nullptr;
    int* best = nullptr; double* bt = nullptr; double* bphi = nullptr; int* cnt = nullptr;
    explicit StatPass(DcseHandle* handle) : h(handle) {}
    StatPass(const StatPass&) = delete;
    ~StatPass() {
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        dev_release(h, part); dev_release(h, lcount); dev_release(h, count); dev_release(h, off); dev_release(h, rec); dev_release(h, dense);
        dev_release(h, best); dev_release(h, bt); dev_release(h, bphi); dev_release(h, cnt);
    }
    int setup(bool want_dense) {
        const size_t ld = (size_t)h->ld;
        chunks = (h->t_count + TOPO_CHUNK - 1) / TOPO_CHUNK;
        groups = h->ld / 64;
        DC_TRY(dev_alloc(h, &part, (size_t)chunks * 4 * ld, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &lcount, (size_t)chunks * ld, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &count, (size_t)chunks * groups, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &best, ld, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &bt, ld, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &bphi, ld, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &cnt, ld, (const int*)nullptr, true));
        if (want_dense) DC_TRY(dev_alloc(h, &dense, (size_t)h->t_count * ld, (const double*)nullptr, true));
        return 0;
    }
    template <bool WRITE>
    void launch(double threshold, long long cap) {
        TopoStatArgs a{};
        a.t = cols_of(h); a.ws = h->ws; a.R = h->R; a.D = h->t_D; a.stat = h->t_stat; a.part = part; a.lcount = lcount; a.count = count; a.off = off; a.rec = rec;
        a.cap = cap; a.dense = dense; a.threshold = threshold; a.count_k = h->t_count; a.batch = h->batch; a.ld = h->ld; a.groups = groups; a.chunks = chunks;
        hipLaunchKernelGGL((k_topo_stat<WRITE>), dim3(chunks, (groups + 3) / 4), dim3(64, 4), 0, h->stream, a);
        if (!WRITE) hipLaunchKernelGGL(k_topo_stat_finish, dim3(groups), dim3(64), 0, h->stream, part, lcount, best, bt, bphi, cnt, chunks, h->ld);
    }
};

// the lanes' candidates (0-based, -1: none) into the handle's lane scratch, B = their right-hand sides, XT = x = G^-1 B, then theta' in place of x
int correct_chain(DcseHandle* h) {
    DC_HIP(hipMemsetAsync(h->B, 0, (size_t)h->n * h->ld * sizeof(double), h->stream));
    hipLaunchKernelGGL(k_topo_rhs, dim3((h->ld + 255) / 256), dim3(256), 0, h->stream, h->newrow, cols_of(h), rows_of(h), h->B, h->ld);
    sweep_pair(h->fac, h->stream, 0, h->B, nullptr, nullptr, h->W, h->XT, h->ld, h->ld / 64, nullptr);
    TopoApplyArgs a{h->newrow, cols_of(h), h->ws, h->R, h->t_D, h->cur, h->XT, h->n, h->ld};
    const int per = 4 * TOPO_APPLY_ROWS;
    hipLaunchKernelGGL(k_topo_apply, dim3((h->n + per - 1) / per, h->ld / 64), dim3(64, 4), 0, h->stream, a);
    DC_HIP(hipGetLastError());
    return 0;
}
int correct_setup(DcseHandle* h, const std::vector<int>& cand) {
    if (!h->XT) DC_TRY(dev_alloc(h, &h->XT, (size_t)h->n * h->ld, (const double*)nullptr, true));
    DC_HIP(sync_copy(h->newrow, cand.data(), (size_t)h->ld * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

}  // namespace

int dcse_topology_set(DcseHandle* h, long long count, const int64_t* branch, const int64_t* ptr, const int64_t* row, const int32_t* sign) {
    const char* who = "jg_dcse_topology_set";
    if (ptr[0] != 0) { h->error = std::string(who) + ": ptr is not 0-based"; return 1; }
    for (long long q = 0; q < count; ++q) {
        const std::string at = ": candidate " + std::to_string(q + 1) + " (branch " + std::to_string((long long)branch[q]) + ")";
        if (branch[q] < 1 || (h->nbr && branch[q] > h->nbr)) { h->error = who + at + ": the branch is out of range"; return 1; }
        if (ptr[q + 1] < ptr[q] || ptr[q + 1] - ptr[q] > h->m) { h->error = who + at + ": ptr is not monotone or the column is longer than the set"; return 1; }
        for (int64_t e = ptr[q]; e < ptr[q + 1]; ++e) {
            if (row[e] < 1 || row[e] > h->m) { h->error = who + at + ": row out of range"; return 1; }
            if (sign[e] != 1 && sign[e] != -1) { h->error = who + at + ": a sign must be +1 or -1"; return 1; }
            if (e > ptr[q] && row[e] <= row[e - 1]) { h->error = who + at + ": the rows of a column must be ascending and unique"; return 1; }
        }
    }
    const int64_t entries = ptr[count];
    if (entries > (1ll << 30)) { h->error = std::string(who) + ": too many entries"; return 1; }
    std::vector<int> p(count + 1), r(entries);
    std::vector<double> s(entries);
    for (long long q = 0; q <= count; ++q) p[q] = (int)ptr[q];
    for (int64_t e = 0; e < entries; ++e) { r[e] = (int)row[e] - 1; s[e] = (double)sign[e]; }
    if (h->t_count == count && p == h->h_tptr && r == h->h_trow && s == h->h_tsgn && std::equal(branch, branch + count, h->h_tbranch.begin())) return 0;     // the same candidates: the denominators stay
    h->topo_valid = false;
    h->t_count = 0;
    if (h->stream) DC_HIP(hipStreamSynchronize(h->stream));
    dev_release(h, h->t_ptr); dev_release(h, h->t_row); dev_release(h, h->t_sgn); dev_release(h, h->t_D); dev_release(h, h->t_norm); dev_release(h, h->t_stat);
    DC_TRY(dev_alloc(h, &h->t_ptr, p.size(), p.data()));
    DC_TRY(dev_alloc(h, &h->t_row, r.size(), r.data()));
    DC_TRY(dev_alloc(h, &h->t_sgn, s.size(), s.data()));
    DC_TRY(dev_alloc(h, &h->t_D, (size_t)count, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->t_norm, (size_t)count, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->t_stat, (size_t)count, (const int*)nullptr, true));
    h->h_tbranch.assign(branch, branch + count); h->h_tptr = p; h->h_trow = r; h->h_tsgn = s;
    h->h_tD.assign(count, 0.0); h->h_tnorm.assign(count, 0.0); h->h_tstat.assign(count, 2);
    h->t_count = (int)count;
    return 0;
}

int dcse_topology_denominators(DcseHandle* h) {
    DC_TRY(need_candidates(h, "jg_dcse_topology_denominators"));
    if (cache_current(h)) return 0;
    h->topo_valid = false;
    const size_t C = (size_t)h->t_count;
    {
        DenominatorPass P(h);
        DC_TRY(P.setup());
        DC_TRY(P.all());
        DC_HIP(hipMemcpyAsync(h->h_tD.data(), h->t_D, C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(hipMemcpyAsync(h->h_tnorm.data(), h->t_norm, C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(sync_copy(h->h_tstat.data(), h->t_stat, C * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    h->topo_valid = true;
    h->topo_factor = h->refactorisations;
    h->topo_runs++;
    return 0;
}

int dcse_topology_screen(DcseHandle* h, double threshold, long long capacity, double* records, long long* totals, int* lane_best, double* lane_t,
                         double* lane_phi, int* lane_count, double* dense_t) {
    const char* who = "jg_dcse_topology_screen";
    DC_TRY(need_candidates(h, who));
    DC_TRY(need_full_set_estimate(h, who));
    DC_TRY(dcse_topology_denominators(h));
    StatPass P(h);
    DC_TRY(P.setup(dense_t != nullptr));
    P.launch<false>(threshold, 0);
    DC_HIP(hipGetLastError());
    const size_t ld = (size_t)h->ld, B = (size_t)h->batch, slots = (size_t)P.chunks * P.groups;
    std::vector<int> cnt(slots), best(ld), lc(ld);
    std::vector<double> bt(ld), bphi(ld);
    DC_HIP(hipMemcpyAsync(cnt.data(), P.count, slots * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipMemcpyAsync(best.data(), P.best, ld * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipMemcpyAsync(bt.data(), P.bt, ld * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipMemcpyAsync(bphi.data(), P.bphi, ld * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(sync_copy(lc.data(), P.cnt, ld * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    long long with_hit = 0;
    for (size_t s = 0; s < B; ++s) {
        if (lane_best) lane_best[s] = best[s];
        if (lane_t) lane_t[s] = bt[s];
        if (lane_phi) lane_phi[s] = bphi[s];
        if (lane_count) lane_count[s] = lc[s];
        with_hit += lc[s] > 0;
    }
    if (dense_t) {
        std::vector<double> t((size_t)h->t_count * ld);
        DC_HIP(sync_copy(t.data(), P.dense, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        for (size_t k = 0; k < (size_t)h->t_count; ++k) std::copy(&t[k * ld], &t[k * ld] + B, dense_t + k * B);
    }
    // offsets in (group, chunk) order; the cut: through the end of the group where the running total reaches the capacity
    std::vector<long long> off(slots);
    long long total = 0, cut = 0;
    for (int g = 0; g < P.groups; ++g) {
        for (int c = 0; c < P.chunks; ++c) { off[(size_t)g * P.chunks + c] = total; total += cnt[(size_t)c * P.groups + g]; }
        if (cut < capacity) cut = total;
    }
    totals[0] = total;
    totals[1] = with_hit;
    const long long kept = std::min(total, capacity);
    if (!kept || !records) return 0;
    DC_TRY(dev_alloc(h, &P.off, slots, off.data()));
    DC_TRY(dev_alloc(h, &P.rec, (size_t)cut * 4, (const double*)nullptr, true));
    P.launch<true>(threshold, cut);
    DC_HIP(hipGetLastError());
    std::vector<double> rec((size_t)cut * 4);
    DC_HIP(sync_copy(rec.data(), P.rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    std::vector<long long> order(cut);
    std::iota(order.begin(), order.end(), 0LL);
    std::sort(order.begin(), order.end(), [&](long long x, long long y) {
        return rec[4 * x] != rec[4 * y] ? rec[4 * x] < rec[4 * y] : rec[4 * x + 1] < rec[4 * y + 1];
    });
    for (long long k = 0; k < kept; ++k) std::copy(&rec[4 * order[k]], &rec[4 * order[k]] + 4, records + 4 * k);
    return 0;
}

int dcse_topology_correct(DcseHandle* h, const int32_t* cand, double* angle) {
    const char* who = "jg_dcse_topology_correct";
    DC_TRY(need_candidates(h, who));
    DC_TRY(need_full_set_estimate(h, who));
    DC_TRY(dcse_topology_denominators(h));
    std::vector<int> c(std::max(h->ld, LDO), -1);
    for (int s = 0; s < h->batch; ++s) {
        if (cand[s] > h->t_count) { h->error = std::string(who) + ": lane " + std::to_string(s + 1) + ": candidate out of range"; return 1; }
        if (cand[s] >= 1 && h->h_tstat[cand[s] - 1] == 0) c[s] = cand[s] - 1;
    }
    DC_TRY(correct_setup(h, c));
    DC_TRY(correct_chain(h));
    const size_t ld = (size_t)h->ld, n = (size_t)h->n;
    std::vector<double> t(n * ld);
    DC_HIP(sync_copy(t.data(), h->XT, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    for (size_t s = 0; s < (size_t)h->batch; ++s) {
        for (size_t j = 0; j < n; ++j) angle[s * n + j] = t[j * ld + s] + h->slack_angle;
        angle[s * n + h->slack] = h->slack_angle;
    }
    return 0;
}

int dcse_topology_time(DcseHandle* h, int kernel, int reps, double* ms) {
    const char* who = "jg_dcse_topology_time";
    DC_TRY(need_candidates(h, who));
    if (kernel <= 3) {
        DenominatorPass P(h);
        DC_TRY(P.setup());
        if (kernel >= 2) { DC_TRY(P.rhs(0)); }
        if (kernel == 3) P.sweep();
        return time_events(h->stream, reps, ms, h->error, [&]() -> int {
            if (kernel == 0) return P.all();
            if (kernel == 1) return P.rhs(0);
            if (kernel == 2) P.sweep(); else P.finish(0);
            return 0;
        });
    }
    DC_TRY(need_full_set_estimate(h, who));
    DC_TRY(dcse_topology_denominators(h));
    if (kernel == 4) {
        StatPass P(h);
        DC_TRY(P.setup(false));
        return time_events(h->stream, reps, ms, h->error, [&]() -> int { P.launch<false>(3.0, 0); return 0; });
    }
    std::vector<int> c(std::max(h->ld, LDO), -1);
    for (int s = 0; s < h->batch; ++s)
        if (h->h_tstat[s % h->t_count] == 0) c[s] = s % h->t_count;
    DC_TRY(correct_setup(h, c));
    return time_events(h->stream, reps, ms, h->error, [&]() -> int { return correct_chain(h); });
}

}  // namespace jg

using jg::DcseHandle;
using jg::api_fail;

extern "C" {

int jg_dcse_topology_set(int64_t h, int64_t count, const int64_t* branch, const int64_t* ptr, const int64_t* row, const int32_t* sign) {
    SE_ENTER(h);
    if (count < 1 || count > (1 << 26) || !branch || !ptr || !row || !sign) return api_fail(1, "jg_dcse_topology_set: bad argument");
    DC_RET(jg::dcse_topology_set(d, count, branch, ptr, row, sign));
    return 0;
}

int jg_dcse_topology_denominators(int64_t h, double* D, double* norm, int32_t* status, int64_t* runs) {
    SE_ENTER(h);
    if (D || norm || status) DC_RET(jg::dcse_topology_denominators(d));      // runs alone: the counter, nothing is formed
    for (int k = 0; k < d->t_count; ++k) {
        if (D) D[k] = d->h_tD[k];
        if (norm) norm[k] = d->h_tnorm[k];
        if (status) status[k] = d->h_tstat[k];
    }
    if (runs) *runs = d->topo_runs;
    return 0;
}

int jg_dcse_topology_screen(int64_t h, double threshold, int64_t capacity, double* records, int64_t* totals, int32_t* lane_best, double* lane_t, double* lane_phi,
                            int32_t* lane_count, double* dense_t) {
    SE_ENTER(h);
    if (!totals || capacity < 0 || (capacity > 0 && !records) || !(threshold > 0.0)) return api_fail(1, "jg_dcse_topology_screen: bad argument");
    long long t[2] = {0, 0};
    DC_RET(jg::dcse_topology_screen(d, threshold, capacity, records, t, lane_best, lane_t, lane_phi, lane_count, dense_t));
    totals[0] = t[0]; totals[1] = t[1];
    return 0;
}

int jg_dcse_topology_correct(int64_t h, const int32_t* candidate, double* angle) {
    SE_ENTER(h);
    if (!candidate || !angle) return api_fail(1, "jg_dcse_topology_correct: null pointer");
    DC_RET(jg::dcse_topology_correct(d, candidate, angle));
    return 0;
}

int jg_dcse_topology_time(int64_t h, int kernel, int reps, double* ms) {
    SE_ENTER(h);
    if (!ms || reps < 1 || kernel < 0 || kernel > 5) return api_fail(1, "jg_dcse_topology_time: bad argument");
    DC_RET(jg::dcse_topology_time(d, kernel, reps, ms));
    return 0;
}

}  // extern "C"
