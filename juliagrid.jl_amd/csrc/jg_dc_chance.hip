// jg_dc_chance.hip -- the DC probabilistic N-1 screen under Gaussian injection uncertainty (jg_dc_chance.hpp has the algebra and the reference loop it
// stands for).
//
// Build: Phi by dc_phi_build (jg_dc_phi.hip) into a state of the screen's own; S, the row flows of the factors without the shift angle
// (dc_phi_row_flows: ONE sweep pair per factor), packed as [rows][lds]; with an injection one more column with the shift angle replaces the base flows of
// this state.  Screen of a block of candidates [k0, k1): k_chance_screen<R, MODE> (lanes = 64 consecutive candidates, each holding S[row of k, 0..R),
// f0[k] / d_k and 1 / d_k in registers; the DC_PAIR_WAVES waves of a workgroup share the chunk and each walks a quarter of the rows: the row's S, f0,
// 1 / rating and candidate position through scalar loads, Phi[m, k..k+63] one coalesced vector load; per (k, m) 2R FMAs, one sqrt, two erfc; the waves
// meet in LDS).  R in {8, 16, 32} by lds.  The records follow the protocol of jg_dc_records.hpp as the group screen does: the count IS the screen kernel's
// per-candidate count, the scatter pass is the screen kernel once more (MODE 2): sorted by (k, branch) without atomics, the first `capacity` kept, the
// totals exact.  Every store is a vector store.
#include "jg_dc_chance.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/jgrid.h"

namespace jg {

namespace {

struct ChanceArgs {
    const double* Phi; const double* f0; const double* rinv; const int* pos; const int* rbranch; const double* S;      // the rows of Phi
    const int* crow; const double* cf0; const double* cdiag; const int* clabel;                                        // the candidates
    double* worst; int* branch; int* wcnt; double* dense;       // the block: [k1 - k0], [k1 - k0], [DC_PAIR_WAVES][ldb], [3][rows][ldb] (MODE 1)
    DcRecords viol;                                              // as the call limits it
    double thr; int rows, ldk, lds, k0, k1, ldb;                 // ldb: k1 - k0 rounded up to 64
};

// P(|f| > rating) of f ~ N(mu, sigma^2), in units of the rating: ri = 1 / rating (0: unrated, P = 0)
__device__ __forceinline__ double chance_p(double mu, double sigma, double ri) {
    if (!(ri > 0.0)) return 0.0;
    const double mr = mu * ri;
    if (!(sigma > 0.0)) return fabs(mr) > 1.0 ? 1.0 : 0.0;
    const double q = 1.0 / (sigma * ri * 1.4142135623730951);
    return 0.5 * erfc((1.0 - mr) * q) + 0.5 * erfc((1.0 + mr) * q);
}

// ---- the screen kernel -------------------------------------------------------------------------------------------------------------------
// MODE 0: the summaries (worst probability, its branch, the count of P >= thr) and the counts of the record protocol.  MODE 1: also the dense mu, sigma
// and P [3][rows][ldb].  MODE 2: the scatter pass -- the same walk, a record is written at r_off[candidate] + the records of the waves before + those of
// this wave so far.  Wave w walks the rows [w q, (w + 1) q), q = rows / DC_PAIR_WAVES rounded up: ascending, so the records of a candidate ascend by branch.
template <int R, int MODE>
__global__ __launch_bounds__(64 * DC_PAIR_WAVES) void k_chance_screen(ChanceArgs a) {
    __shared__ double s_w[DC_PAIR_WAVES][64];
    __shared__ int s_i[DC_PAIR_WAVES][64], s_c[DC_PAIR_WAVES][64];
    const int wave = uniform(threadIdx.y), lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;                       // < ldb
    const int k = a.k0 + i;
    const bool live = k < a.k1;
    const int kk = live ? k : a.k0;                              // a lane behind the block reads the block's first candidate and delivers nothing
    const size_t ldk = (size_t)a.ldk, lds = (size_t)a.lds, ldb = (size_t)a.ldb;
    const bool top = R < 32 || a.lds > 24;                       // R = 32 also serves lds = 24: the last 8 of a row are then not there
    const double dk = 1.0 - a.cdiag[kk];
    const bool sing = fabs(dk) < DC_SINGULAR;
    const bool counts = live && !sing;
    const double inv = sing ? 0.0 : 1.0 / dk, c = sing ? 0.0 : a.cf0[kk] / dk;
    double sk[R];
    {
        const double* srow = a.S + (size_t)a.crow[kk] * lds;
#pragma unroll
        for (int j = 0; j < R; ++j) sk[j] = (j < 24 || top) ? srow[j] : 0.0;
    }
    const double thr = a.thr;
    const int per = (a.rows + DC_PAIR_WAVES - 1) / DC_PAIR_WAVES;
    const int r0 = wave * per, r1 = min(a.rows, r0 + per);
    long long at = 0;
    if (MODE == 2 && counts) {
        at = a.viol.r_off[i];
        for (int w = 0; w < wave; ++w) at += a.wcnt[w * ldb + i];
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int klab = a.clabel[kk];
    double wl = 0.0;
    int il = -1, cnt = 0;
    for (int r = r0; r < r1; ++r) {
        const int pk = ((CInt)a.pos)[r];
        const double f0 = ((CDbl)a.f0)[r], ri = ((CDbl)a.rinv)[r];
        if (MODE != 1 && !(ri > 0.0)) continue;                  // an unrated row enters no count and no record (wave-uniform)
        const CD4 sm = (CD4)(a.S + (size_t)r * lds);
        const double phi = a.Phi[(size_t)r * ldk + kk];
        const double g = phi * inv;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < R / 4; ++q) {
            if (q >= 6 && !top) break;
            const D4 v = sm[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double t = fma(g, sk[4 * q + e], v[e]);   // the COMBINED sensitivity, squared: never the expanded form (jg_dc_chance.hpp)
                acc = fma(t, t, acc);
            }
        }
        double mu = fma(phi, c, f0), sigma = sqrt(acc);
        if (pk == k) { mu = 0.0; sigma = 0.0; }                  // the outaged branch carries nothing, with certainty
        const double p = chance_p(mu, sigma, ri);
        const bool over = counts && p >= thr;
        if (MODE == 1 && live) {
            const size_t o = (size_t)r * ldb + i, plane = (size_t)a.rows * ldb;
            a.dense[o] = sing ? nan : mu; a.dense[plane + o] = sing ? nan : sigma; a.dense[2 * plane + o] = sing ? nan : p;
        }
        if (MODE == 2) {
            if (over) {
                if (at < a.viol.cap) {
                    double* e = (double*)a.viol.rec + at * 5;
                    e[0] = (double)klab; e[1] = (double)(((CInt)a.rbranch)[r] + 1); e[2] = mu; e[3] = sigma; e[4] = p;
                }
                ++at;
            }
        } else {
            if (p > wl) { wl = p; il = r; }                      // rows ascend by branch index, strict comparison: ties go to the lowest branch
            cnt += over ? 1 : 0;
        }
    }
    if (MODE == 2) return;
    s_w[wave][lane] = wl; s_i[wave][lane] = il; s_c[wave][lane] = cnt;
    a.wcnt[wave * ldb + i] = cnt;
    __syncthreads();
    if (wave != 0 || !live) return;
#pragma unroll
    for (int w = 1; w < DC_PAIR_WAVES; ++w) {                    // the waves' shares ascend: strict comparison keeps the lowest branch
        if (s_w[w][lane] > wl) { wl = s_w[w][lane]; il = s_i[w][lane]; }
        cnt += s_c[w][lane];
    }
    a.worst[i] = sing ? nan : wl;
    a.branch[i] = (sing || il < 0) ? 0 : a.rbranch[il] + 1;
    a.viol.r_count[i] = sing ? 0 : cnt;
}

// the base case, no outage: per row of Phi (mu, sigma, P)
__global__ void k_chance_base(const double* f0, const double* S, const double* rinv, double* base, int rows, int lds) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double acc = 0.0;
    for (int j = 0; j < lds; ++j) { const double t = S[(size_t)r * lds + j]; acc = fma(t, t, acc); }
    const double mu = f0[r], sigma = sqrt(acc);
    double* q = base + (size_t)r * 3;
    q[0] = mu; q[1] = sigma; q[2] = chance_p(mu, sigma, rinv[r]);
}

// S [rows][lds] out of the row flows F [rows][ldf] of the r factors: zeros behind r
__global__ void k_chance_pack(const double* F, double* S, int rows, int ldf, int lds, int r) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)rows * lds) return;
    const int row = (int)(t / lds), j = (int)(t % lds);
    S[t] = j < r ? F[(size_t)row * ldf + j] : 0.0;
}
// the base flows of an injection of the build's own: column 0 of F into row_f0, then cand_f0 from it
__global__ void k_chance_row_f0(const double* F, double* f0, int rows, int ldf) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) f0[r] = F[(size_t)r * ldf];
}
__global__ void k_chance_cand_f0(const double* f0, const int* crow, double* cf0, int nk, int ldk) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < ldk) cf0[j] = j < nk ? f0[crow[j]] : 0.0;
}

// ---- the build ------------------------------------------------------------------------------------------------------------------------------
// factors [r][n]; base_rhs [n] nullable: the right-hand side of an injection as jg_dc_set_rhs takes it
int chance_build(DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, int r, const double* factors, const double* base_rhs, int64_t budget,
                 double* info) {
    dc_state_release(h, h->chance);
    DcChanceState* s = h->chance = new DcChanceState();
    const int lds = (r + 7) / 8 * 8, ldf = 64;                   // ldf: one lane batch of 64 lanes holds every factor (DC_CHANCE_MAX <= 64)
    s->r = r; s->lds = lds;
    {                                                            // the rows of Phi are monitored u candidates, ascending (dc_phi_build)
        std::vector<char> is_mon(h->nbr, 0), is_cand(h->nbr, 0);
        for (int m : mon) is_mon[m] = 1;
        for (int m : cand) is_cand[m] = 1;
        int row = 0;
        for (int m = 0; m < h->nbr; ++m)
            if (is_mon[m] || is_cand[m]) { if (is_mon[m]) s->h_mon_row.push_back(row); ++row; }
    }
    const size_t nr = dc_phi_row_labels(h, cand, mon, lds, info).size();       // info [8]: the bytes of S
    const size_t s_bytes = (size_t)info[8], scratch = dc_phi_flows_scratch(h, ldf) + nr * ldf * sizeof(double);
    const std::string extra = "; S needs " + dc_bytes_text(s_bytes) + " (" + std::to_string(nr) + " rows x " + std::to_string(lds) + " factors x 8) and " +
                              dc_bytes_text(scratch) + " of scratch";
    DcPhi* p = &s->phi;
    int rc = 0;
    auto step = [&](int q) { if (q && !rc) rc = q; return rc == 0; };
    auto launched = [&] { return step(dc_hip(h, hipGetLastError(), "launch")); };
    double ms[2] = {0.0, 0.0}, unused[2] = {0.0, 0.0};
    double* F = nullptr;                                         // [nr][ldf] the row flows as dc_phi_row_flows lays them out
    if (step(dc_phi_build(h, p, "jg_dc_chance_build", cand, mon, budget, s_bytes + nr * 3 * sizeof(double) + scratch, extra, info)) &&
        step(dev_alloc(h, s->mem, &s->S, nr * lds, (const double*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->base, nr * 3, (const double*)nullptr, true)) &&
        step(dev_alloc(h, s->mem, &F, nr * ldf, (const double*)nullptr, true)) && step(dc_phi_row_flows(h, p, r, factors, false, F, ldf, ms))) {
        hipLaunchKernelGGL(k_chance_pack, dim3((unsigned)((nr * lds + 255) / 256)), dim3(256), 0, h->stream, F, s->S, (int)nr, ldf, lds, r);
        if (launched() && base_rhs && step(dc_phi_row_flows(h, p, 1, base_rhs, true, F, ldf, unused))) {
            hipLaunchKernelGGL(k_chance_row_f0, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, h->stream, F, p->row_f0, (int)nr, ldf);
            hipLaunchKernelGGL(k_chance_cand_f0, dim3((p->ldk + 255) / 256), dim3(256), 0, h->stream, p->row_f0, p->cand_row, p->cand_f0, p->nk, p->ldk);
            launched();
        }
        step(dc_hip(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize")) && step(dc_phi_bridges(h, p, s->h_bridge));
    }
    dev_release(h, s->mem, F);
    if (rc) return dc_build_failed(h, h->chance, rc);
    dc_phi_flows_ms(ms, s->build_ms, info);
    return 0;
}

// the block's buffers for `rb` candidates (and the dense results, on request: kept once allocated); grown, never shrunk
int chance_block(DcHandle* h, int rb, bool want_dense, long long rec_cap) {
    DcChanceState* s = h->chance;
    if (rb > s->blk_rows || (want_dense && !s->b_dense)) {
        const int n = std::max(rb, s->blk_rows);
        const bool dense = want_dense || s->b_dense != nullptr;
        const size_t ld = ((size_t)n + 63) / 64 * 64, cells = (size_t)s->phi.rows * ld * 3;
        DC_TRY(dc_block_grow(h, s->mem, "jg_dc_chance_screen", n, s->blk_rows, (size_t)n * 24 + ld * DC_PAIR_WAVES * 4 + (dense ? cells * 8 : 0), {&s->viol},
                             dc_blk(s->b_worst, (size_t)n), dc_blk(s->b_branch, (size_t)n), dc_blk(s->b_wcnt, ld * DC_PAIR_WAVES), dc_blk(s->b_dense, dense ? cells : 0)));
    }
    return dc_list_grow(h, s->mem, s->viol, rec_cap);
}

ChanceArgs screen_args(DcHandle* h, int k0, int k1, double thr, long long rec_cap) {
    DcChanceState* s = h->chance;
    const DcPhi* p = &s->phi;
    ChanceArgs a{};
    a.Phi = p->Phi; a.f0 = p->row_f0; a.rinv = p->row_rinv; a.pos = p->row_pos; a.rbranch = p->row_branch; a.S = s->S;
    a.crow = p->cand_row; a.cf0 = p->cand_f0; a.cdiag = p->cand_diag; a.clabel = p->cand_label;
    a.worst = s->b_worst; a.branch = s->b_branch; a.wcnt = s->b_wcnt; a.dense = s->b_dense;
    a.viol = s->viol.limited(rec_cap);
    a.thr = thr; a.rows = p->rows; a.ldk = p->ldk; a.lds = s->lds; a.k0 = k0; a.k1 = k1; a.ldb = (k1 - k0 + 63) / 64 * 64;
    return a;
}
template <int MODE>
void launch_screen(DcHandle* h, const ChanceArgs& a) {
    const dim3 grid(a.ldb / 64), block(64, DC_PAIR_WAVES);
    if (a.lds <= 8) hipLaunchKernelGGL((k_chance_screen<8, MODE>), grid, block, 0, h->stream, a);
    else if (a.lds <= 16) hipLaunchKernelGGL((k_chance_screen<16, MODE>), grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL((k_chance_screen<DC_CHANCE_MAX, MODE>), grid, block, 0, h->stream, a);
}
void launch_base(DcHandle* h) {
    DcChanceState* s = h->chance;
    hipLaunchKernelGGL(k_chance_base, dim3((s->phi.rows + 63) / 64), dim3(64), 0, h->stream, s->phi.row_f0, s->S, s->phi.row_rinv, s->base, s->phi.rows, s->lds);
}

struct ChanceOut {
    double* records; int64_t* totals; double* worst; int32_t* branch; int32_t* count; int32_t* status; double* mu; double* sigma; double* p;
};
int chance_screen(DcHandle* h, int k0, int k1, double thr, long long rec_cap, const ChanceOut& o) {
    DcChanceState* s = h->chance;
    const int rb = k1 - k0;
    const bool dense = o.mu || o.sigma || o.p;
    DC_TRY(chance_block(h, rb, dense, rec_cap));
    dc_phi_rinv(h, &s->phi);
    const ChanceArgs a = screen_args(h, k0, k1, thr, rec_cap);
    if (dense) launch_screen<1>(h, a);
    else launch_screen<0>(h, a);
    std::vector<double> worst(rb);
    std::vector<int> branch(rb);
    DcListCall viol{&s->viol, rec_cap, o.records};
    DC_TRY(dc_block_records(h, rb, {&viol}, [&] {
        DC_HIP(hipMemcpyAsync(worst.data(), s->b_worst, rb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(sync_copy(branch.data(), s->b_branch, rb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        return 0;
    }, [&] { launch_screen<2>(h, a); }));
    long long bridges = 0;
    for (int i = 0; i < rb; ++i) {
        const bool b = s->h_bridge[k0 + i] != 0;
        bridges += b ? 1 : 0;
        if (o.status) o.status[i] = b ? 3 : 0;
        if (o.worst) o.worst[i] = worst[i];
        if (o.branch) o.branch[i] = branch[i];
        if (o.count) o.count[i] = viol.count[i];
    }
    o.totals[0] = (long long)rb; o.totals[1] = viol.total; o.totals[2] = bridges; o.totals[3] = viol.kept; o.totals[4] = viol.total > rec_cap ? 1 : 0;
    if (dense) {                                                 // the device's [3][rows][ldb] as [rb][monitored] each
        const size_t ldb = (size_t)a.ldb, nm = s->h_mon_row.size(), plane = (size_t)s->phi.rows * ldb;
        std::vector<double> t(plane * 3);
        DC_HIP(sync_copy(t.data(), s->b_dense, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        double* const out[3] = {o.mu, o.sigma, o.p};
        for (int q = 0; q < 3; ++q)
            if (out[q])
                for (int i = 0; i < rb; ++i)
                    for (size_t j = 0; j < nm; ++j) out[q][(size_t)i * nm + j] = t[q * plane + (size_t)s->h_mon_row[j] * ldb + i];
    }
    return 0;
}

}  // namespace

void dc_chance_free(DcHandle* h) { dc_state_release(h, h->chance); }

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_chance_build(int64_t h, int64_t r, const double* factors, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored,
                       const double* injection_rhs, int64_t budget_bytes, double* info) {
    DC_ENTER(h);
    const std::string me = "jg_dc_chance_build: ";
    if (!d->nbr) return api_fail(1, me + "jg_dc_set_branches first");
    if (d->h_rhs.empty()) return api_fail(1, me + "jg_dc_set_rhs first");
    if (r < 1 || r > jg::DC_CHANCE_MAX)
        return api_fail(1, me + std::to_string(r) + " factors: 1 to " + std::to_string(jg::DC_CHANCE_MAX) + " are screened (truncate the covariance's factorisation)");
    if (!factors || nk < 1 || !candidates || !info || nm < 0 || (nm && !monitored)) return api_fail(1, me + "factors, one or more candidates, and info, are needed");
    std::vector<int> cand, mon;
    DC_RET(jg::dc_phi_lists(d, "jg_dc_chance_build", nk, candidates, nm, monitored, cand, mon));
    DC_RET(jg::chance_build(d, cand, mon, (int)r, factors, injection_rhs, budget_bytes, info));
    return 0;
}

int jg_dc_chance_screen(int64_t h, int64_t k0, int64_t k1, double probability, int64_t capacity, double* records, int64_t* totals, double* worst,
                        int32_t* worst_branch, int32_t* count, int32_t* status, double* dense_mu, double* dense_sigma, double* dense_p) {
    DC_ENTER(h);
    if (!d->chance) return api_fail(4, "jg_dc_chance_screen: jg_dc_chance_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_chance_screen: jg_dc_set_rating first (the probabilities are those of |from| > rating)");
    if (k0 < 0 || k1 <= k0 || k1 > d->chance->phi.nk) return api_fail(1, "jg_dc_chance_screen: rows [k0, k1) out of range");
    if (!(probability > 0.0 && probability <= 1.0) || capacity < 0 || (capacity && !records) || !totals)
        return api_fail(1, "jg_dc_chance_screen: bad argument (0 < probability <= 1)");
    jg::ChanceOut o{records, totals, worst, worst_branch, count, status, dense_mu, dense_sigma, dense_p};
    DC_RET(jg::chance_screen(d, (int)k0, (int)k1, probability, capacity, o));
    return 0;
}

int jg_dc_chance_get_dims(int64_t h, int64_t* dims) {
    DC_ENTER(h);
    if (!d->chance) return api_fail(4, "jg_dc_chance_get_dims: jg_dc_chance_build first");
    if (!dims) return api_fail(1, "jg_dc_chance_get_dims: null pointer");
    const jg::DcChanceState* s = d->chance;
    dims[0] = s->phi.nk; dims[1] = s->phi.ldk; dims[2] = s->phi.rows; dims[3] = (int64_t)s->h_mon_row.size(); dims[4] = s->r; dims[5] = s->lds;
    return 0;
}

int jg_dc_chance_get_base(int64_t h, double* mean, double* std_dev, double* probability) {
    DC_ENTER(h);
    if (!d->chance) return api_fail(4, "jg_dc_chance_get_base: jg_dc_chance_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_chance_get_base: jg_dc_set_rating first");
    jg::DcChanceState* s = d->chance;
    jg::dc_phi_rinv(d, &s->phi);
    jg::launch_base(d);
    DC_API_HIP(hipGetLastError());
    std::vector<double> t((size_t)s->phi.rows * 3);
    DC_API_HIP(jg::sync_copy(t.data(), s->base, t.size() * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    for (size_t j = 0; j < s->h_mon_row.size(); ++j) {
        const double* q = t.data() + (size_t)s->h_mon_row[j] * 3;
        if (mean) mean[j] = q[0];
        if (std_dev) std_dev[j] = q[1];
        if (probability) probability[j] = q[2];
    }
    return 0;
}

int jg_dc_chance_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms) {
    DC_ENTER(h);
    jg::DcChanceState* s = d->chance;
    return jg::dc_phi_time_kernel(d, "chance", s ? &s->phi : nullptr, s ? s->blk_rows : 0, kernel, k0, k1, reps, ms,
                                  [&] {
        return [d, a = jg::screen_args(d, (int)k0, (int)k1, 1.0, 0)](int which) {
            if (which == 0) jg::launch_screen<0>(d, a);
            else jg::launch_base(d);
        };
    });
}

int jg_dc_chance_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_chance_free(d);
    return 0;
}

}  // extern "C"
