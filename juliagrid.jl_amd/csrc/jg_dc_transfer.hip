// jg_dc_transfer.hip -- the DC transfer-capability screen over transfers x N-1 outages (jg_dc_transfer.hpp has the algebra and the reference loop it
// stands for).
//
// Build: Phi by the build the three screens share (dc_phi_build, jg_dc_phi.hip), into a state of the screen's own; then G, the row flows of the
// directions without the shift angle (dc_phi_row_flows: the sweep pair of jg_dc_sweep.hip, DC_PAIR_LANES directions at a time); the base flows
// are the build's own, or one more such batch of one lane for a base profile.  Screen of a row block [k0, k1): k_transfer_screen walks the rows once (lanes
// = 64 consecutive candidates k of a chunk, a wave keeps DC_TRANSFER_TILE transfers in registers, the waves of a workgroup share the chunk so its Phi rows
// meet in the vector L1; 1 / rating_m, F0[m], the row's candidate position and G[m, t..t+3] through scalar loads, Phi[m, k..k+63] one coalesced vector load
// reused for every transfer of the tile; nothing is written per m).  The summaries come out of the block's dense result without atomics: per candidate and
// per transfer minima, the records by k_dc_rows and dc_block_records (jg_dc_records.hpp has the protocol) under the policy TransferRows, sorted by (k, t).
// Every store is a vector store.
#include "jg_dc_transfer.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "../../include/jgrid.h"

namespace jg {

namespace {

// sign(g) x: the sign bit of g flips x
__device__ __forceinline__ double flip_by(double x, double g) {
    return __longlong_as_double(__double_as_longlong(x) ^ (__double_as_longlong(g) & (long long)0x8000000000000000ull));
}
// One row against the running minimum (bn / bd, br) of a case, in loading space: fl = f rinv (signed), g the sensitivity, ri = rinv (0: not monitored or not
// rated).  limit = (1 - sign(g) fl) / (|g| ri); an ineligible row is (1, 0) = +inf and never wins; strict comparison, rows ascending.
__device__ __forceinline__ void transfer_row(double fl, double g, double ri, bool eligible, double cutoff, int r, double& bn, double& bd, int& br) {
    const double ag = fabs(g);
    const bool el = eligible && ag > cutoff;
    const double num = el ? 1.0 - flip_by(fl, g) : 1.0;
    const double den = el ? ag * ri : 0.0;
    if (num * bd < bn * den) { bn = num; bd = den; br = r; }
}
__device__ __forceinline__ double transfer_limit(double bn, double bd) { return bd > 0.0 ? bn / bd : __longlong_as_double(0x7ff0000000000000LL); }

// ---- the screen kernel -------------------------------------------------------------------------------------------------------------------
struct TransferScreenArgs {
    const double* Phi; const double* G; const double* f0; const double* rinv; const int* pos;
    const int* crow; const double* cdiag;
    double* tc; int* row;                                       // [k1 - k0][ldt]
    double cutoff; int rows, ldk, ldt, T, k0, k1, kbase;        // kbase: k0 rounded down to a multiple of 64 (a chunk's row of Phi is one aligned 512-byte load)
    const int* cisl; const int* rpre;                            // SHED: the candidates' (side, lo, hi, 0) and the rows' preorder[from]
};
// SHED (a screen built in shed mode): a bridge candidate's column of Phi holds Z[:,k], its coefficients are s_k F0[k] and s_k G[k,t] without a denominator,
// and a row whose from end lies in its preorder interval left with it: ineligible, (1, 0).  The row's number is a scalar load, the interval sits in the lane.
template <bool SHED>
__global__ __launch_bounds__(64 * DC_PAIR_WAVES) void k_transfer_screen(TransferScreenArgs a) {
    constexpr int K = DC_TRANSFER_TILE;
    const int wave = uniform(threadIdx.y);
    const int t0 = (blockIdx.y * DC_PAIR_WAVES + wave) * K;     // < ldt: G is [rows][ldt], 0 behind T
    if (t0 >= a.T) return;
    const int c0 = a.kbase + blockIdx.x * 64;
    const int k = c0 + threadIdx.x;                             // < ldk: the per-candidate arrays are [ldk], 0 behind nk; so are the columns of Phi
    const size_t ldk = (size_t)a.ldk, ldt = (size_t)a.ldt;
    const double dk = 1.0 - a.cdiag[k];
    const int rk = a.crow[k];
    bool sing = fabs(dk) < DC_SINGULAR;
    double cf = sing ? 0.0 : a.f0[rk] / dk;
    double cg[K], bn[K], bd[K];
    int br[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        cg[i] = sing ? 0.0 : a.G[(size_t)rk * ldt + t0 + i] / dk;
        bn[i] = 1.0; bd[i] = 0.0; br[i] = -1;
    }
    int lo = 1, hi = 0;
    if constexpr (SHED) {
        const I4 q = ((const I4*)a.cisl)[k];
        lo = q[1]; hi = q[2];
        if (q[0] != 0) {                                         // what left m over the bridge: at zero transfer, and per unit of each transfer
            const double sk = q[0] > 0 ? 1.0 : -1.0;
            sing = false;
            cf = sk * a.f0[rk];
#pragma unroll
            for (int i = 0; i < K; ++i) cg[i] = sk * a.G[(size_t)rk * ldt + t0 + i];
        }
    }
    const double cutoff = a.cutoff;
    const double* pcol = a.Phi + k;
    auto row = [&](int r, int pk, auto hit_c) {
        constexpr bool HIT = decltype(hit_c)::value;
        const double ri = ((CDbl)a.rinv)[r], fr = ((CDbl)a.f0)[r];
        const D4 g4 = *(CD4)(a.G + (size_t)r * ldt + t0);
        const double ph = pcol[(size_t)r * ldk];
        const double fl = fma(ph, cf, fr) * ri;
        bool other = !(HIT && pk == k);                         // the outaged branch limits nothing
        if constexpr (SHED) {
            const int pr = ((CInt)a.rpre)[r];
            other = other && !(pr >= lo && pr <= hi);            // nor does a branch that left with the bridge
        }
#pragma unroll
        for (int i = 0; i < K; ++i) transfer_row(fl, fma(ph, cg[i], g4[i]), ri, other, cutoff, r, bn[i], bd[i], br[i]);
    };
    for (int r = 0; r < a.rows; ++r) {
        const int pk = ((CInt)a.pos)[r];
        // only a row whose branch is one of this chunk's own candidates (at most 64 of the rows) needs the test per lane
        if ((unsigned)(pk - c0) < 64u) row(r, pk, std::true_type{});
        else row(r, pk, std::false_type{});
    }
    if (k < a.k0 || k >= a.k1) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int t = t0 + i;
        if (t >= a.T) continue;
        const size_t o = (size_t)(k - a.k0) * ldt + t;
        a.tc[o] = sing ? nan : transfer_limit(bn[i], bd[i]);
        a.row[o] = sing ? -1 : br[i];
    }
}

// ---- summaries out of the block's dense result: the transfer screen's policy of k_dc_rows (jg_dc_records.hpp) ------------------------------------
// Row k's columns are the transfers 0 .. T; one list, the cases with TC < amount[t] (a NaN, the capability of a bridge candidate, compares false); the
// row's minimum from +inf.  A record carries g of the limiting branch, formed as the screen kernel forms it; a case without one (+inf below an infinite
// amount) takes its slot and is not written.
struct TransferRows {
    static constexpr int LISTS = 1;
    const double* tc; const int* row; const double* amount; const int* clabel; const int* rbranch;
    const double* Phi; const double* G; const int* crow; const double* cdiag; const int* cisl;      // cisl: shed mode (else null), the candidates' (side, lo, hi, 0)
    DcRecords list[1]; double* r_red;
    int ldk, ldt, T, k0, k1;
    __device__ int first(int) const { return 0; }
    __device__ int cols() const { return T; }
    __device__ bool valid(int, int t) const { return t < T; }
    __device__ double value(int i, int t) const { return tc[(size_t)i * ldt + t]; }
    __device__ bool hit(int, double v, int t) const { return v < amount[t]; }
    __device__ void write(int, long long at, int klab, int i, int k, int t, double v) const {
        const int r = row[(size_t)i * ldt + t];
        if (r < 0) return;
        const int rk = crow[k];
        const int sd = cisl ? cisl[4 * k] : 0;
        const double cgk = sd ? (sd > 0 ? 1.0 : -1.0) * G[(size_t)rk * ldt + t] : G[(size_t)rk * ldt + t] / (1.0 - cdiag[k]);
        const double g = fma(Phi[(size_t)r * ldk + k], cgk, G[(size_t)r * ldt + t]);
        double* e = (double*)list[0].rec + at * 5;
        e[0] = (double)klab; e[1] = (double)t; e[2] = (double)(rbranch[r] + 1); e[3] = v; e[4] = g;
    }
    static __device__ double identity() { return __longlong_as_double(0x7ff0000000000000LL); }
    static __device__ bool better(double v, double m) { return v < m; }
    static __device__ double combine(double x, double y) { return fmin(x, y); }
};
// per transfer over the block's candidates, rows ascending and strict: the least capability (bridges aside), the block row that gives it (-1: none), its limiting row
__global__ void k_transfer_cols(const double* tc, const int* row, double* c_min, int* c_at, int* c_row, int ldt, int T, int rb) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ldt) return;
    double mn = __longlong_as_double(0x7ff0000000000000LL);
    int at = -1;
    if (t < T)
        for (int i = 0; i < rb; ++i) {
            const double v = tc[(size_t)i * ldt + t];
            if (v < mn) { mn = v; at = i; }
        }
    c_min[t] = mn; c_at[t] = at; c_row[t] = at < 0 ? -1 : row[(size_t)at * ldt + t];
}
// the base case of every transfer (no outage): the capability, its limiting row (-1: none), monitored branches above their rating at zero transfer
__global__ void k_transfer_base(const double* G, const double* f0, const double* rinv, double* base, double cutoff, int rows, int ldt, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    double bn = 1.0, bd = 0.0;
    int br = -1, cnt = 0;
    for (int r = 0; r < rows; ++r) {
        const double ri = ((CDbl)rinv)[r];
        const double fl = ((CDbl)f0)[r] * ri;
        transfer_row(fl, G[(size_t)r * ldt + t], ri, true, cutoff, r, bn, bd, br);
        cnt += fabs(fl) > 1.0 ? 1 : 0;
    }
    double* q = base + (size_t)t * 3;
    q[0] = transfer_limit(bn, bd); q[1] = (double)br; q[2] = (double)cnt;
}
// the base flows of a base profile: lane 0 of its one lane batch
__global__ void k_transfer_pick(const double* F, double* f0, int rows, int ld) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) f0[r] = F[(size_t)r * ld];
}

// dirs [T][n]: net injection per unit of transfer; base_rhs [n] nullable: the right-hand side of a base profile as jg_dc_set_rhs takes it
int transfer_build(DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, int T, const double* dirs, const double* base_rhs, int64_t budget,
                   double* info) {
    dc_state_release(h, h->transfer);
    const bool shed = h->transfer_shed == 1;
    h->transfer_shed = 0;
    const int ldt = (T + 63) / 64 * 64;
    const std::vector<int> label = dc_phi_row_labels(h, cand, mon, ldt, info);
    const int nr = (int)label.size();
    const size_t g_bytes = (size_t)info[8];
    const size_t scratch = dc_phi_flows_scratch(h, ldt) + (base_rhs ? (size_t)nr * 64 * sizeof(double) : 0);
    DcTransferState* s = h->transfer = new DcTransferState();
    s->T = T; s->ldt = ldt; s->h_row_label = label;
    const std::string extra = "; G needs " + dc_bytes_text(g_bytes) + " (" + std::to_string(nr) + " rows x " + std::to_string(ldt) + " transfers x 8) and " +
                              dc_bytes_text(scratch) + " of scratch";
    DcPhi* p = &s->phi;
    int rc = 0;
    auto step = [&](int r) { if (r && !rc) rc = r; return rc == 0; };
    double ms[2] = {0.0, 0.0};
    if (step(dc_phi_build(h, p, "jg_dc_transfer_build", cand, mon, budget, g_bytes + scratch, extra, info, shed)) &&
        step(dev_alloc(h, s->mem, &s->G, (size_t)nr * ldt, (const double*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->f0, (size_t)nr, (const double*)nullptr, true)) &&
        step(dev_alloc(h, s->mem, &s->c_min, (size_t)ldt, (const double*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->c_at, (size_t)ldt, (const int*)nullptr, true)) &&
        step(dev_alloc(h, s->mem, &s->c_row, (size_t)ldt, (const int*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->amount, (size_t)ldt, (const double*)nullptr, true)) &&
        step(dev_alloc(h, s->mem, &s->base, (size_t)ldt * 3, (const double*)nullptr, true))) {
        if (base_rhs) {
            double* Fb = nullptr;                                // [nr][64]: one lane batch of one lane
            double unused[2] = {0.0, 0.0};
            if (step(dev_alloc(h, s->mem, &Fb, (size_t)nr * 64, (const double*)nullptr, true)) && step(dc_phi_row_flows(h, p, 1, base_rhs, true, Fb, 64, unused))) {
                hipLaunchKernelGGL(k_transfer_pick, dim3((nr + 255) / 256), dim3(256), 0, h->stream, Fb, s->f0, nr, 64);
                step(dc_hip(h, hipGetLastError(), "launch")) && step(dc_hip(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize"));
            }
            dev_release(h, s->mem, Fb);
        } else {
            step(dc_hip(h, sync_copy(s->f0, p->row_f0, (size_t)nr * sizeof(double), hipMemcpyDeviceToDevice, h->stream), "copy of the base flows"));
        }
        if (!rc) step(dc_phi_row_flows(h, p, T, dirs, false, s->G, ldt, ms));
        if (!rc) step(dc_phi_bridges(h, p, s->h_bridge));
    }
    if (rc) return dc_build_failed(h, h->transfer, rc);
    dc_phi_flows_ms(ms, s->build_ms, info);
    return 0;
}

// the block's buffers for `rb` rows; grown, never shrunk
int transfer_block(DcHandle* h, int rb, long long rec_cap) {
    DcTransferState* s = h->transfer;
    if (rb > s->blk_rows) {
        const size_t cells = (size_t)rb * s->ldt, r = (size_t)rb;
        DC_TRY(dc_block_grow(h, s->mem, "jg_dc_transfer_screen", rb, s->blk_rows, cells * 12, {&s->below}, dc_blk(s->b_tc, cells), dc_blk(s->b_row, cells), dc_blk(s->r_min, r)));
    }
    return dc_list_grow(h, s->mem, s->below, rec_cap);
}

TransferScreenArgs screen_args(DcHandle* h, int k0, int k1, double cutoff) {
    DcTransferState* s = h->transfer;
    const DcPhi* p = &s->phi;
    TransferScreenArgs a{};
    a.Phi = p->Phi; a.G = s->G; a.f0 = s->f0; a.rinv = p->row_rinv; a.pos = p->row_pos; a.crow = p->cand_row; a.cdiag = p->cand_diag;
    a.tc = s->b_tc; a.row = s->b_row;
    a.cutoff = cutoff; a.rows = p->rows; a.ldk = p->ldk; a.ldt = s->ldt; a.T = s->T; a.k0 = k0; a.k1 = k1; a.kbase = k0 / 64 * 64;
    a.cisl = p->shed ? p->cand_isl : nullptr; a.rpre = p->shed ? p->row_pre : nullptr;
    return a;
}
void launch_screen(DcHandle* h, const TransferScreenArgs& a) {
    const int tiles = (a.T + DC_TRANSFER_TILE - 1) / DC_TRANSFER_TILE;
    const dim3 grid((a.k1 - a.kbase + 63) / 64, (tiles + DC_PAIR_WAVES - 1) / DC_PAIR_WAVES), block(64, DC_PAIR_WAVES);
    if (a.cisl) hipLaunchKernelGGL(k_transfer_screen<true>, grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL(k_transfer_screen<false>, grid, block, 0, h->stream, a);
}
TransferRows list_args(DcHandle* h, int k0, int k1, long long rec_cap) {
    DcTransferState* s = h->transfer;
    const DcPhi* p = &s->phi;
    TransferRows a{};
    a.tc = s->b_tc; a.row = s->b_row; a.amount = s->amount; a.clabel = p->cand_label; a.rbranch = p->row_branch;
    a.Phi = p->Phi; a.G = s->G; a.crow = p->cand_row; a.cdiag = p->cand_diag; a.cisl = p->shed ? p->cand_isl : nullptr;
    a.list[0] = s->below.limited(rec_cap); a.r_red = s->r_min;
    a.ldk = p->ldk; a.ldt = s->ldt; a.T = s->T; a.k0 = k0; a.k1 = k1;
    return a;
}
void launch_stats(DcHandle* h, const TransferRows& a) {
    DcTransferState* s = h->transfer;
    dc_launch_rows<false>(h, a);
    hipLaunchKernelGGL(k_transfer_cols, dim3((s->ldt + 255) / 256), dim3(256), 0, h->stream, s->b_tc, s->b_row, s->c_min, s->c_at, s->c_row, s->ldt, s->T, a.k1 - a.k0);
}

struct TransferOut {
    const double* amount; double* records; int64_t* islanding; int64_t* totals; double* worst;
    double* capability; int64_t* cap_outage; int64_t* cap_branch; double* base;
    double* d_tc; int32_t* d_branch;
};
int transfer_screen(DcHandle* h, int k0, int k1, double cutoff, long long rec_cap, const TransferOut& o) {
    DcTransferState* s = h->transfer;
    DcPhi* p = &s->phi;
    const int rb = k1 - k0, T = s->T, ldt = s->ldt;
    const double inf = std::numeric_limits<double>::infinity();
    DC_TRY(transfer_block(h, rb, rec_cap));
    {
        std::vector<double> am(ldt, -inf);                       // no amount: nothing lies below it, no records
        if (o.amount) std::copy(o.amount, o.amount + T, am.begin());
        DC_HIP(sync_copy(s->amount, am.data(), (size_t)ldt * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    dc_phi_rinv(h, p);
    launch_screen(h, screen_args(h, k0, k1, cutoff));
    const TransferRows la = list_args(h, k0, k1, rec_cap);
    launch_stats(h, la);
    if (o.base) hipLaunchKernelGGL(k_transfer_base, dim3((T + 63) / 64), dim3(64), 0, h->stream, s->G, s->f0, p->row_rinv, s->base, cutoff, p->rows, ldt, T);
    std::vector<int> cat(ldt), crow(ldt);
    std::vector<double> rmin(rb), cmin(ldt), base(o.base ? (size_t)T * 3 : 0);
    DcListCall below{&s->below, rec_cap, o.records};
    DC_TRY(dc_block_records(h, rb, {&below}, [&] {
        DC_HIP(hipMemcpyAsync(rmin.data(), s->r_min, rb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(hipMemcpyAsync(cat.data(), s->c_at, ldt * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(hipMemcpyAsync(crow.data(), s->c_row, ldt * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (o.base) DC_HIP(hipMemcpyAsync(base.data(), s->base, (size_t)T * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(sync_copy(cmin.data(), s->c_min, ldt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        return 0;
    }, [&] { dc_launch_rows<true>(h, la); }));
    o.totals[0] = (long long)rb * T; o.totals[1] = below.total; o.totals[2] = dc_bridge_list(*p, s->h_bridge, k0, k1, o.islanding); o.totals[3] = below.kept;
    o.totals[4] = below.total > rec_cap ? 1 : 0;
    if (o.worst) for (int i = 0; i < rb; ++i) o.worst[k0 + i] = s->h_bridge[k0 + i] ? std::numeric_limits<double>::quiet_NaN() : rmin[i];
    if (o.capability && o.cap_outage && o.cap_branch)
        for (int t = 0; t < T; ++t)
            if (cmin[t] < o.capability[t]) {                    // strict, blocks ascending: the first candidate that gives the least value, whatever the block size
                o.capability[t] = cmin[t]; o.cap_outage[t] = p->h_cand[k0 + cat[t]] + 1; o.cap_branch[t] = crow[t] < 0 ? 0 : s->h_row_label[crow[t]];
            }
    if (o.base)
        for (int t = 0; t < T; ++t) {
            const int r = (int)base[(size_t)t * 3 + 1];
            o.base[(size_t)t * 3] = base[(size_t)t * 3]; o.base[(size_t)t * 3 + 1] = r < 0 ? 0.0 : (double)s->h_row_label[r]; o.base[(size_t)t * 3 + 2] = base[(size_t)t * 3 + 2];
        }
    if (o.d_tc) DC_TRY(dc_dense(h, o.d_tc, (const double*)s->b_tc, rb, ldt, T, [](int, int, double v) { return v; }));
    if (o.d_branch) DC_TRY(dc_dense(h, o.d_branch, (const int*)s->b_row, rb, ldt, T, [s](int, int, int r) { return r < 0 ? 0 : s->h_row_label[r]; }));    // a row's label
    return 0;
}

}  // namespace

void dc_transfer_free(DcHandle* h) { dc_state_release(h, h->transfer); }

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_transfer_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t transfers, const double* directions,
                         const double* base_rhs, int64_t budget_bytes, double* info) {
    DC_ENTER(h);
    if (!d->nbr) return api_fail(1, "jg_dc_transfer_build: jg_dc_set_branches first");
    if (d->h_rhs.empty()) return api_fail(1, "jg_dc_transfer_build: jg_dc_set_rhs first");
    if (nk < 1 || !candidates || !info || nm < 0 || (nm && !monitored)) return api_fail(1, "jg_dc_transfer_build: one or more candidates, and info, are needed");
    if (transfers < 1 || transfers > (1 << 24) || !directions) return api_fail(1, "jg_dc_transfer_build: one or more transfer directions are needed");
    std::vector<int> cand, mon;
    DC_RET(jg::dc_phi_lists(d, "jg_dc_transfer_build", nk, candidates, nm, monitored, cand, mon));
    DC_RET(jg::transfer_build(d, cand, mon, (int)transfers, directions, base_rhs, budget_bytes, info));
    return 0;
}

int jg_dc_transfer_screen(int64_t h, int64_t k0, int64_t k1, double cutoff, const double* amount, int64_t capacity, double* records, int64_t* islanding,
                          int64_t* totals, double* worst, double* capability, int64_t* limiting_outage, int64_t* limiting_branch, double* base,
                          double* dense_capability, int32_t* dense_branch) {
    DC_ENTER(h);
    if (!d->transfer) return api_fail(4, "jg_dc_transfer_screen: jg_dc_transfer_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_transfer_screen: jg_dc_set_rating first (a branch limits at |from| = rating)");
    if (k0 < 0 || k1 <= k0 || k1 > d->transfer->phi.nk) return api_fail(1, "jg_dc_transfer_screen: rows [k0, k1) out of range");
    if (!(cutoff > 0.0) || capacity < 0 || (capacity && !records) || !totals) return api_fail(1, "jg_dc_transfer_screen: bad argument");
    if ((capability || limiting_outage || limiting_branch) && !(capability && limiting_outage && limiting_branch))
        return api_fail(1, "jg_dc_transfer_screen: capability, limiting_outage and limiting_branch go together");
    jg::TransferOut o{amount, records, islanding, totals, worst, capability, limiting_outage, limiting_branch, base, dense_capability, dense_branch};
    DC_RET(jg::transfer_screen(d, (int)k0, (int)k1, cutoff, amount ? capacity : 0, o));
    return 0;
}

int jg_dc_transfer_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms) {
    DC_ENTER(h);
    jg::DcTransferState* s = d->transfer;
    return jg::dc_phi_time_kernel(d, "transfer", s ? &s->phi : nullptr, s ? s->blk_rows : 0, kernel, k0, k1, reps, ms,
                                  [&] {
        return [d, sa = jg::screen_args(d, (int)k0, (int)k1, 1e-6), la = jg::list_args(d, (int)k0, (int)k1, 0)](int which) {
            if (which == 0) jg::launch_screen(d, sa);
            else jg::launch_stats(d, la);
        };
    });
}

int jg_dc_transfer_set_island_mode(int64_t h, int mode) {
    DC_ENTER(h);
    return jg::dc_phi_set_island_mode(d, "transfer", mode, d->transfer_shed);
}

int jg_dc_transfer_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* labels, int64_t* buses, int64_t* m, int64_t* side) {
    DC_ENTER(h);
    return jg::dc_phi_get_shed_table(d, "transfer", d->transfer ? &d->transfer->phi : nullptr, k0, k1, count, labels, buses, m, side);
}

int jg_dc_transfer_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow, double* transfer) {
    DC_ENTER(h);
    jg::DcTransferState* s = d->transfer;
    if (!s) return api_fail(4, "jg_dc_transfer_get_shed: jg_dc_transfer_build first");
    if (!flow || !transfer || k0 < 0 || k1 < k0 || k1 > s->phi.nk) return api_fail(1, "jg_dc_transfer_get_shed: bad argument");
    DC_RET(jg::dc_phi_shed_gather(d, &s->phi, (int)k0, (int)k1, s->f0, 1, 1, flow));
    DC_RET(jg::dc_phi_shed_gather(d, &s->phi, (int)k0, (int)k1, s->G, s->ldt, s->T, transfer));
    return 0;
}

int jg_dc_transfer_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_transfer_free(d);
    return 0;
}

}  // extern "C"
