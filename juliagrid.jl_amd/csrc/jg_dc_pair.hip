// jg_dc_pair.hip -- the DC N-2 screen over all pairs of a candidate list (jg_dc_pair.hpp has the algebra and the reference loop it stands for).
//
// Build: Phi by dc_phi_build (jg_dc_phi.hip).  Screen of a row block [k0, k1): k_pair_screen solves the 2 x 2 systems and
// walks the rows of Phi once (a wave = DC_PAIR_TILE candidates k in registers x 64 consecutive l; Phi[m, k..], f0_m, 1 / rating_m through scalar loads,
// Phi[m, l..l+63] one coalesced vector load reused for every k of the tile; nothing is written per m); the records come out of the block's dense result by
// k_dc_rows and dc_block_records (jg_dc_records.hpp has the protocol) under the policy PairRows, sorted by (k, l).  Every store is a vector store.  A screen
// built in shed mode launches the second instance of k_pair_screen, which sheds the bridges of a pair (jg_dc_pair.hpp has the table); the summaries are the same.
#include "jg_dc_pair.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/jgrid.h"

namespace jg {

namespace {

// ---- the screen kernel -------------------------------------------------------------------------------------------------------------------
struct PairScreenArgs {
    const double* Phi; const double* f0; const double* rinv; const int* pos; const int* rbranch;
    const int* crow; const double* cdiag; const double* cf0;
    double* load; int* branch; int* count; double* det;         // [k1 - k0][ldk]; det nullable
    double thr; int rows, ldk, nk, k0, k1, kbase;                // kbase: k0 rounded down to a multiple of the tile (the scalar loads of a tile are 32-byte aligned)
};
struct PairShedArgs : PairScreenArgs {                           // what the SHED instance takes (the other one's argument block is the plain one, as it was)
    const int* cisl; const int* rpre;                            // the candidates' (side, lo, hi, 0) and the rows' preorder[from]
};
// SHED (a screen built in shed mode, jg_dc_pair.hpp): a bridge candidate's column of Phi holds Z[:,c] and its coefficient is g_c = s_c f0_c without a solve; a
// row whose from end lies in the preorder interval of either bridge left with it and carries 0.  The tile's intervals and the row's number are wave-uniform
// (scalar loads, scalar compares, and only a row inside one of them takes the slow path); the lane's interval masks 1 / rating once per row, not per pair.
template <bool SHED>
__global__ __launch_bounds__(64 * DC_PAIR_WAVES) void k_pair_screen(std::conditional_t<SHED, PairShedArgs, PairScreenArgs> a) {
    constexpr int T = DC_PAIR_TILE;
    const int wave = uniform(threadIdx.y);
    const int kt = a.kbase + (blockIdx.y * DC_PAIR_WAVES + wave) * T;
    const int l0 = blockIdx.x * 64;
    if (kt >= a.k1 || l0 + 63 <= kt) return;                     // no pair (k, l > k) of this tile in this chunk
    const int l = l0 + threadIdx.x;
    const size_t ldk = (size_t)a.ldk;
    const bool lane_ok = l < a.nk;
    const double dl = a.cdiag[l], fl = a.cf0[l];
    const int rl = a.crow[l];
    double ck[T], cl[T], wl[T], dt[T];
    int il[T], cnt[T];
    bool ok[T], sing[T];
    int lo[T], hi[T];                                            // SHED: the tile's intervals
    int sl = 0, lol = 1, hil = 0, prl = 0;                       // SHED: the lane's side and interval, and the preorder number of its row
    if constexpr (SHED) {
        const I4 q = ((const I4*)a.cisl)[l];
        sl = q[0]; lol = q[1]; hil = q[2]; prl = a.rpre[rl];
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int k = kt + t;                                    // < ldk: the per-candidate arrays are [ldk], 0 behind nk
        const double dk = ((CDbl)a.cdiag)[k], fk = ((CDbl)a.cf0)[k];
        const int rk = ((CInt)a.crow)[k];
        const double pkl = a.Phi[(size_t)rk * ldk + l];          // Phi[k, l]: a row, coalesced
        const double plk = a.Phi[(size_t)rl * ldk + k];          // Phi[l, k]: a gather, once per pair
        const double a11 = 1.0 - dk, a22 = 1.0 - dl;
        // SHED spells out the fused forms the plain expressions contract to: which product the compiler fuses depends on what else uses the operands, and a
        // pair of two non-bridges has to round as it does in the other instance (held bitwise by tests/test_dc_pair_shed_gpu.py)
        const double det = SHED ? fma(a11, a22, -(pkl * plk)) : a11 * a22 - pkl * plk;
        ok[t] = k >= a.k0 && k < a.k1 && lane_ok && l > k;
        sing[t] = fabs(det) < DC_SINGULAR;
        const bool live = ok[t] && !sing[t];
        ck[t] = live ? (SHED ? fma(pkl, fl, a22 * fk) : a22 * fk + pkl * fl) / det : 0.0;
        cl[t] = live ? (SHED ? fma(a11, fl, plk * fk) : plk * fk + a11 * fl) / det : 0.0;
        dt[t] = det; wl[t] = 0.0; il[t] = -1; cnt[t] = 0;
        lo[t] = 1; hi[t] = 0;
        if constexpr (SHED) {
            const I4 q = ((CI4)a.cisl)[k];
            const int prk = ((CInt)a.rpre)[rk];
            lo[t] = q[1]; hi[t] = q[2];
            const bool bk = q[0] != 0, bl = sl != 0;
            if (bk || bl) {                                      // a pair with a bridge: no 2 x 2 solve (the table of jg_dc_pair.hpp)
                const double gk = q[0] < 0 ? -fk : fk, gl = sl < 0 ? -fl : fl;      // what left m over the bridge before the outage
                const bool l_behind = prl >= q[1] && prl <= q[2], k_behind = prk >= lol && prk <= hil;     // (an empty interval holds nothing)
                const bool behind = l_behind || k_behind;
                const double den = bk == bl ? 1.0 : (bk ? a22 : a11);                // the one non-bridge's own denominator
                const double cm = (bk ? fma(plk, gk, fl) : fma(pkl, gl, fk)) / den;  // ... and its coefficient on M, the bridge's island shed first
                sing[t] = !behind && fabs(den) < DC_SINGULAR;
                const bool on = ok[t] && !sing[t];
                ck[t] = (!on || k_behind) ? 0.0 : (bk ? gk : cm);
                cl[t] = (!on || l_behind) ? 0.0 : (bl ? gl : cm);
                dt[t] = behind ? 1.0 : den;
            }
        }
    }
    const double thr = a.thr;
    auto row = [&](int r, int pk, int pr, auto hit_c) {
        constexpr bool HIT = decltype(hit_c)::value;
        const double f0 = ((CDbl)a.f0)[r], ri = ((CDbl)a.rinv)[r];
        const double* prow = a.Phi + (size_t)r * ldk;
        double pt[T];
        const D4 q0 = *(CD4)(prow + kt);
        pt[0] = q0[0]; pt[1] = q0[1]; pt[2] = q0[2]; pt[3] = q0[3];
        if constexpr (T == 8) {
            const D4 q1 = *(CD4)(prow + kt + 4);
            pt[4] = q1[0]; pt[5] = q1[1]; pt[6] = q1[2]; pt[7] = q1[3];
        }
        const double pl = prow[l];
        double ril = ri;
        if constexpr (SHED) ril = (pr >= lol && pr <= hil) ? 0.0 : ri;       // a row that left with the lane's bridge: loading 0, once per row
#pragma unroll
        for (int t = 0; t < T; ++t) {
            double v = fma(pt[t], ck[t], fma(pl, cl[t], f0));
            if (HIT && (pk == kt + t || pk == l)) v = 0.0;       // the two outaged branches carry nothing
            double ld = fabs(v) * ril;
            if (SHED && HIT && pr >= lo[t] && pr <= hi[t]) ld = 0.0;         // nor does a row that left with the tile's bridge
            if (ld > wl[t]) { wl[t] = ld; il[t] = r; }           // rows ascend by branch index, strict comparison: ties go to the lowest branch (k_dc_flows)
            cnt[t] += ld > thr ? 1 : 0;
        }
    };
    for (int r = 0; r < a.rows; ++r) {
        const int pk = ((CInt)a.pos)[r];
        // only a row whose branch is one of this wave's candidates (at most T + 64 of the rows) needs the test per lane
        bool hit = (unsigned)(pk - kt) < (unsigned)T || (unsigned)(pk - l0) < 64u;
        int pr = 0;
        if constexpr (SHED) {                                    // ... or, in shed mode, a row inside the interval of one of the tile's bridges
            pr = ((CInt)a.rpre)[r];
#pragma unroll
            for (int t = 0; t < T; ++t) hit = hit || (pr >= lo[t] && pr <= hi[t]);
        }
        if (hit) row(r, pk, pr, std::true_type{});
        else row(r, pk, pr, std::false_type{});
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (!ok[t]) continue;
        const size_t o = (size_t)(kt + t - a.k0) * ldk + l;
        a.load[o] = sing[t] ? nan : wl[t];
        a.branch[o] = (sing[t] || il[t] < 0) ? 0 : a.rbranch[il[t]] + 1;
        a.count[o] = sing[t] ? 0 : cnt[t];
        if (a.det) a.det[o] = dt[t];
    }
}

// ---- records out of the block's dense result: the pair's policy of k_dc_rows (jg_dc_records.hpp) --------------------------------------------------
// Row k's columns are the triangle l > k; two lists, the violators v > thr and the islanding pairs (v is NaN); the row's maximum from 0.
struct PairRows {
    static constexpr int LISTS = 2;
    const double* load; const int* branch; const int* count; const int* clabel;
    DcRecords list[2]; double* r_red;
    double thr; int ldk, nk, k0, k1;
    __device__ int first(int k) const { return (k + 1) / 64 * 64; }
    __device__ int cols() const { return nk; }
    __device__ bool valid(int k, int l) const { return l > k && l < nk; }
    __device__ double value(int i, int l) const { return load[(size_t)i * ldk + l]; }
    __device__ bool hit(int q, double v, int) const { return q ? v != v : v > thr; }
    __device__ void write(int q, long long at, int klab, int i, int, int l, double v) const {
        if (q) { long long* e = (long long*)list[1].rec + at * 2; e[0] = klab; e[1] = clabel[l]; return; }
        double* e = (double*)list[0].rec + at * 5;
        e[0] = (double)klab; e[1] = (double)clabel[l]; e[2] = (double)branch[(size_t)i * ldk + l]; e[3] = v; e[4] = (double)count[(size_t)i * ldk + l];
    }
    static __device__ double identity() { return 0.0; }
    static __device__ bool better(double v, double m) { return v > m; }
    static __device__ double combine(double x, double y) { return fmax(x, y); }
};
// worst loading over the block's pairs (k, l) per l: with r_max (per k) the per-candidate ranking
__global__ void k_pair_colmax(const double* load, double* c_max, int ldk, int nk, int k0, int k1) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= ldk) return;
    double mx = 0.0;
    if (l < nk)
        for (int k = k0; k < min(k1, l); ++k) {
            const double v = load[(size_t)(k - k0) * ldk + l];
            if (v > mx) mx = v;
        }
    c_max[l] = mx;
}

int pair_build(DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, int64_t budget, double* info, bool shed) {
    dc_state_release(h, h->pair);
    DcPairState* p = h->pair = new DcPairState();
    int rc = dc_phi_build(h, &p->phi, "jg_dc_pair_build", cand, mon, budget, 0, "", info, shed);
    if (!rc) rc = dev_alloc(h, p->mem, &p->c_max, (size_t)p->phi.ldk, (const double*)nullptr, true);
    return rc ? dc_build_failed(h, h->pair, rc) : 0;
}

// the block's buffers for `rb` rows (and the determinants, on request: kept once allocated); grown, never shrunk
int pair_block(DcHandle* h, int rb, bool want_det, long long rec_cap, long long isl_cap) {
    DcPairState* p = h->pair;
    if (rb > p->blk_rows || (want_det && !p->b_det)) {
        const int rows = std::max(rb, p->blk_rows);
        const bool det = want_det || p->b_det != nullptr;
        const size_t cells = (size_t)rows * p->phi.ldk, r = (size_t)rows;
        DC_TRY(dc_block_grow(h, p->mem, "jg_dc_pair_screen", rows, p->blk_rows, cells * (det ? 24 : 16), {&p->viol, &p->isl}, dc_blk(p->b_load, cells), dc_blk(p->b_branch, cells),
                             dc_blk(p->b_count, cells), dc_blk(p->b_det, det ? cells : 0), dc_blk(p->r_max, r)));
    }
    DC_TRY(dc_list_grow(h, p->mem, p->viol, rec_cap));
    return dc_list_grow(h, p->mem, p->isl, isl_cap);
}

PairShedArgs screen_args(DcHandle* h, int k0, int k1, double thr, bool det) {
    DcPairState* p = h->pair;
    PairShedArgs a{};
    a.Phi = p->phi.Phi; a.f0 = p->phi.row_f0; a.rinv = p->phi.row_rinv; a.pos = p->phi.row_pos; a.rbranch = p->phi.row_branch;
    a.crow = p->phi.cand_row; a.cdiag = p->phi.cand_diag; a.cf0 = p->phi.cand_f0;
    a.load = p->b_load; a.branch = p->b_branch; a.count = p->b_count; a.det = det ? p->b_det : nullptr;
    a.thr = thr; a.rows = p->phi.rows; a.ldk = p->phi.ldk; a.nk = p->phi.nk; a.k0 = k0; a.k1 = k1; a.kbase = k0 / DC_PAIR_TILE * DC_PAIR_TILE;
    a.cisl = p->phi.shed ? p->phi.cand_isl : nullptr; a.rpre = p->phi.shed ? p->phi.row_pre : nullptr;
    return a;
}
void launch_screen(DcHandle* h, const PairShedArgs& a) {
    const int tiles = (a.k1 - a.kbase + DC_PAIR_TILE - 1) / DC_PAIR_TILE;
    const dim3 grid(a.ldk / 64, (tiles + DC_PAIR_WAVES - 1) / DC_PAIR_WAVES), block(64, DC_PAIR_WAVES);
    if (a.cisl) hipLaunchKernelGGL(k_pair_screen<true>, grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL(k_pair_screen<false>, grid, block, 0, h->stream, (const PairScreenArgs&)a);
}
PairRows list_args(DcHandle* h, int k0, int k1, double thr, long long rec_cap, long long isl_cap) {
    DcPairState* p = h->pair;
    PairRows a{};
    a.load = p->b_load; a.branch = p->b_branch; a.count = p->b_count; a.clabel = p->phi.cand_label;
    a.list[0] = p->viol.limited(rec_cap); a.list[1] = p->isl.limited(isl_cap); a.r_red = p->r_max;
    a.thr = thr; a.ldk = p->phi.ldk; a.nk = p->phi.nk; a.k0 = k0; a.k1 = k1;
    return a;
}
void launch_stats(DcHandle* h, const PairRows& a) {
    DcPairState* p = h->pair;
    dc_launch_rows<false>(h, a);
    hipLaunchKernelGGL(k_pair_colmax, dim3((a.ldk + 255) / 256), dim3(256), 0, h->stream, p->b_load, p->c_max, a.ldk, a.nk, a.k0, a.k1);
}

struct PairOut {
    double* records; int64_t* islanding; int64_t* totals; double* worst;
    double* d_load; int32_t* d_branch; int32_t* d_count; double* d_det;
};
int pair_screen(DcHandle* h, int k0, int k1, double thr, long long rec_cap, long long isl_cap, const PairOut& o) {
    DcPairState* p = h->pair;
    const int rb = k1 - k0, nk = p->phi.nk, ldk = p->phi.ldk;
    DC_TRY(pair_block(h, rb, o.d_det != nullptr, rec_cap, isl_cap));
    dc_phi_rinv(h, &p->phi);
    launch_screen(h, screen_args(h, k0, k1, thr, o.d_det != nullptr));
    const PairRows la = list_args(h, k0, k1, thr, rec_cap, isl_cap);
    launch_stats(h, la);
    std::vector<double> rmax(rb), cmax(ldk);
    DcListCall viol{&p->viol, rec_cap, o.records}, isl{&p->isl, isl_cap, o.islanding};
    DC_TRY(dc_block_records(h, rb, {&viol, &isl}, [&] {
        DC_HIP(hipMemcpyAsync(rmax.data(), p->r_max, rb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(sync_copy(cmax.data(), p->c_max, ldk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        return 0;
    }, [&] { dc_launch_rows<true>(h, la); }));
    long long pairs = 0;
    for (int i = 0; i < rb; ++i) pairs += nk - 1 - (k0 + i);
    o.totals[0] = pairs; o.totals[1] = viol.total; o.totals[2] = isl.total; o.totals[3] = viol.kept; o.totals[4] = isl.kept;
    o.totals[5] = (viol.total > rec_cap ? 1 : 0) | (isl.total > isl_cap ? 2 : 0);
    if (o.worst)
        for (int j = 0; j < nk; ++j) {
            double w = cmax[j];
            if (j >= k0 && j < k1) w = std::max(w, rmax[j - k0]);
            o.worst[j] = std::max(o.worst[j], w);
        }
    auto upper = [k0](int i, int l, auto v) { return l > k0 + i ? v : decltype(v)(0); };       // the block's dense results are [k1 - k0][nk], 0 where l <= k
    if (o.d_load) DC_TRY(dc_dense(h, o.d_load, (const double*)p->b_load, rb, ldk, nk, upper));
    if (o.d_branch) DC_TRY(dc_dense(h, o.d_branch, (const int*)p->b_branch, rb, ldk, nk, upper));
    if (o.d_count) DC_TRY(dc_dense(h, o.d_count, (const int*)p->b_count, rb, ldk, nk, upper));
    if (o.d_det) DC_TRY(dc_dense(h, o.d_det, (const double*)p->b_det, rb, ldk, nk, upper));
    return 0;
}

}  // namespace

void dc_pair_free(DcHandle* h) { dc_state_release(h, h->pair); }

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_pair_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t budget_bytes, double* info) {
    DC_ENTER(h);
    const bool shed = d->pair_shed == 1;                         // the mode of THIS build alone, also when it is refused below
    d->pair_shed = 0;
    if (!d->nbr) return api_fail(1, "jg_dc_pair_build: jg_dc_set_branches first");
    if (d->h_rhs.empty()) return api_fail(1, "jg_dc_pair_build: jg_dc_set_rhs first");
    if (nk < 2 || !candidates || !info || nm < 0 || (nm && !monitored)) return api_fail(1, "jg_dc_pair_build: two or more candidates, and info, are needed");
    std::vector<int> cand, mon;
    DC_RET(jg::dc_phi_lists(d, "jg_dc_pair_build", nk, candidates, nm, monitored, cand, mon));
    DC_RET(jg::pair_build(d, cand, mon, budget_bytes, info, shed));
    return 0;
}

int jg_dc_pair_screen(int64_t h, int64_t k0, int64_t k1, double threshold, int64_t capacity, double* records, int64_t island_capacity, int64_t* islanding,
                      int64_t* totals, double* worst, double* dense_load, int32_t* dense_branch, int32_t* dense_count, double* dense_det) {
    DC_ENTER(h);
    if (!d->pair) return api_fail(4, "jg_dc_pair_screen: jg_dc_pair_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_pair_screen: jg_dc_set_rating first (the loadings are |from| / rating)");
    if (k0 < 0 || k1 <= k0 || k1 > d->pair->phi.nk) return api_fail(1, "jg_dc_pair_screen: rows [k0, k1) out of range");
    if (!(threshold >= 0.0) || capacity < 0 || island_capacity < 0 || (capacity && !records) || (island_capacity && !islanding) || !totals)
        return api_fail(1, "jg_dc_pair_screen: bad argument");
    jg::PairOut o{records, islanding, totals, worst, dense_load, dense_branch, dense_count, dense_det};
    DC_RET(jg::pair_screen(d, (int)k0, (int)k1, threshold, capacity, island_capacity, o));
    return 0;
}

int jg_dc_pair_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms) {
    DC_ENTER(h);
    jg::DcPairState* p = d->pair;
    return jg::dc_phi_time_kernel(d, "pair", p ? &p->phi : nullptr, p ? p->blk_rows : 0, kernel, k0, k1, reps, ms,
                                  [&] {
        return [d, sa = jg::screen_args(d, (int)k0, (int)k1, 1.0, false), la = jg::list_args(d, (int)k0, (int)k1, 1.0, 0, 0)](int which) {
            if (which == 0) jg::launch_screen(d, sa);
            else jg::launch_stats(d, la);
        };
    });
}

int jg_dc_pair_set_island_mode(int64_t h, int mode) {
    DC_ENTER(h);
    return jg::dc_phi_set_island_mode(d, "pair", mode, d->pair_shed);
}

int jg_dc_pair_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* labels, int64_t* buses, int64_t* m, int64_t* side) {
    DC_ENTER(h);
    return jg::dc_phi_get_shed_table(d, "pair", d->pair ? &d->pair->phi : nullptr, k0, k1, count, labels, buses, m, side);
}

int jg_dc_pair_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow) {
    DC_ENTER(h);
    if (!d->pair) return api_fail(4, "jg_dc_pair_get_shed: jg_dc_pair_build first");
    if (!flow || k0 < 0 || k1 < k0 || k1 > d->pair->phi.nk) return api_fail(1, "jg_dc_pair_get_shed: bad argument");
    DC_RET(jg::dc_phi_shed_gather(d, &d->pair->phi, (int)k0, (int)k1, d->pair->phi.row_f0, 1, 1, flow));      // the base flows: one "profile"
    return 0;
}

int jg_dc_pair_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_pair_free(d);
    return 0;
}

}  // extern "C"
