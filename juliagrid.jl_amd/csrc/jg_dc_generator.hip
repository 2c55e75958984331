// jg_dc_generator.hip -- the DC generator-outage screen: G-1 and generator x branch cases (jg_dc_generator.hpp has the algebra and the reference loop it
// stands for).
//
// Build: Phi by the build the screens share (dc_phi_build, jg_dc_phi.hip), into a state of the screen's own; Psi, the row flows per unit injection at
// every distinct generator bus (dc_phi_row_flows without the shift angle: the sweep pair of jg_dc_sweep.hip on unit right-hand sides, DC_PAIR_LANES buses
// at a time); then k_gen_flows, F0 = f0 + Psi A with A in CSC (a wave = DC_GEN_FLOW_ROWS rows in registers x 64 consecutive generators; f0 through scalar
// loads, an entry of A once for all the rows, the gather from a row of Psi stays inside that row).  Screen of a row block [k0, k1): the series' block screen
// (dc_series_launch_screen: k_series_screen on this state's Phi and F0), its column summaries and its base-case kernel (the G-1 cases); the records come
// out of the block's dense result by k_dc_rows and dc_block_records (jg_dc_records.hpp has the protocol) under the policy GeneratorRows, whose walk has
// the G-1 cases as row 0 in front of the candidates' rows, sorted by (k, g).  Every store is a vector store.
#include "jg_dc_generator.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/jgrid.h"
#include "jg_dc_series.hpp"

namespace jg {

namespace {

// ---- F0 = f0 + Psi A ---------------------------------------------------------------------------------------------------------------------------
// Lane g walks column g of A (one entry with slack pickup; every bus that picks up with participation, where the lanes of a wave meet on the same
// entries of Psi).  Rows behind the last are clamped for the loads and not stored; columns behind G are not stored: F0 is zeroed when it is allocated.
struct GenFlowArgs { const double* Psi; const double* f0; const int* aptr; const int* arow; const double* aval; double* F0; int rows, ldb, ldg, G; };
__global__ __launch_bounds__(256) void k_gen_flows(GenFlowArgs a) {
    constexpr int R = DC_GEN_FLOW_ROWS;
    const int wave = uniform(threadIdx.y);
    const int r0 = (blockIdx.x * 4 + wave) * R;
    const int g = blockIdx.y * 64 + threadIdx.x;                // < ldg
    if (r0 >= a.rows || g >= a.G) return;
    const size_t ldb = (size_t)a.ldb;
    const double* prow[R];
    double acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int r = min(r0 + i, a.rows - 1);                  // wave-uniform
        prow[i] = a.Psi + (size_t)r * ldb;
        acc[i] = ((CDbl)a.f0)[r];
    }
    const int e1 = a.aptr[g + 1];
    for (int e = a.aptr[g]; e < e1; ++e) {
        const int b = a.arow[e];                                // < nb <= ldb (checked on the host)
        const double v = a.aval[e];
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = fma(prow[i][b], v, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (r0 + i < a.rows) a.F0[(size_t)(r0 + i) * a.ldg + g] = acc[i];
}

// ---- summaries out of the block's dense result: the generator screen's policy of k_dc_rows (jg_dc_records.hpp) ---------------------------------------
// The walk's rows are numbered 0 (the G-1 cases, kept as base [G][3] by the series' base-case kernel) and 1 + k (candidate position k); k0 / k1 bound the
// WALK.  off = 1: the block starts with row 0, its dense rows follow from block row 1.  One list, the violators v > thr (a NaN, the loading of a bridge
// candidate, compares false); the row's maximum from 0.
struct GeneratorRows {
    static constexpr int LISTS = 1;
    const double* load; const int* branch; const int* count; const double* base; const int* clabel;
    DcRecords list[1]; double* r_red;
    double thr; int ldg, G, k0, k1, off;
    __device__ int first(int) const { return 0; }
    __device__ int cols() const { return G; }
    __device__ bool valid(int, int g) const { return g < G; }
    __device__ double value(int i, int g) const { return (off && i == 0) ? base[(size_t)g * 3] : load[(size_t)(i - off) * ldg + g]; }
    __device__ bool hit(int, double v, int) const { return v > thr; }
    __device__ void write(int, long long at, int klab, int i, int, int g, double v) const {
        double* e = (double*)list[0].rec + at * 5;
        const bool row0 = off && i == 0;
        e[0] = (double)klab; e[1] = (double)g; e[3] = v;
        e[2] = row0 ? base[(size_t)g * 3 + 1] : (double)branch[(size_t)(i - off) * ldg + g];
        e[4] = row0 ? base[(size_t)g * 3 + 2] : (double)count[(size_t)(i - off) * ldg + g];
    }
    static __device__ double identity() { return 0.0; }
    static __device__ bool better(double v, double m) { return v > m; }
    static __device__ double combine(double x, double y) { return fmax(x, y); }
};

GenFlowArgs flow_args(DcGeneratorState* s) {
    return GenFlowArgs{s->Psi, s->phi.row_f0, s->a_ptr, s->a_row, s->a_val, s->F0, s->phi.rows, s->ldb, s->ldg, s->G};
}
void launch_flows(DcHandle* h, const GenFlowArgs& a) {
    const dim3 grid((a.rows + 4 * DC_GEN_FLOW_ROWS - 1) / (4 * DC_GEN_FLOW_ROWS), a.ldg / 64), block(64, 4);
    hipLaunchKernelGGL(k_gen_flows, grid, block, 0, h->stream, a);
}

// buses [nb]: 0-based, ascending; aptr [G + 1], arow [nnz] < nb, aval [nnz]: A in CSC
int generator_build(DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, int G, const std::vector<int>& buses, const int64_t* aptr,
                    const int64_t* arow, const double* aval, int64_t budget, double* info) {
    dc_state_release(h, h->generator);
    const bool shed = h->generator_shed == 1;
    h->generator_shed = 0;
    const int n = h->n, nb = (int)buses.size(), ldg = (G + 63) / 64 * 64, ldb = std::max((nb + 63) / 64 * 64, 64);
    const long long nnz = aptr[G];
    const int nr = (int)dc_phi_row_labels(h, cand, mon, ldg, info).size();
    const size_t f0_bytes = (size_t)info[8], psi_bytes = (size_t)nr * ldb * sizeof(double), a_bytes = (size_t)nnz * 12 + ((size_t)ldg + 1) * 4;
    const size_t scratch = dc_phi_flows_scratch(h, ldb);
    DcGeneratorState* s = h->generator = new DcGeneratorState();
    s->G = G; s->ldg = ldg; s->nb = nb; s->ldb = ldb; s->nnz = nnz;
    const std::string extra = "; F0 needs " + dc_bytes_text(f0_bytes) + " (" + std::to_string(nr) + " rows x " + std::to_string(ldg) + " generators x 8), Psi " +
                              dc_bytes_text(psi_bytes) + " (" + std::to_string(ldb) + " generator buses), A " + dc_bytes_text(a_bytes) + " and " +
                              dc_bytes_text(scratch) + " of scratch";
    std::vector<int> hp((size_t)ldg + 1), hr((size_t)nnz), wl;
    for (int g = 0; g <= ldg; ++g) hp[g] = (int)aptr[std::min(g, G)];
    for (long long e = 0; e < nnz; ++e) hr[e] = (int)arow[e];
    int rc = 0;
    auto step = [&](int r) { if (r && !rc) rc = r; return rc == 0; };
    double ms[2] = {0.0, 0.0};
    step(dc_phi_build(h, &s->phi, "jg_dc_generator_build", cand, mon, budget, f0_bytes + psi_bytes + a_bytes + scratch, extra, info, shed)) &&
        step(dev_alloc(h, s->mem, &s->F0, (size_t)nr * ldg, (const double*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->Psi, (size_t)nr * ldb, (const double*)nullptr, true)) &&
        step(dev_alloc(h, s->mem, &s->c_max, (size_t)ldg, (const double*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->c_viol, (size_t)ldg, (const int*)nullptr, true)) &&
        step(dev_alloc(h, s->mem, &s->base, (size_t)ldg * 3, (const double*)nullptr, true)) && step(dev_alloc(h, s->mem, &s->a_ptr, hp.size(), hp.data())) &&
        step(dev_alloc(h, s->mem, &s->a_row, (size_t)nnz, hr.data())) && step(dev_alloc(h, s->mem, &s->a_val, (size_t)nnz, aval));
    if (!rc) {                                                   // the labels of the walk: row 0, then the candidates
        wl.assign((size_t)s->phi.ldk + 1, 0);
        for (int k = 0; k < s->phi.nk; ++k) wl[k + 1] = s->phi.h_cand[k] + 1;
        step(dev_alloc(h, s->mem, &s->walk_label, wl.size(), wl.data()));
    }
    std::vector<double> unit;                                    // unit right-hand sides of one lane batch of generator buses
    for (int c0 = 0; c0 < nb && !rc; c0 += DC_PAIR_LANES) {
        const int cnt = std::min(DC_PAIR_LANES, nb - c0);
        unit.assign((size_t)cnt * n, 0.0);
        for (int q = 0; q < cnt; ++q) unit[(size_t)q * n + buses[c0 + q]] = 1.0;
        step(dc_phi_row_flows(h, &s->phi, cnt, unit.data(), false, s->Psi + c0, ldb, ms));      // columns c0 .. c0 + cnt - 1 of Psi
    }
    float flow_ms = 0.f;
    if (!rc) {
        hipEvent_t ev[2] = {nullptr, nullptr};
        for (auto& e : ev) step(dc_hip(h, hipEventCreate(&e), "hipEventCreate"));
        if (!rc) {
            step(dc_hip(h, hipEventRecord(ev[0], h->stream), "hipEventRecord"));
            launch_flows(h, flow_args(s));
            step(dc_hip(h, hipGetLastError(), "k_gen_flows")) && step(dc_hip(h, hipEventRecord(ev[1], h->stream), "hipEventRecord")) &&
                step(dc_hip(h, hipEventSynchronize(ev[1]), "hipEventSynchronize")) && step(dc_hip(h, hipEventElapsedTime(&flow_ms, ev[0], ev[1]), "hipEventElapsedTime"));
        }
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    }
    step(rc ? rc : dc_phi_bridges(h, &s->phi, s->h_bridge));
    if (rc) return dc_build_failed(h, h->generator, rc);
    dc_phi_flows_ms(ms, s->build_ms, info);
    s->build_ms[3] = info[13] = (double)flow_ms;
    info[12] = (double)psi_bytes; info[14] = (double)nb; info[15] = (double)nnz;
    return 0;
}

// the block's buffers for `wr` rows of the walk; grown, never shrunk
int generator_block(DcHandle* h, int wr, long long rec_cap) {
    DcGeneratorState* s = h->generator;
    if (wr > s->blk_rows) {
        const size_t cells = (size_t)wr * s->ldg, r = (size_t)wr;
        DC_TRY(dc_block_grow(h, s->mem, "jg_dc_generator_screen", wr, s->blk_rows, cells * 16, {&s->viol}, dc_blk(s->b_load, cells), dc_blk(s->b_branch, cells),
                             dc_blk(s->b_count, cells), dc_blk(s->r_max, r)));
    }
    return dc_list_grow(h, s->mem, s->viol, rec_cap);
}

DcSeriesBlock block_of(DcGeneratorState* s) { return DcSeriesBlock{&s->phi, s->F0, s->ldg, s->G, s->b_load, s->b_branch, s->b_count}; }

// the walk of the candidate rows [k0, k1): row 0 belongs to the call that starts at candidate 0
GeneratorRows list_args(DcHandle* h, int k0, int k1, double thr, long long rec_cap) {
    DcGeneratorState* s = h->generator;
    GeneratorRows a{};
    a.load = s->b_load; a.branch = s->b_branch; a.count = s->b_count; a.base = s->base; a.clabel = s->walk_label;
    a.list[0] = s->viol.limited(rec_cap); a.r_red = s->r_max;
    a.thr = thr; a.ldg = s->ldg; a.G = s->G; a.off = k0 == 0 ? 1 : 0; a.k0 = k0 + 1 - a.off; a.k1 = k1 + 1;
    return a;
}
void launch_stats(DcHandle* h, const GeneratorRows& a) {
    DcGeneratorState* s = h->generator;
    dc_launch_rows<false>(h, a);
    dc_series_launch_cols(h, block_of(s), s->c_max, s->c_viol, a.thr, a.k1 - a.k0 - a.off);
}

struct GeneratorOut {
    double* records; int64_t* islanding; int64_t* totals; double* worst; double* worst_generator; int64_t* viol_generator; double* base;
    double* d_load; int32_t* d_branch; int32_t* d_count;
};
int generator_screen(DcHandle* h, int k0, int k1, double thr, long long rec_cap, const GeneratorOut& o) {
    DcGeneratorState* s = h->generator;
    DcPhi* p = &s->phi;
    const int rb = k1 - k0, G = s->G, ldg = s->ldg;
    DC_TRY(generator_block(h, rb + 1, rec_cap));
    dc_phi_rinv(h, p);
    const DcSeriesBlock blk = block_of(s);
    dc_series_launch_screen(h, blk, k0, k1, thr);
    const GeneratorRows la = list_args(h, k0, k1, thr, rec_cap);
    const int wr = la.k1 - la.k0;
    const bool want_base = la.off || o.base;
    if (want_base) dc_series_launch_base(h, blk, s->base, thr);      // (in front of the count pass: row 0 of the walk reads it)
    launch_stats(h, la);
    std::vector<int> cviol(ldg);
    std::vector<double> rmax(wr), cmax(ldg), base(want_base ? (size_t)G * 3 : 0);
    DcListCall viol{&s->viol, rec_cap, o.records};
    DC_TRY(dc_block_records(h, wr, {&viol}, [&] {
        DC_HIP(hipMemcpyAsync(rmax.data(), s->r_max, wr * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(hipMemcpyAsync(cviol.data(), s->c_viol, ldg * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (want_base) DC_HIP(hipMemcpyAsync(base.data(), s->base, base.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(sync_copy(cmax.data(), s->c_max, ldg * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        return 0;
    }, [&] { dc_launch_rows<true>(h, la); }));
    o.totals[0] = (long long)wr * G; o.totals[1] = viol.total; o.totals[2] = dc_bridge_list(*p, s->h_bridge, k0, k1, o.islanding); o.totals[3] = viol.kept;
    o.totals[4] = viol.total > rec_cap ? 1 : 0;
    if (o.base) std::copy(base.begin(), base.end(), o.base);
    if (o.worst) for (int i = 0; i < rb; ++i) o.worst[k0 + i] = rmax[i + la.off];
    if (o.worst_generator)
        for (int g = 0; g < G; ++g) o.worst_generator[g] = std::max(o.worst_generator[g], la.off ? std::max(cmax[g], base[(size_t)g * 3]) : cmax[g]);
    if (o.viol_generator) for (int g = 0; g < G; ++g) o.viol_generator[g] += cviol[g];
    auto same = [](int, int, auto v) { return v; };
    if (o.d_load) DC_TRY(dc_dense(h, o.d_load, (const double*)s->b_load, rb, ldg, G, same));
    if (o.d_branch) DC_TRY(dc_dense(h, o.d_branch, (const int*)s->b_branch, rb, ldg, G, same));
    if (o.d_count) DC_TRY(dc_dense(h, o.d_count, (const int*)s->b_count, rb, ldg, G, same));
    return 0;
}

}  // namespace

void dc_generator_free(DcHandle* h) { dc_state_release(h, h->generator); }

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_generator_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t generators, int64_t nbus,
                          const int64_t* buses, const int64_t* colptr, const int64_t* rowidx, const double* values, int64_t budget_bytes, double* info) {
    DC_ENTER(h);
    const std::string me = "jg_dc_generator_build: ";
    if (!d->nbr) return api_fail(1, me + "jg_dc_set_branches first");
    if (d->h_rhs.empty()) return api_fail(1, me + "jg_dc_set_rhs first");
    if (nk < 1 || !candidates || !info || nm < 0 || (nm && !monitored)) return api_fail(1, me + "one or more candidates, and info, are needed");
    if (generators < 1 || generators > (1 << 24) || !colptr) return api_fail(1, me + "one or more generator outages are needed");
    if (nbus < 0 || nbus > d->n || (nbus && !buses)) return api_fail(1, me + "the generator buses: at most one per bus");
    std::vector<int> bus((size_t)nbus);
    for (int64_t j = 0; j < nbus; ++j) {
        if (buses[j] < 1 || buses[j] > d->n) return api_fail(1, me + "generator bus out of range");
        if (j && buses[j] <= buses[j - 1]) return api_fail(1, me + "the generator buses must ascend strictly (no bus twice)");
        bus[j] = (int)buses[j] - 1;
    }
    if (colptr[0] != 0) return api_fail(1, me + "colptr starts at 0");
    for (int64_t g = 0; g < generators; ++g)
        if (colptr[g + 1] < colptr[g]) return api_fail(1, me + "colptr must not descend");
    const int64_t nnz = colptr[generators];
    if (nnz > INT32_MAX || (nnz && (!rowidx || !values))) return api_fail(1, me + "rowidx and values [colptr[generators]] are needed");
    for (int64_t e = 0; e < nnz; ++e)
        if (rowidx[e] < 0 || rowidx[e] >= nbus || !std::isfinite(values[e])) return api_fail(1, me + "an entry of A names no generator bus (0-based row) or is not finite");
    std::vector<int> cand, mon;
    DC_RET(jg::dc_phi_lists(d, "jg_dc_generator_build", nk, candidates, nm, monitored, cand, mon));
    DC_RET(jg::generator_build(d, cand, mon, (int)generators, bus, colptr, rowidx, values, budget_bytes, info));
    return 0;
}

int jg_dc_generator_screen(int64_t h, int64_t k0, int64_t k1, double threshold, int64_t capacity, double* records, int64_t* islanding, int64_t* totals,
                           double* worst, double* worst_generator, int64_t* violating_generator, double* base, double* dense_load, int32_t* dense_branch,
                           int32_t* dense_count) {
    DC_ENTER(h);
    if (!d->generator) return api_fail(4, "jg_dc_generator_screen: jg_dc_generator_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_generator_screen: jg_dc_set_rating first (the loadings are |from| / rating)");
    if (k0 < 0 || k1 <= k0 || k1 > d->generator->phi.nk) return api_fail(1, "jg_dc_generator_screen: rows [k0, k1) out of range");
    if (!(threshold >= 0.0) || capacity < 0 || (capacity && !records) || !totals) return api_fail(1, "jg_dc_generator_screen: bad argument");
    jg::GeneratorOut o{records, islanding, totals, worst, worst_generator, violating_generator, base, dense_load, dense_branch, dense_count};
    DC_RET(jg::generator_screen(d, (int)k0, (int)k1, threshold, capacity, o));
    return 0;
}

int jg_dc_generator_get_flows(int64_t h, double* flows) {
    DC_ENTER(h);
    jg::DcGeneratorState* s = d->generator;
    if (!s) return api_fail(4, "jg_dc_generator_get_flows: jg_dc_generator_build first");
    if (!flows) return api_fail(1, "jg_dc_generator_get_flows: bad argument");
    auto same = [](int, int, double v) { return v; };
    DC_RET(jg::dc_dense(d, flows, (const double*)s->F0, s->phi.rows, s->ldg, s->G, same));
    return 0;
}

int jg_dc_generator_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms) {
    DC_ENTER(h);
    jg::DcGeneratorState* s = d->generator;
    if (s && kernel == 2) {                                      // k_gen_flows again: F0 from Psi and A, the same values
        if (!ms || reps < 1) return api_fail(1, "jg_dc_generator_time_kernel: bad argument");
        const int rc = jg::time_events(d->stream, reps, ms, d->error, [&]() -> int { jg::launch_flows(d, jg::flow_args(s)); return 0; });
        return rc ? api_fail(rc, d->error) : 0;
    }
    return jg::dc_phi_time_kernel(d, "generator", s ? &s->phi : nullptr, s ? s->blk_rows - 1 : 0, kernel, k0, k1, reps, ms,
                                  [&] {
        return [d, s, k0, k1, la = jg::list_args(d, (int)k0, (int)k1, 1.0, 0)](int which) {
            if (which == 0) jg::dc_series_launch_screen(d, jg::block_of(s), (int)k0, (int)k1, 1.0);
            else jg::launch_stats(d, la);
        };
    });
}

int jg_dc_generator_set_island_mode(int64_t h, int mode) {
    DC_ENTER(h);
    return jg::dc_phi_set_island_mode(d, "generator", mode, d->generator_shed);
}

int jg_dc_generator_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* labels, int64_t* buses, int64_t* m, int64_t* side) {
    DC_ENTER(h);
    return jg::dc_phi_get_shed_table(d, "generator", d->generator ? &d->generator->phi : nullptr, k0, k1, count, labels, buses, m, side);
}

int jg_dc_generator_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow) {
    DC_ENTER(h);
    jg::DcGeneratorState* s = d->generator;
    if (!s) return api_fail(4, "jg_dc_generator_get_shed: jg_dc_generator_build first");
    if (!flow || k0 < 0 || k1 < k0 || k1 > s->phi.nk) return api_fail(1, "jg_dc_generator_get_shed: bad argument");
    DC_RET(jg::dc_phi_shed_gather(d, &s->phi, (int)k0, (int)k1, s->F0, s->ldg, s->G, flow));
    return 0;
}

int jg_dc_generator_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_generator_free(d);
    return 0;
}

}  // extern "C"
