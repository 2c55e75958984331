// jg_dc_cascade.hip -- the DC cascading-outage screen (jg_dc_cascade.hpp has the rule and the reference loop it stands for).
//
// Build: the candidates are the sorted union of the initiating members and the monitored branches in service (whatever can trip needs its column); Phi by
// dc_phi_build (jg_dc_phi.hip); the events go up as candidate positions.  Run of a block of cascades [c0, c1): ONE launch of k_cascade<K, RULE, MODE>,
// K in {2, 4, 8} by `most`.  Lanes are 64 consecutive cascades; the DC_PAIR_WAVES waves of a workgroup share them.  The stage loop is inside the kernel:
// every wave repeats its lane's small solve in registers (dc_group_lu; cheaper than handing c through LDS, and every wave needs it), walks its quarter of
// the rows of Phi in ascending order exactly as k_group_screen does (the row's f0, 1 / rating and candidate position through scalar loads, up to K gathers
// per lane inside the ONE row), and the waves meet in LDS for the worst loading and its branch, the overload count and the ordered trips.  Every wave
// appends the same trips to its copy of the set.  The loop goes on while any lane of the workgroup runs (__syncthreads_or): all 64 x 4 threads reach every
// barrier, a finished lane idles with its result held.  No host synchronisation and no second launch between stages.  Every store is a vector store.
#include "jg_dc_cascade.hpp"
#include "jg_dc_group_lu.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/jgrid.h"

namespace jg {

namespace {

// rows of the block's integer and double results, each [ldb]
constexpr int CO_STATUS = 0, CO_STAGES = 1, CO_SIZE = 2, CO_PENDING = 3, CO_BRANCH = 4, CO_LABEL = 5, CO_STAGE = 5 + DC_CASCADE_MAX, CO_INTS = 5 + 2 * DC_CASCADE_MAX;
constexpr int CD_WORST = 0, CD_LOAD = 1, CD_DBLS = 1 + DC_CASCADE_MAX;

struct CascadeArgs {
    const double* Phi; const double* f0; const double* rinv; const int* pos; const int* rbranch;     // the rows of Phi
    const int* crow; const double* cf0; const int* clabel;       // the candidates
    const int* epos;                                             // the events: [DC_CASCADE_MAX][lde]
    int* oi; double* od; double* flow;                           // the block: [CO_INTS][ldb], [CD_DBLS][ldb], [rows][ldb] (MODE 1)
    double thr; int rows, ldk, lde, c0, c1, ldb, most;           // ldb: c1 - c0 rounded up to 64
};

// RULE 0: every overloaded branch trips.  A wave keeps the first K overloaded candidate positions of its quarter and their loadings in registers (a fixed
// unrolled select per slot, no array indexed by a runtime value) and its full count; the merge takes the waves in ascending order, so a stage's trips
// ascend by branch; when the counts sum to more than most - |S| nothing is appended.  RULE 1: the most loaded branch trips (strict comparison over
// ascending rows and ascending waves: ties go to the lowest branch).  MODE 1: also the dense flows [rows][ldb] of the state a lane's last walk saw -- its
// final one, since a cascade ends in the stage that appends nothing.
template <int K, int RULE, int MODE>
__global__ __launch_bounds__(64 * DC_PAIR_WAVES) void k_cascade(CascadeArgs a) {
    constexpr int KS = RULE == 0 ? K : 1;                        // trips a wave hands over per stage
    __shared__ double s_w[DC_PAIR_WAVES][64], s_fl[DC_PAIR_WAVES * KS][64];
    __shared__ int s_i[DC_PAIR_WAVES][64], s_c[DC_PAIR_WAVES][64], s_fp[DC_PAIR_WAVES * KS][64];
    const int wave = uniform(threadIdx.y), lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;                       // < ldb
    const int g = a.c0 + i;
    const bool live = g < a.c1;
    const size_t ldk = (size_t)a.ldk, lde = (size_t)a.lde, ldb = (size_t)a.ldb;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double thr = a.thr;
    const int per = (a.rows + DC_PAIR_WAVES - 1) / DC_PAIR_WAVES;
    const int r0 = wave * per, r1 = min(a.rows, r0 + per);
    const bool writer = live && wave == 0;
    int p[K];                                                    // the set: candidate positions in the order they left, -1 behind the last
    int n = 0;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        p[s] = live ? a.epos[s * lde + g] : -1;
        n += p[s] >= 0 ? 1 : 0;
    }
    if (writer) {
#pragma unroll
        for (int s = 0; s < DC_CASCADE_MAX; ++s) {
            const bool in = s < K && p[s < K ? s : 0] >= 0;
            a.oi[(CO_LABEL + s) * ldb + i] = in ? a.clabel[p[s < K ? s : 0]] : 0;
            a.oi[(CO_STAGE + s) * ldb + i] = in ? 0 : -1;
            a.od[(CD_LOAD + s) * ldb + i] = nan;
        }
    }
    bool run = live;
    int status = 0, stg = 0, pending = 0, bfin = 0;
    double wfin = nan;
    for (;;) {
        double c[K];
        bool sing = false;
        if (run) sing = dc_group_lu<K>(a.Phi, ldk, a.crow, a.cf0, p, c);      // (the matrix is dead before the walk starts)
        else {
#pragma unroll
            for (int s = 0; s < K; ++s) c[s] = 0.0;
        }
        const bool walk = run && !sing;
        double wl = 0.0;
        int il = -1, cnt = 0, fp[KS];
        double fl[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) { fp[s] = 0; fl[s] = 0.0; }
        if (__ballot(run) != 0ull) {                             // (wave-uniform; no barrier inside)
            int q[K];
#pragma unroll
            for (int s = 0; s < K; ++s) q[s] = p[s] < 0 ? 0 : p[s];
            for (int r = r0; r < r1; ++r) {
                const int pk = ((CInt)a.pos)[r];
                const double f0 = ((CDbl)a.f0)[r], ri = ((CDbl)a.rinv)[r];
                const double* prow = a.Phi + (size_t)r * ldk;
                double v = f0;
#pragma unroll
                for (int s = 0; s < K; ++s) v = fma(prow[q[s]], c[s], v);
                if (pk >= 0) {                                   // a candidate's row: 0 for the cascades it has left in
                    bool member = false;
#pragma unroll
                    for (int s = 0; s < K; ++s) member = member || p[s] == pk;
                    if (member) v = 0.0;
                }
                const double ld = fabs(v) * ri;
                if (MODE == 1 && run) a.flow[(size_t)r * ldb + i] = sing ? nan : v;
                if (ld > wl) { wl = ld; il = r; }                // rows ascend by branch index, strict comparison: ties go to the lowest branch
                const bool over = walk && pk >= 0 && ld > thr;   // (a rated row is monitored, and a monitored row in service is a candidate)
                if (RULE == 0) {
#pragma unroll
                    for (int s = 0; s < K; ++s)
                        if (over && cnt == s) { fp[s < KS ? s : 0] = pk; fl[s < KS ? s : 0] = ld; }
                } else if (over && ld > fl[0]) { fl[0] = ld; fp[0] = pk; }
                cnt += over ? 1 : 0;
            }
        }
        s_w[wave][lane] = wl; s_i[wave][lane] = il; s_c[wave][lane] = cnt;
#pragma unroll
        for (int s = 0; s < KS; ++s) { s_fp[wave * KS + s][lane] = fp[s]; s_fl[wave * KS + s][lane] = fl[s]; }
        __syncthreads();
        if (run) {                                               // every wave merges alike: its copy of the set stays the workgroup's
            wl = s_w[0][lane]; il = s_i[0][lane];
            int total = s_c[0][lane];
#pragma unroll
            for (int w = 1; w < DC_PAIR_WAVES; ++w) {            // the waves' shares ascend: strict comparison keeps the lowest branch
                if (s_w[w][lane] > wl) { wl = s_w[w][lane]; il = s_i[w][lane]; }
                total += s_c[w][lane];
            }
            const int trips = RULE == 0 ? total : (total > 0 ? 1 : 0);
            if (sing) { status = 3; run = false; wfin = nan; bfin = 0; }
            else {
                wfin = wl; bfin = il < 0 ? 0 : a.rbranch[il] + 1;
                if (trips == 0) { status = 0; run = false; }
                else if (n + trips > a.most) { status = DC_CASCADE_TRUNCATED; pending = total; run = false; }
                else {
                    ++stg;
                    if (RULE == 0) {
#pragma unroll
                        for (int w = 0; w < DC_PAIR_WAVES; ++w) {
                            const int cw = s_c[w][lane];
#pragma unroll
                            for (int s = 0; s < KS; ++s) {
                                if (s < cw) {
                                    const int pk = s_fp[w * KS + s][lane];
#pragma unroll
                                    for (int t = 0; t < K; ++t) p[t] = t == n ? pk : p[t];
                                    if (writer) {
                                        a.oi[(CO_LABEL + n) * ldb + i] = a.clabel[pk];
                                        a.oi[(CO_STAGE + n) * ldb + i] = stg;
                                        a.od[(CD_LOAD + n) * ldb + i] = s_fl[w * KS + s][lane];
                                    }
                                    ++n;
                                }
                            }
                        }
                    } else {
                        double bl = s_fl[0][lane];
                        int pk = s_fp[0][lane];
#pragma unroll
                        for (int w = 1; w < DC_PAIR_WAVES; ++w)
                            if (s_fl[w][lane] > bl) { bl = s_fl[w][lane]; pk = s_fp[w][lane]; }
#pragma unroll
                        for (int t = 0; t < K; ++t) p[t] = t == n ? pk : p[t];
                        if (writer) {
                            a.oi[(CO_LABEL + n) * ldb + i] = a.clabel[pk];
                            a.oi[(CO_STAGE + n) * ldb + i] = stg;
                            a.od[(CD_LOAD + n) * ldb + i] = bl;
                        }
                        ++n;
                    }
                }
            }
        }
        if (!__syncthreads_or(run ? 1 : 0)) break;               // (also what keeps the next stage's LDS writes behind this stage's reads)
    }
    if (!writer) return;
    a.oi[CO_STATUS * ldb + i] = status; a.oi[CO_STAGES * ldb + i] = stg; a.oi[CO_SIZE * ldb + i] = n; a.oi[CO_PENDING * ldb + i] = pending;
    a.oi[CO_BRANCH * ldb + i] = bfin; a.od[CD_WORST * ldb + i] = wfin;
}

// ---- the build ------------------------------------------------------------------------------------------------------------------------------
int cascade_build(DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, const std::vector<int>& off, const std::vector<int>& member,
                  int64_t budget, double* info) {
    dc_state_release(h, h->cascade);
    DcCascadeState* s = h->cascade = new DcCascadeState();
    const int ne = (int)off.size() - 1, lde = (ne + 63) / 64 * 64;
    s->nevents = ne; s->lde = lde;
    std::vector<int> cpos(h->nbr, -1), epos((size_t)DC_CASCADE_MAX * lde, -1);
    for (size_t j = 0; j < cand.size(); ++j) cpos[cand[j]] = (int)j;
    s->h_size.resize(ne);
    for (int g = 0; g < ne; ++g) {
        s->h_size[g] = off[g + 1] - off[g];
        for (int q = off[g]; q < off[g + 1]; ++q) epos[(size_t)(q - off[g]) * lde + g] = cpos[member[q]];
    }
    {                                                            // the rows of Phi are monitored u candidates, ascending (dc_phi_build)
        std::vector<char> is_mon(h->nbr, 0);
        for (int m : mon) is_mon[m] = 1;
        int row = 0;
        for (int m = 0; m < h->nbr; ++m)
            if (is_mon[m] || cpos[m] >= 0) { if (is_mon[m]) s->h_mon_row.push_back(row); ++row; }
    }
    const size_t extra = (size_t)DC_CASCADE_MAX * lde * sizeof(int);
    int rc = dc_phi_build(h, &s->phi, "jg_dc_cascade_build", cand, mon, budget, extra, "; the events need " + dc_bytes_text(extra), info);
    if (!rc) rc = dev_alloc(h, s->mem, &s->e_pos, epos.size(), epos.data());
    return rc ? dc_build_failed(h, h->cascade, rc) : 0;
}

// the block's buffers for `rb` cascades (and the dense flows, on request: kept once allocated); grown, never shrunk
int cascade_block(DcHandle* h, int rb, bool want_flow) {
    DcCascadeState* s = h->cascade;
    if (rb > s->blk_rows || (want_flow && !s->b_flow)) {
        const int rows = std::max(rb, s->blk_rows);
        const bool flow = want_flow || s->b_flow != nullptr;
        const size_t ld = ((size_t)rows + 63) / 64 * 64, cells = (size_t)s->phi.rows * ld;
        DC_TRY(dc_block_grow(h, s->mem, "jg_dc_cascade_run", rows, s->blk_rows, ld * (CO_INTS * sizeof(int) + CD_DBLS * sizeof(double)) + (flow ? cells * 8 : 0),
                             std::initializer_list<DcRecords*>{}, dc_blk(s->b_int, ld * CO_INTS), dc_blk(s->b_dbl, ld * CD_DBLS), dc_blk(s->b_flow, flow ? cells : 0)));
    }
    return 0;
}

CascadeArgs cascade_args(DcHandle* h, int c0, int c1, double thr, int most) {
    DcCascadeState* s = h->cascade;
    CascadeArgs a{};
    a.Phi = s->phi.Phi; a.f0 = s->phi.row_f0; a.rinv = s->phi.row_rinv; a.pos = s->phi.row_pos; a.rbranch = s->phi.row_branch;
    a.crow = s->phi.cand_row; a.cf0 = s->phi.cand_f0; a.clabel = s->phi.cand_label;
    a.epos = s->e_pos; a.oi = s->b_int; a.od = s->b_dbl; a.flow = s->b_flow;
    a.thr = thr; a.rows = s->phi.rows; a.ldk = s->phi.ldk; a.lde = s->lde; a.c0 = c0; a.c1 = c1; a.ldb = (c1 - c0 + 63) / 64 * 64; a.most = most;
    return a;
}
template <int RULE, int MODE>
void launch_k(DcHandle* h, const CascadeArgs& a) {
    const dim3 grid(a.ldb / 64), block(64, DC_PAIR_WAVES);
    if (a.most <= 2) hipLaunchKernelGGL((k_cascade<2, RULE, MODE>), grid, block, 0, h->stream, a);
    else if (a.most <= 4) hipLaunchKernelGGL((k_cascade<4, RULE, MODE>), grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL((k_cascade<DC_CASCADE_MAX, RULE, MODE>), grid, block, 0, h->stream, a);
}
void launch_cascade(DcHandle* h, const CascadeArgs& a, int rule, bool flow) {
    if (rule == 0) { if (flow) launch_k<0, 1>(h, a); else launch_k<0, 0>(h, a); }
    else { if (flow) launch_k<1, 1>(h, a); else launch_k<1, 0>(h, a); }
}

struct CascadeOut {
    int32_t* status; int32_t* stages; int32_t* size; int64_t* tripped; int32_t* stage; double* loading; double* worst; int32_t* branch; int32_t* pending;
    double* flow; double* ms;
};
int cascade_run(DcHandle* h, int c0, int c1, double thr, int rule, int most, const CascadeOut& o) {
    DcCascadeState* s = h->cascade;
    const int rb = c1 - c0;
    DC_TRY(cascade_block(h, rb, o.flow != nullptr));
    dc_phi_rinv(h, &s->phi);
    const CascadeArgs a = cascade_args(h, c0, c1, thr, most);
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (o.ms) { DC_HIP(hipEventCreate(&ev[0])); DC_HIP(hipEventCreate(&ev[1])); DC_HIP(hipEventRecord(ev[0], h->stream)); }
    launch_cascade(h, a, rule, o.flow != nullptr);
    if (o.ms) (void)hipEventRecord(ev[1], h->stream);
    DC_HIP(hipGetLastError());
    const size_t ldb = (size_t)a.ldb;
    std::vector<int> oi(ldb * CO_INTS);
    std::vector<double> od(ldb * CD_DBLS);
    DC_HIP(hipMemcpyAsync(oi.data(), s->b_int, oi.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(sync_copy(od.data(), s->b_dbl, od.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (o.ms) {
        float t = 0.f;
        const hipError_t e = hipEventElapsedTime(&t, ev[0], ev[1]);
        (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
        DC_HIP(e);
        *o.ms = (double)t;
    }
    for (int i = 0; i < rb; ++i) {
        if (o.status) o.status[i] = oi[CO_STATUS * ldb + i];
        if (o.stages) o.stages[i] = oi[CO_STAGES * ldb + i];
        if (o.size) o.size[i] = oi[CO_SIZE * ldb + i];
        if (o.pending) o.pending[i] = oi[CO_PENDING * ldb + i];
        if (o.branch) o.branch[i] = oi[CO_BRANCH * ldb + i];
        if (o.worst) o.worst[i] = od[CD_WORST * ldb + i];
        for (int q = 0; q < most; ++q) {
            if (o.tripped) o.tripped[(size_t)i * most + q] = oi[(CO_LABEL + q) * ldb + i];
            if (o.stage) o.stage[(size_t)i * most + q] = oi[(CO_STAGE + q) * ldb + i];
            if (o.loading) o.loading[(size_t)i * most + q] = od[(CD_LOAD + q) * ldb + i];
        }
    }
    if (o.flow) {                                                // the device's [rows][ldb] as [rb][monitored]
        const size_t nm = s->h_mon_row.size();
        std::vector<double> t((size_t)s->phi.rows * ldb);
        DC_HIP(sync_copy(t.data(), s->b_flow, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        for (int i = 0; i < rb; ++i)
            for (size_t j = 0; j < nm; ++j) o.flow[(size_t)i * nm + j] = t[(size_t)s->h_mon_row[j] * ldb + i];
    }
    return 0;
}

}  // namespace

void dc_cascade_free(DcHandle* h) { dc_state_release(h, h->cascade); }

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_cascade_build(int64_t h, int64_t nevents, const int64_t* offsets, const int64_t* members, int64_t nm, const int64_t* monitored, int64_t budget_bytes,
                        double* info) {
    DC_ENTER(h);
    const std::string me = "jg_dc_cascade_build: ";
    if (!d->nbr) return api_fail(1, me + "jg_dc_set_branches first");
    if (d->h_rhs.empty()) return api_fail(1, me + "jg_dc_set_rhs first");
    if (nevents < 1 || nevents > (1 << 24) || !offsets || !members || !info || nm < 0 || (nm && !monitored)) return api_fail(1, me + "one or more events, and info, are needed");
    if (offsets[0] != 0) return api_fail(1, me + "offsets [0] is 0");
    std::vector<int> off(nevents + 1, 0), member;
    std::vector<char> in(d->nbr, 0);
    for (int64_t g = 0; g < nevents; ++g) {
        const int64_t k = offsets[g + 1] - offsets[g];
        const std::string who = me + "event " + std::to_string(g);
        if (k < 1) return api_fail(1, who + " is empty");
        if (k > jg::DC_CASCADE_MAX) return api_fail(1, who + " has " + std::to_string(k) + " members, " + std::to_string(jg::DC_CASCADE_MAX) + " at the most");
        for (int64_t q = offsets[g]; q < offsets[g + 1]; ++q) {
            const int64_t m = members[q] - 1;
            if (m < 0 || m >= d->nbr) return api_fail(1, who + ": branch out of range");
            if (d->h_y[m] == 0.0) return api_fail(1, who + ": branch " + std::to_string(m + 1) + " is out of service");
            for (int64_t q2 = offsets[g]; q2 < q; ++q2)
                if (members[q2] == members[q]) return api_fail(1, who + " names branch " + std::to_string(m + 1) + " twice");
            in[m] = 1;
            member.push_back((int)m);
        }
        off[g + 1] = (int)member.size();
    }
    // whatever can trip needs its column: the monitored branches in service join the candidates (null: every branch in service is monitored)
    for (int64_t j = 0; j < nm; ++j) {
        const int64_t m = monitored[j] - 1;
        if (m < 0 || m >= d->nbr) return api_fail(1, me + "monitored branch out of range");
        if (d->h_y[m] != 0.0) in[m] = 1;
    }
    if (!monitored)
        for (int m = 0; m < d->nbr; ++m) if (d->h_y[m] != 0.0) in[m] = 1;
    std::vector<int64_t> labels;
    for (int m = 0; m < d->nbr; ++m) if (in[m]) labels.push_back(m + 1);
    std::vector<int> cand, mon;
    DC_RET(jg::dc_phi_lists(d, "jg_dc_cascade_build", (int64_t)labels.size(), labels.data(), nm, monitored, cand, mon));
    DC_RET(jg::cascade_build(d, cand, mon, off, member, budget_bytes, info));
    return 0;
}

int jg_dc_cascade_run(int64_t h, int64_t c0, int64_t c1, double trip, int rule, int most, int32_t* status, int32_t* stages, int32_t* size, int64_t* tripped,
                      int32_t* stage, double* loading, double* worst, int32_t* worst_branch, int32_t* pending, double* dense_flow, double* ms) {
    DC_ENTER(h);
    const std::string me = "jg_dc_cascade_run: ";
    if (!d->cascade) return api_fail(4, me + "jg_dc_cascade_build first");
    if (!d->b_rating) return api_fail(1, me + "jg_dc_set_rating first (the loadings are |from| / rating)");
    if (c0 < 0 || c1 <= c0 || c1 > d->cascade->nevents) return api_fail(1, me + "cascades [c0, c1) out of range");
    if (!(trip >= 0.0) || rule < 0 || rule > 1 || most < 2 || most > jg::DC_CASCADE_MAX) return api_fail(1, me + "trip >= 0, rule 0 or 1, most 2 to " + std::to_string(jg::DC_CASCADE_MAX));
    for (int64_t g = c0; g < c1; ++g)
        if (d->cascade->h_size[g] > most)
            return api_fail(1, me + "event " + std::to_string(g) + " has " + std::to_string(d->cascade->h_size[g]) + " members, most is " + std::to_string(most));
    jg::DcCascadeState* s = d->cascade;
    s->last_trip = trip; s->last_most = most;
    jg::CascadeOut o{status, stages, size, tripped, stage, loading, worst, worst_branch, pending, dense_flow, ms};
    DC_RET(jg::cascade_run(d, (int)c0, (int)c1, trip, rule, most, o));
    return 0;
}

int jg_dc_cascade_get_dims(int64_t h, int64_t* dims) {
    DC_ENTER(h);
    if (!d->cascade) return api_fail(4, "jg_dc_cascade_get_dims: jg_dc_cascade_build first");
    if (!dims) return api_fail(1, "jg_dc_cascade_get_dims: null pointer");
    const jg::DcCascadeState* s = d->cascade;
    dims[0] = s->nevents; dims[1] = s->lde; dims[2] = s->phi.nk; dims[3] = s->phi.rows; dims[4] = (int64_t)s->h_mon_row.size();
    dims[5] = *std::max_element(s->h_size.begin(), s->h_size.end());
    return 0;
}

int jg_dc_cascade_get_candidates(int64_t h, int64_t* labels) {
    DC_ENTER(h);
    if (!d->cascade) return api_fail(4, "jg_dc_cascade_get_candidates: jg_dc_cascade_build first");
    if (!labels) return api_fail(1, "jg_dc_cascade_get_candidates: null pointer");
    for (int k = 0; k < d->cascade->phi.nk; ++k) labels[k] = d->cascade->phi.h_cand[k] + 1;
    return 0;
}

int jg_dc_cascade_get_base(int64_t h, double* flow) {
    DC_ENTER(h);
    if (!d->cascade) return api_fail(4, "jg_dc_cascade_get_base: jg_dc_cascade_build first");
    if (!flow) return api_fail(1, "jg_dc_cascade_get_base: null pointer");
    const jg::DcCascadeState* s = d->cascade;
    std::vector<double> f0(s->phi.rows);
    DC_API_HIP(jg::sync_copy(f0.data(), s->phi.row_f0, f0.size() * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    for (size_t j = 0; j < s->h_mon_row.size(); ++j) flow[j] = f0[s->h_mon_row[j]];
    return 0;
}

int jg_dc_cascade_time_kernel(int64_t h, int kernel, int64_t c0, int64_t c1, int reps, double* ms) {
    DC_ENTER(h);
    jg::DcCascadeState* s = d->cascade;
    return jg::dc_phi_time_kernel_rows(d, "cascade", s ? &s->phi : nullptr, s ? s->nevents : 0, s ? s->blk_rows : 0, kernel, c0, c1, reps, ms,
                                       [&] {
        return [d, a = jg::cascade_args(d, (int)c0, (int)c1, s->last_trip, s->last_most)](int which) { jg::launch_cascade(d, a, which, false); };
    });
}

int jg_dc_cascade_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_cascade_free(d);
    return 0;
}

}  // extern "C"
