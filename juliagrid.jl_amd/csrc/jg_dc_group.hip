// jg_dc_group.hip -- the DC common-mode screen over named outage groups of 1 to DC_GROUP_MAX branches (jg_dc_group.hpp has the algebra and the reference
// loop it stands for).
//
// Build: the candidates are the sorted union of all members; Phi by dc_phi_build (jg_dc_phi.hip); the groups go up as candidate positions.  Screen of a block
// of groups [g0, g1): k_group_solve<K> (a lane = a group: I - Phi_SS gathered into registers, LU with partial pivoting fully unrolled, c and the status
// out), then k_group_screen<K, MODE> (lanes = groups; the DC_PAIR_WAVES waves of a workgroup share one chunk of 64 groups and each walks a quarter of the
// rows of Phi: the row's f0, 1 / rating and candidate position through scalar loads, up to K gathers per lane inside the ONE row of Phi; the waves meet in
// LDS).  K in {2, 4, 8} by the largest group of the block.  The records follow the protocol of jg_dc_records.hpp -- a count pass, the host's prefix sum
// (dc_block_records), a scatter pass -- but the count IS the screen kernel's per-group count and the scatter pass is the screen kernel once more (MODE 2),
// which writes a violating row at the group's offset + the violators of the rows before it: sorted by (group, branch) without atomics, the first `capacity`
// kept, the totals exact.  Every store is a vector store.
#include "jg_dc_group.hpp"
#include "jg_dc_group_lu.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/jgrid.h"

namespace jg {

namespace {

struct GroupArgs {
    const double* Phi; const double* f0; const double* rinv; const int* pos; const int* rbranch;     // the rows of Phi
    const int* crow; const double* cf0;                          // the candidates
    const int* gpos; double* c; int* status;                     // the groups: [DC_GROUP_MAX][ldg], [DC_GROUP_MAX][ldg], [ldg]
    double* worst; int* branch; int* wcnt; double* flow;         // the block: [g1 - g0], [g1 - g0], [DC_PAIR_WAVES][ldb], [rows][ldb] (MODE 1)
    DcRecords viol, isl;                                         // as the call limits them
    double thr; int rows, ldk, ldg, g0, g1, ldb;                 // ldb: g1 - g0 rounded up to 64
};

// ---- the k x k solve ----------------------------------------------------------------------------------------------------------------------
// One lane per group; the solve itself is dc_group_lu (jg_dc_group_lu.hpp), which the cascade screen shares.
template <int K>
__global__ __launch_bounds__(64) void k_group_solve(GroupArgs a) {
    const int g = a.g0 + blockIdx.x * 64 + threadIdx.x;
    if (g >= a.g1) return;
    const size_t ldg = (size_t)a.ldg;
    int q[K];
    double c[K];
#pragma unroll
    for (int i = 0; i < K; ++i) q[i] = a.gpos[i * ldg + g];
    const bool sing = dc_group_lu<K>(a.Phi, (size_t)a.ldk, a.crow, a.cf0, q, c);
#pragma unroll
    for (int i = 0; i < K; ++i) a.c[i * ldg + g] = c[i];
    a.status[g] = sing ? 3 : 0;
}

// ---- the screen kernel -------------------------------------------------------------------------------------------------------------------
// MODE 0: the summaries (worst loading, its branch, the count) and the counts of the record protocol.  MODE 1: also the dense flows [rows][ldb].
// MODE 2: the scatter pass -- the same walk, a violating row is written at r_off[group] + the violators of the waves before + those of this wave so far.
// Wave w walks the rows [w q, (w + 1) q), q = rows / DC_PAIR_WAVES rounded up: ascending, so the records of a group ascend by branch.
template <int K, int MODE>
__global__ __launch_bounds__(64 * DC_PAIR_WAVES) void k_group_screen(GroupArgs a) {
    __shared__ double s_w[DC_PAIR_WAVES][64];
    __shared__ int s_i[DC_PAIR_WAVES][64], s_c[DC_PAIR_WAVES][64];
    const int wave = uniform(threadIdx.y), lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;                       // < ldb
    const int g = a.g0 + i;
    const bool live = g < a.g1;
    const size_t ldk = (size_t)a.ldk, ldg = (size_t)a.ldg, ldb = (size_t)a.ldb;
    int p[K], q[K];
    double c[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
        p[s] = live ? a.gpos[s * ldg + g] : -1;
        q[s] = p[s] < 0 ? 0 : p[s];
        c[s] = p[s] < 0 ? 0.0 : a.c[s * ldg + g];
    }
    const bool sing = live && a.status[g] == 3;
    const bool counts = live && !sing;
    const double thr = a.thr;
    const int per = (a.rows + DC_PAIR_WAVES - 1) / DC_PAIR_WAVES;
    const int r0 = wave * per, r1 = min(a.rows, r0 + per);
    long long at = 0;
    if (MODE == 2 && counts) {
        at = a.viol.r_off[i];
        for (int w = 0; w < wave; ++w) at += a.wcnt[w * ldb + i];
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double wl = 0.0;
    int il = -1, cnt = 0;
    for (int r = r0; r < r1; ++r) {
        const int pk = ((CInt)a.pos)[r];
        const double f0 = ((CDbl)a.f0)[r], ri = ((CDbl)a.rinv)[r];
        const double* prow = a.Phi + (size_t)r * ldk;
        double v = f0;
#pragma unroll
        for (int s = 0; s < K; ++s) v = fma(prow[q[s]], c[s], v);
        if (pk >= 0) {                                           // a candidate's row: 0 for the groups it is a member of (the sum there is c_s, not 0)
            bool member = false;
#pragma unroll
            for (int s = 0; s < K; ++s) member = member || p[s] == pk;
            if (member) v = 0.0;
        }
        const double ld = fabs(v) * ri;
        const bool over = counts && ld > thr;
        if (MODE == 1 && live) a.flow[(size_t)r * ldb + i] = sing ? nan : v;
        if (MODE == 2) {
            if (over) {
                if (at < a.viol.cap) {
                    double* e = (double*)a.viol.rec + at * 4;
                    e[0] = (double)g; e[1] = (double)(((CInt)a.rbranch)[r] + 1); e[2] = v; e[3] = ld;
                }
                ++at;
            }
        } else {
            if (ld > wl) { wl = ld; il = r; }                    // rows ascend by branch index, strict comparison: ties go to the lowest branch (k_dc_flows)
            cnt += over ? 1 : 0;
        }
    }
    if (MODE == 2) {
        if (wave == 0 && sing) {
            const long long ai = a.isl.r_off[i];
            if (ai < a.isl.cap) ((long long*)a.isl.rec)[ai] = g;
        }
        return;
    }
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
    a.viol.r_count[i] = cnt;
    a.isl.r_count[i] = sing ? 1 : 0;
}

// ---- the build ------------------------------------------------------------------------------------------------------------------------------
int group_build(DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, const std::vector<int>& off, const std::vector<int>& member,
                int64_t budget, double* info) {
    dc_state_release(h, h->group);
    DcGroupState* s = h->group = new DcGroupState();
    const int ng = (int)off.size() - 1, ldg = (ng + 63) / 64 * 64;
    s->ngroups = ng; s->ldg = ldg;
    std::vector<int> cpos(h->nbr, -1), gpos((size_t)DC_GROUP_MAX * ldg, -1);
    for (size_t j = 0; j < cand.size(); ++j) cpos[cand[j]] = (int)j;
    s->h_size.resize(ng);
    for (int g = 0; g < ng; ++g) {
        s->h_size[g] = off[g + 1] - off[g];
        for (int q = off[g]; q < off[g + 1]; ++q) gpos[(size_t)(q - off[g]) * ldg + g] = cpos[member[q]];
    }
    {                                                            // the rows of Phi are monitored u candidates, ascending (dc_phi_build)
        std::vector<char> is_mon(h->nbr, 0);
        for (int m : mon) is_mon[m] = 1;
        int row = 0;
        for (int m = 0; m < h->nbr; ++m)
            if (is_mon[m] || cpos[m] >= 0) { if (is_mon[m]) s->h_mon_row.push_back(row); ++row; }
    }
    const size_t extra = (size_t)DC_GROUP_MAX * ldg * (sizeof(int) + sizeof(double)) + (size_t)ldg * sizeof(int);
    int rc = dc_phi_build(h, &s->phi, "jg_dc_group_build", cand, mon, budget, extra, "; the groups need " + dc_bytes_text(extra), info);
    if (!rc) rc = dev_alloc(h, s->mem, &s->g_pos, gpos.size(), gpos.data());
    if (!rc) rc = dev_alloc(h, s->mem, &s->c, (size_t)DC_GROUP_MAX * ldg, (const double*)nullptr, true);
    if (!rc) rc = dev_alloc(h, s->mem, &s->status, (size_t)ldg, (const int*)nullptr, true);
    return rc ? dc_build_failed(h, h->group, rc) : 0;
}

// the block's buffers for `rb` groups (and the dense flows, on request: kept once allocated); grown, never shrunk
int group_block(DcHandle* h, int rb, bool want_flow, long long rec_cap, long long isl_cap) {
    DcGroupState* s = h->group;
    if (rb > s->blk_groups || (want_flow && !s->b_flow)) {
        const int groups = std::max(rb, s->blk_groups);
        const bool flow = want_flow || s->b_flow != nullptr;
        const size_t ld = ((size_t)groups + 63) / 64 * 64, cells = (size_t)s->phi.rows * ld;
        DC_TRY(dc_block_grow(h, s->mem, "jg_dc_group_screen", groups, s->blk_groups, (size_t)groups * 36 + ld * DC_PAIR_WAVES * 4 + (flow ? cells * 8 : 0), {&s->viol, &s->isl},
                             dc_blk(s->b_worst, (size_t)groups), dc_blk(s->b_branch, (size_t)groups), dc_blk(s->b_wcnt, ld * DC_PAIR_WAVES), dc_blk(s->b_flow, flow ? cells : 0)));
    }
    DC_TRY(dc_list_grow(h, s->mem, s->viol, rec_cap));
    return dc_list_grow(h, s->mem, s->isl, isl_cap);
}

GroupArgs screen_args(DcHandle* h, int g0, int g1, double thr, long long rec_cap, long long isl_cap) {
    DcGroupState* s = h->group;
    GroupArgs a{};
    a.Phi = s->phi.Phi; a.f0 = s->phi.row_f0; a.rinv = s->phi.row_rinv; a.pos = s->phi.row_pos; a.rbranch = s->phi.row_branch;
    a.crow = s->phi.cand_row; a.cf0 = s->phi.cand_f0;
    a.gpos = s->g_pos; a.c = s->c; a.status = s->status;
    a.worst = s->b_worst; a.branch = s->b_branch; a.wcnt = s->b_wcnt; a.flow = s->b_flow;
    a.viol = s->viol.limited(rec_cap); a.isl = s->isl.limited(isl_cap);
    a.thr = thr; a.rows = s->phi.rows; a.ldk = s->phi.ldk; a.ldg = s->ldg; a.g0 = g0; a.g1 = g1; a.ldb = (g1 - g0 + 63) / 64 * 64;
    return a;
}
// K of a block: the smallest instance that holds its largest group
int block_k(const DcGroupState* s, int g0, int g1) {
    const int most = *std::max_element(s->h_size.begin() + g0, s->h_size.begin() + g1);
    return most <= 2 ? 2 : most <= 4 ? 4 : DC_GROUP_MAX;
}
void launch_solve(DcHandle* h, const GroupArgs& a, int K) {
    const dim3 grid(a.ldb / 64), block(64);
    if (K == 2) hipLaunchKernelGGL(k_group_solve<2>, grid, block, 0, h->stream, a);
    else if (K == 4) hipLaunchKernelGGL(k_group_solve<4>, grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL(k_group_solve<DC_GROUP_MAX>, grid, block, 0, h->stream, a);
}
template <int MODE>
void launch_screen(DcHandle* h, const GroupArgs& a, int K) {
    const dim3 grid(a.ldb / 64), block(64, DC_PAIR_WAVES);
    if (K == 2) hipLaunchKernelGGL((k_group_screen<2, MODE>), grid, block, 0, h->stream, a);
    else if (K == 4) hipLaunchKernelGGL((k_group_screen<4, MODE>), grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL((k_group_screen<DC_GROUP_MAX, MODE>), grid, block, 0, h->stream, a);
}

struct GroupOut {
    double* records; int64_t* islanding; int64_t* totals; int32_t* status; double* worst; int32_t* branch; int32_t* count; double* flow; double* ms;
};
int group_screen(DcHandle* h, int g0, int g1, double thr, long long rec_cap, long long isl_cap, const GroupOut& o) {
    DcGroupState* s = h->group;
    const int rb = g1 - g0, K = block_k(s, g0, g1);
    DC_TRY(group_block(h, rb, o.flow != nullptr, rec_cap, isl_cap));
    dc_phi_rinv(h, &s->phi);
    const GroupArgs a = screen_args(h, g0, g1, thr, rec_cap, isl_cap);
    hipEvent_t ev[2] = {nullptr, nullptr};                      // around the solves and the screen kernel (the download of the counts waits for both)
    if (o.ms) { DC_HIP(hipEventCreate(&ev[0])); DC_HIP(hipEventCreate(&ev[1])); DC_HIP(hipEventRecord(ev[0], h->stream)); }
    launch_solve(h, a, K);
    if (o.flow) launch_screen<1>(h, a, K);
    else launch_screen<0>(h, a, K);
    if (o.ms) (void)hipEventRecord(ev[1], h->stream);
    std::vector<double> worst(rb);
    std::vector<int> branch(rb);
    DcListCall viol{&s->viol, rec_cap, o.records}, isl{&s->isl, isl_cap, o.islanding};
    DC_TRY(dc_block_records(h, rb, {&viol, &isl}, [&] {
        DC_HIP(hipMemcpyAsync(worst.data(), s->b_worst, rb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(sync_copy(branch.data(), s->b_branch, rb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        return 0;
    }, [&] { launch_screen<2>(h, a, K); }));
    if (o.ms) {
        float t = 0.f;
        const hipError_t e = hipEventElapsedTime(&t, ev[0], ev[1]);
        (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
        DC_HIP(e);
        *o.ms = (double)t;
    }
    o.totals[0] = rb; o.totals[1] = viol.total; o.totals[2] = isl.total; o.totals[3] = viol.kept; o.totals[4] = isl.kept;
    o.totals[5] = (viol.total > rec_cap ? 1 : 0) | (isl.total > isl_cap ? 2 : 0);
    for (int i = 0; i < rb; ++i) {
        if (o.status) o.status[i] = isl.count[i] ? 3 : 0;
        if (o.worst) o.worst[i] = worst[i];
        if (o.branch) o.branch[i] = branch[i];
        if (o.count) o.count[i] = viol.count[i];
    }
    if (o.flow) {                                                // the device's [rows][ldb] as [rb][monitored]
        const size_t ldb = (size_t)a.ldb, nm = s->h_mon_row.size();
        std::vector<double> t((size_t)s->phi.rows * ldb);
        DC_HIP(sync_copy(t.data(), s->b_flow, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        for (int i = 0; i < rb; ++i)
            for (size_t j = 0; j < nm; ++j) o.flow[(size_t)i * nm + j] = t[(size_t)s->h_mon_row[j] * ldb + i];
    }
    return 0;
}

}  // namespace

void dc_group_free(DcHandle* h) { dc_state_release(h, h->group); }

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_group_build(int64_t h, int64_t ngroups, const int64_t* offsets, const int64_t* members, int64_t nm, const int64_t* monitored, int64_t budget_bytes,
                      double* info) {
    DC_ENTER(h);
    const std::string me = "jg_dc_group_build: ";
    if (!d->nbr) return api_fail(1, me + "jg_dc_set_branches first");
    if (d->h_rhs.empty()) return api_fail(1, me + "jg_dc_set_rhs first");
    if (ngroups < 1 || ngroups > (1 << 24) || !offsets || !members || !info || nm < 0 || (nm && !monitored)) return api_fail(1, me + "one or more groups, and info, are needed");
    if (offsets[0] != 0) return api_fail(1, me + "offsets [0] is 0");
    std::vector<int> off(ngroups + 1, 0), member;
    std::vector<char> in(d->nbr, 0);
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t k = offsets[g + 1] - offsets[g];
        const std::string who = me + "group " + std::to_string(g);
        if (k < 1) return api_fail(1, who + " is empty");
        if (k > jg::DC_GROUP_MAX) return api_fail(1, who + " has " + std::to_string(k) + " members, " + std::to_string(jg::DC_GROUP_MAX) + " at the most");
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
    std::vector<int64_t> labels;
    for (int m = 0; m < d->nbr; ++m) if (in[m]) labels.push_back(m + 1);
    std::vector<int> cand, mon;
    DC_RET(jg::dc_phi_lists(d, "jg_dc_group_build", (int64_t)labels.size(), labels.data(), nm, monitored, cand, mon));
    DC_RET(jg::group_build(d, cand, mon, off, member, budget_bytes, info));
    return 0;
}

int jg_dc_group_screen(int64_t h, int64_t g0, int64_t g1, double threshold, int64_t capacity, double* records, int64_t island_capacity, int64_t* islanding,
                       int64_t* totals, int32_t* status, double* worst, int32_t* worst_branch, int32_t* count, double* dense_flow, double* ms) {
    DC_ENTER(h);
    if (!d->group) return api_fail(4, "jg_dc_group_screen: jg_dc_group_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_group_screen: jg_dc_set_rating first (the loadings are |from| / rating)");
    if (g0 < 0 || g1 <= g0 || g1 > d->group->ngroups) return api_fail(1, "jg_dc_group_screen: groups [g0, g1) out of range");
    if (!(threshold >= 0.0) || capacity < 0 || island_capacity < 0 || (capacity && !records) || (island_capacity && !islanding) || !totals)
        return api_fail(1, "jg_dc_group_screen: bad argument");
    jg::GroupOut o{records, islanding, totals, status, worst, worst_branch, count, dense_flow, ms};
    DC_RET(jg::group_screen(d, (int)g0, (int)g1, threshold, capacity, island_capacity, o));
    return 0;
}

int jg_dc_group_get_dims(int64_t h, int64_t* dims) {
    DC_ENTER(h);
    if (!d->group) return api_fail(4, "jg_dc_group_get_dims: jg_dc_group_build first");
    if (!dims) return api_fail(1, "jg_dc_group_get_dims: null pointer");
    const jg::DcGroupState* s = d->group;
    dims[0] = s->ngroups; dims[1] = s->ldg; dims[2] = s->phi.nk; dims[3] = s->phi.rows; dims[4] = (int64_t)s->h_mon_row.size();
    dims[5] = *std::max_element(s->h_size.begin(), s->h_size.end());
    return 0;
}

int jg_dc_group_get_candidates(int64_t h, int64_t* labels) {
    DC_ENTER(h);
    if (!d->group) return api_fail(4, "jg_dc_group_get_candidates: jg_dc_group_build first");
    if (!labels) return api_fail(1, "jg_dc_group_get_candidates: null pointer");
    for (int k = 0; k < d->group->phi.nk; ++k) labels[k] = d->group->phi.h_cand[k] + 1;
    return 0;
}

int jg_dc_group_get_base(int64_t h, double* flow) {
    DC_ENTER(h);
    if (!d->group) return api_fail(4, "jg_dc_group_get_base: jg_dc_group_build first");
    if (!flow) return api_fail(1, "jg_dc_group_get_base: null pointer");
    const jg::DcGroupState* s = d->group;
    std::vector<double> f0(s->phi.rows);
    DC_API_HIP(jg::sync_copy(f0.data(), s->phi.row_f0, f0.size() * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    for (size_t j = 0; j < s->h_mon_row.size(); ++j) flow[j] = f0[s->h_mon_row[j]];
    return 0;
}

int jg_dc_group_time_kernel(int64_t h, int kernel, int64_t g0, int64_t g1, int reps, double* ms) {
    DC_ENTER(h);
    jg::DcGroupState* s = d->group;
    return jg::dc_phi_time_kernel_rows(d, "group", s ? &s->phi : nullptr, s ? s->ngroups : 0, s ? s->blk_groups : 0, kernel, g0, g1, reps, ms,
                                       [&] {
        return [d, a = jg::screen_args(d, (int)g0, (int)g1, 1.0, 0, 0), K = jg::block_k(d->group, (int)g0, (int)g1)](int which) {
            if (which == 0) jg::launch_screen<0>(d, a, K);
            else jg::launch_solve(d, a, K);
        };
    });
}

int jg_dc_group_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_group_free(d);
    return 0;
}

}  // extern "C"
