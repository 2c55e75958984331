// jg_dc.hip -- DC power flow and the batched DC N-1 screen on one shared scalar factor (jg_dc.hpp has the algebra and the reference lines it stands for).
//
// The scalar factorisation of the ONE base matrix (once per base case), the level-scheduled sweeps with scenarios as lanes and the branch-flow kernel
// are jg_dc_sweep.hip's (declared in jg_dc_sweep.hpp), shared with jg_dcse.hip; here: the rank-1 combine, the screen summary and the C ABI.
#include "jg_dc.hpp"
#include "jg_dc_abi.hpp"
#include "jg_dc_pair.hpp"
#include "jg_dc_series.hpp"
#include "jg_dc_transfer.hpp"
#include "jg_dc_generator.hpp"
#include "jg_dc_group.hpp"
#include "jg_dc_chance.hpp"
#include "jg_dc_cascade.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/jgrid.h"
#include "jg_engine.hpp"

namespace jg {

namespace {

// ---- the rank-1 combine ------------------------------------------------------------------------------------------------------------------
struct DcCombineArgs {
    const double* Z; const double* XS; const double* th0;      // z_s [n][ld]; B^-1 rhs_s [n][ld] of the groups with ginj; theta_0 [n][64], lane 0
    const int* ginj;                                            // nullable [ld / 64]
    const int* of; const int* ot; const int* obr; const double* oy; const double* osh;
    double* TH; int* status;
    double slack_angle; int n, ld, slack;
    // ISL (island mode 1 and a lane that needs it): preorder [n]; isl [ld] = (S end of the bridge or -1, lo, hi, side); rhs0 [n][64] / RHS [n][ld] the
    // right-hand sides the shed record sums; ipart [chunks][2][ld]; ig [ld]
    const int* preorder; const I4* isl; const double* rhs0; const double* RHS; double* ipart; double* ig;
};
constexpr int DC_COMBINE_ROWS = 8;
// ISL: a lane whose outage is a bridge, set in island mode 1, has o_from = m (the bridge's end on the slack's side; -1: m is the slack) and o_to = -1, so
// Z holds z = B^-1 e_m.  theta = x0 + g z outside the preorder interval lo .. hi of the side S that leaves, NaN inside, status 4; g = the flow on the
// bridge that left m.  Each wave also leaves the buses of S among its rows and their right-hand side in ipart (k_dc_island_final adds them up in
// order).  The other lanes take the expressions of ISL = false unchanged.
template <bool ISL>
__global__ __launch_bounds__(256) void k_dc_combine(DcCombineArgs a) {
    const int wave = uniform(threadIdx.y);
    const int grp = blockIdx.y;
    const size_t ld = (size_t)a.ld, bl = (size_t)grp * 64 + threadIdx.x;
    const bool own = a.ginj && ((CInt)a.ginj)[grp] != 0;
    const int fi = a.of[bl], ti = a.ot[bl];
    const bool has = a.obr[bl] >= 0;
    const double yk = a.oy[bl], sh = a.osh[bl];
    auto x0 = [&](int bus) { return own ? a.XS[(size_t)bus * ld + bl] : a.th0[(size_t)bus * 64]; };
    const double az = (fi >= 0 ? a.Z[(size_t)fi * ld + bl] : 0.0) - (ti >= 0 ? a.Z[(size_t)ti * ld + bl] : 0.0);
    const double ax = ((fi >= 0 ? x0(fi) : 0.0) - (ti >= 0 ? x0(ti) : 0.0)) - sh * az;
    const double den = 1.0 - yk * az;
    const bool sing = has && fabs(den) < DC_SINGULAR;
    double c = (has && !sing) ? yk * ax / den - sh : 0.0;            // theta = x0 - sh z + z y (a'x) / den
    bool dead = sing, island = false;
    int lo = 1, hi = 0;
    if (ISL) {
        const I4 q = a.isl[bl];
        island = q[0] >= 0;
        if (island) {
            lo = q[1]; hi = q[2];
            const double xm = fi >= 0 ? x0(fi) : 0.0, xs = x0(q[0]);
            c = q[3] > 0 ? yk * (xm - xs) - sh : -(yk * (xs - xm) - sh);      // +- y_k (x_f - x_t - shiftAngle_k), + when m is the from end
            dead = false;
        }
        if (blockIdx.x == 0 && wave == 0) a.ig[bl] = island ? c : 0.0;
    }
    if (blockIdx.x == 0 && wave == 0) a.status[bl] = island ? 4 : (sing ? 3 : 0);
    const int b0 = (blockIdx.x * 4 + wave) * DC_COMBINE_ROWS;
    double shed_n = 0.0, shed_p = 0.0;
    for (int bus = b0; bus < min(b0 + DC_COMBINE_ROWS, a.n); ++bus) {
        double th = x0(bus) + c * a.Z[(size_t)bus * ld + bl] + a.slack_angle;
        if (bus == a.slack) th = a.slack_angle;
        if (dead) th = __longlong_as_double(0x7ff8000000000000LL);
        if (ISL) {
            const int pre = ((CInt)a.preorder)[bus];
            if (pre >= lo && pre <= hi) {
                th = __longlong_as_double(0x7ff8000000000000LL);
                shed_n += 1.0;
                shed_p += own ? a.RHS[(size_t)bus * ld + bl] : a.rhs0[(size_t)bus * 64];
            }
        }
        a.TH[(size_t)bus * ld + bl] = th;
    }
    if (ISL) {
        double* q = a.ipart + (size_t)(blockIdx.x * 4 + wave) * 2 * ld + bl;
        q[0] = shed_n; q[ld] = shed_p;
    }
}
// the shed record of every lane: the chunks of k_dc_combine<true> in ascending order
__global__ __launch_bounds__(64) void k_dc_island_final(const double* ipart, double* irec, int chunks, int ld) {
    const size_t bl = (size_t)blockIdx.x * 64 + threadIdx.x;
    double cnt = 0.0, net = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const double* q = ipart + (size_t)c * 2 * ld + bl;
        cnt += q[0]; net += q[ld];
    }
    irec[bl] = cnt; irec[(size_t)ld + bl] = net;                         // (row 2 of irec, g, is k_dc_combine's)
}

// ---- the rank-2 combine of the lanes with a second outage (jg_dc_set_outage_pairs) ------------------------------------------------------------
// theta = x0 + z1 c1 + z2 c2 with (I - Y A' Z) c = f0 on the lane's two branches, f0_k = y_k a_k' x0 - shiftAngle_k y_k (jg_dc_pair.hpp: the same 2 x 2
// system as the N-2 screen's).  Runs behind k_dc_combine on the lane groups that hold such a lane and writes ONLY those lanes.
struct DcCombine2Args {
    const double* Z; const double* Z2; const double* XS; const double* th0;
    const int* ginj; const int* groups;
    const int* of; const int* ot; const double* oy; const double* osh;
    const int* of2; const int* ot2; const int* obr2; const double* oy2; const double* osh2;
    double* TH; int* status;
    double slack_angle; int n, ld, slack;
};
__global__ __launch_bounds__(256) void k_dc_combine2(DcCombine2Args a) {
    const int wave = uniform(threadIdx.y);
    const int grp = ((CInt)a.groups)[blockIdx.y];
    const size_t ld = (size_t)a.ld, bl = (size_t)grp * 64 + threadIdx.x;
    if (a.obr2[bl] < 0) return;
    const bool own = a.ginj && ((CInt)a.ginj)[grp] != 0;
    auto x0 = [&](int bus) { return own ? a.XS[(size_t)bus * ld + bl] : a.th0[(size_t)bus * 64]; };
    auto dot = [&](int fi, int ti, auto&& v) { return (fi >= 0 ? v(fi) : 0.0) - (ti >= 0 ? v(ti) : 0.0); };
    auto z1 = [&](int bus) { return a.Z[(size_t)bus * ld + bl]; };
    auto z2 = [&](int bus) { return a.Z2[(size_t)bus * ld + bl]; };
    const int f1 = a.of[bl], t1 = a.ot[bl], f2 = a.of2[bl], t2 = a.ot2[bl];
    const double y1 = a.oy[bl], y2 = a.oy2[bl];
    const double a11 = 1.0 - y1 * dot(f1, t1, z1), a12 = -y1 * dot(f1, t1, z2);
    const double a21 = -y2 * dot(f2, t2, z1), a22 = 1.0 - y2 * dot(f2, t2, z2);
    const double g1 = y1 * dot(f1, t1, x0) - a.osh[bl], g2 = y2 * dot(f2, t2, x0) - a.osh2[bl];
    const double det = a11 * a22 - a12 * a21;
    const bool sing = fabs(det) < DC_SINGULAR;
    const double c1 = sing ? 0.0 : (a22 * g1 - a12 * g2) / det, c2 = sing ? 0.0 : (a11 * g2 - a21 * g1) / det;
    if (blockIdx.x == 0 && wave == 0) a.status[bl] = sing ? 3 : 0;
    const int b0 = (blockIdx.x * 4 + wave) * DC_COMBINE_ROWS;
    for (int bus = b0; bus < min(b0 + DC_COMBINE_ROWS, a.n); ++bus) {
        double th = x0(bus) + c1 * z1(bus) + c2 * z2(bus) + a.slack_angle;
        if (bus == a.slack) th = a.slack_angle;
        if (sing) th = __longlong_as_double(0x7ff8000000000000LL);
        a.TH[(size_t)bus * ld + bl] = th;
    }
}

// chunks in ascending order, strict comparison: ties go to the lowest branch index (as k_screen_final)
__global__ __launch_bounds__(64) void k_dc_screen_final(const double* part, const int* status, double* screen, int chunks, int ld, int batch) {
    const size_t bl = (size_t)blockIdx.x * 64 + threadIdx.x;
    double wl = 0.0, wf = 0.0, il = 0.0, jf = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const double* q = part + (size_t)c * 4 * ld + bl;
        const double l = q[0], i = q[ld], f = q[2 * (size_t)ld], j = q[3 * (size_t)ld];
        if (l > wl) { wl = l; il = i; }
        if (f > wf) { wf = f; jf = j; }
    }
    if (bl < (size_t)batch) {
        double* r = screen + bl * 5;
        r[0] = wl; r[1] = il; r[2] = wf; r[3] = jf; r[4] = (double)status[bl];
    }
}
// angle | status, scenario-major [batch][n + 1]: the record a gather carries
__global__ __launch_bounds__(256) void k_dc_pack(const double* TH, const int* status, double* dst, int n, int ld, int batch) {
    const size_t bl = (size_t)blockIdx.y * 64 + threadIdx.x;
    if (bl >= (size_t)batch) return;
    const int bus = blockIdx.x * 4 + threadIdx.y;
    if (bus < n) dst[bl * (n + 1) + bus] = TH[(size_t)bus * ld + bl];
    else if (bus == n) dst[bl * (n + 1) + n] = (double)status[bl];
}
__global__ void k_dc_fill_rhs(const double* rhs0, double* RHS, int n, int ld) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)n * ld) RHS[i] = rhs0[(i / ld) * 64];
}

// z = B^-1 (e_from - e_to) of every lane's outage
void sweep_outages(DcHandle* h) { sweep_pair(h->fac, h->stream, 1, nullptr, h->o_from, h->o_to, h->W, h->Z, h->ld, h->ld / 64, nullptr); }

void launch_combine(DcHandle* h) {
    DcCombineArgs c{};
    c.Z = h->Z; c.XS = h->XS; c.th0 = h->th0; c.ginj = h->n_glist ? h->ginj : nullptr;
    c.of = h->o_from; c.ot = h->o_to; c.obr = h->o_br; c.oy = h->o_y; c.osh = h->o_sh;
    c.TH = h->TH; c.status = h->status; c.slack_angle = h->slack_angle; c.n = h->n; c.ld = h->ld; c.slack = h->slack;
    const int per = 4 * DC_COMBINE_ROWS;
    if (h->n_isl) {                                                      // a batch without an island lane runs the kernel it always ran
        c.preorder = h->preorder; c.isl = (const I4*)h->isl; c.rhs0 = h->rhs0; c.RHS = h->RHS; c.ipart = h->ipart; c.ig = h->irec + 2 * (size_t)h->ld;
        hipLaunchKernelGGL(k_dc_combine<true>, dim3((h->n + per - 1) / per, h->ld / 64), dim3(64, 4), 0, h->stream, c);
    } else
        hipLaunchKernelGGL(k_dc_combine<false>, dim3((h->n + per - 1) / per, h->ld / 64), dim3(64, 4), 0, h->stream, c);
    if (!h->n_glist2) return;
    DcCombine2Args q{};
    q.Z = h->Z; q.Z2 = h->Z2; q.XS = h->XS; q.th0 = h->th0; q.ginj = c.ginj; q.groups = h->glist2;
    q.of = h->o_from; q.ot = h->o_to; q.oy = h->o_y; q.osh = h->o_sh;
    q.of2 = h->o2_from; q.ot2 = h->o2_to; q.obr2 = h->o2_br; q.oy2 = h->o2_y; q.osh2 = h->o2_sh;
    q.TH = h->TH; q.status = h->status; q.slack_angle = h->slack_angle; q.n = h->n; q.ld = h->ld; q.slack = h->slack;
    hipLaunchKernelGGL(k_dc_combine2, dim3((h->n + per - 1) / per, h->n_glist2), dim3(64, 4), 0, h->stream, q);
}

int launch_flows(DcHandle* h, bool store) {
    if (!h->nbr) { h->error = "jg_dc_set_branches has not been called"; return 1; }
    if (store && !h->flows) DC_TRY(dev_alloc(h, &h->flows, (size_t)h->nbr * h->ld, (const double*)nullptr, true));
    DcFlowArgs f{};
    f.TH = h->TH; f.bf = h->b_from; f.bt = h->b_to; f.by = h->b_y; f.bs = h->b_shift; f.rating = h->b_rating; f.obr = h->o_br; f.obr2 = h->o2_br;
    f.flows = store ? h->flows : nullptr; f.part = h->part; f.nbr = h->nbr; f.ld = h->ld;
    if (h->n_isl) { f.preorder = h->preorder; f.isl = (const I4*)h->isl; }
    launch_dc_flows(f, h->n_isl != 0, dim3((h->n_chunks + 3) / 4, h->ld / 64), h->stream);
    hipLaunchKernelGGL(k_dc_screen_final, dim3(h->ld / 64), dim3(64), 0, h->stream, h->part, h->status, h->screen, h->n_chunks, h->ld, h->batch);
    DC_HIP(hipGetLastError());
    return 0;
}

// the launch chain of a batch: sweeps for z, (sweeps for the groups with injections of their own,) combine.  One straight line on the handle's stream.
int solve_chain(DcHandle* h) {
    sweep_outages(h);
    if (h->n_glist) sweep_pair(h->fac, h->stream, 0, h->RHS, nullptr, nullptr, h->W, h->XS, h->ld, h->n_glist, h->glist);
    if (h->n_glist2) sweep_pair(h->fac, h->stream, 1, nullptr, h->o2_from, h->o2_to, h->W, h->Z2, h->ld, h->n_glist2, h->glist2);   // a second sweep pair, for the groups with a second outage only
    launch_combine(h);
    DC_HIP(hipGetLastError());
    return 0;
}

int dc_create(DcHandle* h, int64_t n64, const int64_t* colptr, const int64_t* rowval, const double* nzval, int64_t slack1, double slack_angle, int64_t batch, int device) {
    const int n = (int)n64;
    h->n = n; h->batch = (int)batch; h->ld = (int)((batch + 63) / 64 * 64); h->device = device; h->slack = (int)slack1 - 1; h->slack_angle = slack_angle;
    if (colptr[0] != 1) { h->error = "colptr is not 1-based"; return 1; }
    const int nnz = (int)(colptr[n] - 1);
    // the pattern is structurally symmetric with sorted rows (SparseMatrixCSC): the row-CSR pattern is the same pair of arrays; values are transposed entry by entry
    std::vector<int> rp(n + 1), ci(nnz);
    for (int j = 0; j <= n; ++j) rp[j] = (int)(colptr[j] - 1);
    for (int j = 0; j < n; ++j) {
        if (rp[j + 1] < rp[j]) { h->error = "colptr is not monotone"; return 1; }
        for (int p = rp[j]; p < rp[j + 1]; ++p) {
            ci[p] = (int)(rowval[p] - 1);
            if (ci[p] < 0 || ci[p] >= n || (p > rp[j] && ci[p] <= ci[p - 1])) { h->error = "rowval: rows of a column must be sorted, unique and in 1..n"; return 1; }
        }
    }
    std::vector<double> A(nnz);
    for (int r = 0; r < n; ++r)
        for (int q = rp[r]; q < rp[r + 1]; ++q) {
            const int c = ci[q];                                           // entry (r, c) of the row form = pointer of row r in column c
            const int* lo = ci.data() + rp[c]; const int* hi = ci.data() + rp[c + 1];
            const int* it = std::lower_bound(lo, hi, r);
            if (it == hi || *it != r) { h->error = "the nodal matrix pattern is not structurally symmetric"; return 1; }
            double v = nzval[it - ci.data()];
            if (r == h->slack || c == h->slack) v = (r == c) ? 1.0 : 0.0;   // the slack row and column leave the system (dcPowerFlow.jl:63-80): an identity row here
            A[q] = v;
        }
    BlockSymbolic S;
    if (analyze(n, rp.data(), ci.data(), DC_POLICY_NO_TOP, S) != 0) { h->error = "symbolic analysis failed (pattern must contain the diagonal)"; return 1; }
    DC_HIP(hipSetDevice(device));
    DC_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    DcFactor& F = h->fac;
    DC_TRY(factor_tables(h, F, n, S));
    DC_TRY(dev_alloc(h, &F.A, (size_t)nnz, A.data()));                       // slack row / column as identity
    DC_TRY(dev_alloc(h, &F.X, (size_t)S.n_entries + 1, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.dinv, (size_t)n, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &F.bad, (size_t)1, (const int*)nullptr, true));
    factor_numeric(F, h->stream);                                           // once
    DC_HIP(hipGetLastError());
    DC_TRY(build_sweep(h, F, F.fwd, forward_levels(n, S), S.l_ptr, S.l_ent, S.l_col, false));
    DC_TRY(build_sweep(h, F, F.bwd, S.bwd_level, S.u_ptr, S.u_ent, S.u_col, true));
    int bad = 0;
    DC_HIP(sync_copy(&bad, F.bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    dev_release(h, F.f_ent); dev_release(h, F.t_ptr); dev_release(h, F.t_a); dev_release(h, F.t_d); dev_release(h, F.t_b);
    dev_release(h, F.e_src); dev_release(h, F.diag); dev_release(h, F.A); dev_release(h, F.X); dev_release(h, F.bad);
    if (bad) { h->error = "zero or non-finite pivot in the DC nodal matrix (an island without the slack bus?)"; return 3; }
    const size_t ld = (size_t)h->ld;
    DC_TRY(dev_alloc(h, &h->rhs0, (size_t)n * 64, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->W0, ((size_t)n + 1) * 64, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->th0, (size_t)n * 64, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->W, ((size_t)n + 1) * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->Z, (size_t)n * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->TH, (size_t)n * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->o_from, ld, (const int*)nullptr, false));
    DC_TRY(dev_alloc(h, &h->o_to, ld, (const int*)nullptr, false));
    DC_TRY(dev_alloc(h, &h->o_br, ld, (const int*)nullptr, false));
    DC_HIP(sync_fill(h->o_from, 0xff, ld * sizeof(int), h->stream));       // -1: no outage
    DC_HIP(sync_fill(h->o_to, 0xff, ld * sizeof(int), h->stream));
    DC_HIP(sync_fill(h->o_br, 0xff, ld * sizeof(int), h->stream));
    DC_TRY(dev_alloc(h, &h->o_y, ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->o_sh, ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->status, ld, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->screen, ld * 5, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->ginj, ld / 64, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->glist, ld / 64, (const int*)nullptr, true));
    h->h_ginj.assign(ld / 64, 0);
    return 0;
}

void dc_destroy(DcHandle* h) {
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    dc_pair_free(h);
    dc_series_free(h);
    dc_transfer_free(h);
    dc_generator_free(h);
    dc_group_free(h);
    dc_chance_free(h);
    dc_cascade_free(h);
    for (void* p : h->allocs) hipFree(p);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

}  // namespace

int dc_base_solve(DcHandle* h) {
    if (h->h_rhs.empty()) { h->error = "jg_dc_set_rhs has not been called"; return 1; }
    DC_HIP(hipMemcpy2DAsync(h->rhs0, 64 * sizeof(double), h->h_rhs.data(), sizeof(double), sizeof(double), (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    sweep_pair(h->fac, h->stream, 0, h->rhs0, nullptr, nullptr, h->W0, h->th0, 64, 1, nullptr);
    DC_HIP(hipGetLastError());
    h->base_dirty = false;
    return 0;
}

void dc_handle_island_table(DcHandle* h) {
    if (!h->h_pre.empty()) return;
    h->h_pre.resize(h->n); h->h_blo.resize(h->nbr); h->h_bhi.resize(h->nbr); h->h_bside.resize(h->nbr);
    dc_island_table(h->n, h->nbr, h->h_from.data(), h->h_to.data(), h->h_y.data(), h->slack, h->h_pre.data(), h->h_blo.data(), h->h_bhi.data(), h->h_bside.data());
}

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_create(int64_t* out, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, int64_t slack, double slack_angle,
                 int64_t batch, int device) {
    if (!out || !colptr || !rowval || !nzval || n < 1 || n > (1 << 24) || slack < 1 || slack > n || batch < 1 || batch > (1 << 20)) return api_fail(1, "jg_dc_create: bad argument");
    DcHandle* h = new DcHandle();
    const int rc = jg::dc_create(h, n, colptr, rowval, nzval, slack, slack_angle, batch, device);
    if (rc) { const std::string msg = h->error; jg::dc_destroy(h); *out = 0; return api_fail(rc, msg); }
    *out = (int64_t)reinterpret_cast<intptr_t>(h);
    return 0;
}

void jg_dc_destroy(int64_t h) {
    if (h) jg::dc_destroy(reinterpret_cast<DcHandle*>(static_cast<intptr_t>(h)));
}

int jg_dc_dims(int64_t h, int64_t* dims) {
    DC_ENTER(h);
    if (!dims) return api_fail(1, "jg_dc_dims: null pointer");
    dims[0] = d->n; dims[1] = d->batch; dims[2] = d->ld; dims[3] = d->nbr; dims[4] = d->fac.n_entries; dims[5] = d->fac.n_fact_levels;
    dims[6] = (int64_t)d->fac.fwd.h_lev.size() - 1; dims[7] = (int64_t)d->fac.bwd.h_lev.size() - 1;
    dims[8] = (int64_t)(d->fac.fwd.launches.size() + d->fac.bwd.launches.size()); dims[9] = d->fac.fwd.terms + d->fac.bwd.terms;
    return 0;
}

int jg_dc_set_rhs(int64_t h, const double* rhs) {
    DC_ENTER(h);
    if (!rhs) return api_fail(1, "jg_dc_set_rhs: null pointer");
    d->h_rhs.assign(rhs, rhs + d->n);
    d->h_rhs[d->slack] = 0.0;
    d->base_dirty = true; d->solved = false;
    std::fill(d->h_ginj.begin(), d->h_ginj.end(), 0); d->n_glist = 0;
    return 0;
}

int jg_dc_set_injections(int64_t h, int64_t lane0, int64_t count, const double* rhs) {
    DC_ENTER(h);
    if (lane0 < 0 || count < 0 || lane0 + count > d->batch || (count && !rhs)) return api_fail(1, "jg_dc_set_injections: lanes out of range");
    if (d->h_rhs.empty()) return api_fail(1, "jg_dc_set_injections: jg_dc_set_rhs first");
    if (!count) return 0;
    const size_t n = (size_t)d->n, ld = (size_t)d->ld;
    if (!d->RHS) {
        DC_RET(jg::dev_alloc(d, &d->RHS, n * ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->XS, n * ld, (const double*)nullptr, true));
    }
    bool any = false;
    for (int g : d->h_ginj) any = any || g;
    if (!any) {                                                            // every lane starts from the base right-hand side
        if (d->base_dirty) DC_RET(jg::dc_base_solve(d));
        hipLaunchKernelGGL(jg::k_dc_fill_rhs, dim3((unsigned)((n * ld + 255) / 256)), dim3(256), 0, d->stream, d->rhs0, d->RHS, d->n, d->ld);
    }
    std::vector<double> t(n * (size_t)count);
    for (size_t s = 0; s < (size_t)count; ++s)
        for (size_t i = 0; i < n; ++i) t[i * count + s] = (int)i == d->slack ? 0.0 : rhs[s * n + i];
    DC_API_HIP(hipMemcpy2DAsync(d->RHS + lane0, ld * sizeof(double), t.data(), (size_t)count * sizeof(double), (size_t)count * sizeof(double), n, hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    for (int64_t s = lane0; s < lane0 + count; ++s) d->h_ginj[s / 64] = 1;
    std::vector<int> list;
    for (size_t g = 0; g < d->h_ginj.size(); ++g) if (d->h_ginj[g]) list.push_back((int)g);
    d->n_glist = (int)list.size();
    DC_API_HIP(jg::sync_copy(d->ginj, d->h_ginj.data(), d->h_ginj.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(jg::sync_copy(d->glist, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
    d->solved = false;
    return 0;
}

int jg_dc_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, const double* shift) {
    DC_ENTER(h);
    if (nbr < 1 || !from || !to || !admittance || !shift) return api_fail(1, "jg_dc_set_branches: bad argument");
    if (d->nbr) return api_fail(1, "jg_dc_set_branches: the branch table is already set");
    std::vector<int> f(nbr), t(nbr);
    for (int64_t k = 0; k < nbr; ++k) {
        if (from[k] < 1 || from[k] > d->n || to[k] < 1 || to[k] > d->n) return api_fail(1, "jg_dc_set_branches: bus index out of range");
        f[k] = (int)from[k] - 1; t[k] = (int)to[k] - 1;
    }
    d->h_from = f; d->h_to = t; d->h_y.assign(admittance, admittance + nbr); d->h_shift.assign(shift, shift + nbr);
    d->n_chunks = (int)((nbr + jg::DC_FLOW_BRANCHES - 1) / jg::DC_FLOW_BRANCHES);
    DC_RET(jg::dev_alloc(d, &d->b_from, (size_t)nbr, f.data()));
    DC_RET(jg::dev_alloc(d, &d->b_to, (size_t)nbr, t.data()));
    DC_RET(jg::dev_alloc(d, &d->b_y, (size_t)nbr, admittance));
    DC_RET(jg::dev_alloc(d, &d->b_shift, (size_t)nbr, shift));
    DC_RET(jg::dev_alloc(d, &d->part, (size_t)d->n_chunks * 4 * d->ld, (const double*)nullptr, true));
    d->nbr = (int)nbr;
    return 0;
}

int jg_dc_set_rating(int64_t h, const double* rating) {
    DC_ENTER(h);
    if (!d->nbr) return api_fail(1, "jg_dc_set_rating: jg_dc_set_branches first");
    if (!rating) { d->b_rating = nullptr; return 0; }                     // (the buffer stays with the handle)
    if (!d->rating_buf) DC_RET(jg::dev_alloc(d, &d->rating_buf, (size_t)d->nbr, (const double*)nullptr, true));
    DC_API_HIP(jg::sync_copy(d->rating_buf, rating, (size_t)d->nbr * sizeof(double), hipMemcpyHostToDevice, d->stream));
    d->b_rating = d->rating_buf;
    return 0;
}

// lanes lane0 .. : outage of branch[s] and, where branch2 is given and not 0, of branch2[s] as well
static int dc_set_lane_outages(DcHandle* d, const char* who, int64_t lane0, int64_t count, const int64_t* branch, const int64_t* branch2) {
    const std::string me = who;
    if (lane0 < 0 || count < 0 || lane0 + count > d->batch || (count && !branch)) return api_fail(1, me + ": lanes out of range");
    if (!d->nbr) return api_fail(1, me + ": jg_dc_set_branches first");
    if (!count) return 0;
    std::vector<int> of(count), ot(count), ob(count), of2(count, -1), ot2(count, -1), ob2(count, -1);
    std::vector<double> oy(count), os(count), oy2(count, 0.0), os2(count, 0.0);
    std::vector<int> isl(d->isl ? 4 * (size_t)count : 0), isl_m(count, 0);      // (a handle that never saw island mode 1 keeps no such table)
    for (size_t s = 0; s < isl.size(); s += 4) { isl[s] = -1; isl[s + 1] = 1; isl[s + 2] = 0; isl[s + 3] = 0; }
    bool second = false;
    for (int64_t s = 0; s < count; ++s) {
        int64_t k = branch[s] - 1, k2 = branch2 ? branch2[s] - 1 : -1;
        if (k < -1 || k >= d->nbr || k2 < -1 || k2 >= d->nbr) return api_fail(1, me + ": branch index out of range");
        if (k >= 0 && k == k2) return api_fail(1, me + ": the two outages of a lane must be different branches");
        if (k < 0) { k = k2; k2 = -1; }
        if (k < 0) { of[s] = ot[s] = ob[s] = -1; oy[s] = os[s] = 0.0; continue; }
        of[s] = d->h_from[k] == d->slack ? -1 : d->h_from[k];           // the slack's component of a = e_from - e_to is dropped
        ot[s] = d->h_to[k] == d->slack ? -1 : d->h_to[k];
        ob[s] = (int)k; oy[s] = d->h_y[k]; os[s] = d->h_shift[k] * d->h_y[k];
        if (d->island_mode == 1 && k2 < 0 && d->h_bside[k] != 0) {       // a bridge, alone in its lane: the right-hand side of the sweep is e_m
            const int m = d->h_bside[k] > 0 ? d->h_from[k] : d->h_to[k];
            of[s] = m == d->slack ? -1 : m; ot[s] = -1;
            isl[4 * s] = d->h_bside[k] > 0 ? d->h_to[k] : d->h_from[k]; isl[4 * s + 1] = d->h_blo[k]; isl[4 * s + 2] = d->h_bhi[k]; isl[4 * s + 3] = d->h_bside[k];
            isl_m[s] = m + 1;
        }
        if (k2 < 0) continue;
        second = true;
        of2[s] = d->h_from[k2] == d->slack ? -1 : d->h_from[k2];
        ot2[s] = d->h_to[k2] == d->slack ? -1 : d->h_to[k2];
        ob2[s] = (int)k2; oy2[s] = d->h_y[k2]; os2[s] = d->h_shift[k2] * d->h_y[k2];
    }
    if (second && !d->o2_br) {                                           // the first second outage of the handle
        const size_t ld = (size_t)d->ld;
        DC_RET(jg::dev_alloc(d, &d->o2_from, ld, (const int*)nullptr, false));
        DC_RET(jg::dev_alloc(d, &d->o2_to, ld, (const int*)nullptr, false));
        DC_RET(jg::dev_alloc(d, &d->o2_br, ld, (const int*)nullptr, false));
        DC_API_HIP(jg::sync_fill(d->o2_from, 0xff, ld * sizeof(int), d->stream));
        DC_API_HIP(jg::sync_fill(d->o2_to, 0xff, ld * sizeof(int), d->stream));
        DC_API_HIP(jg::sync_fill(d->o2_br, 0xff, ld * sizeof(int), d->stream));
        DC_RET(jg::dev_alloc(d, &d->o2_y, ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->o2_sh, ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->Z2, (size_t)d->n * ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->glist2, ld / 64, (const int*)nullptr, true));
        d->h_o2.assign(ld, -1);
    }
    DC_API_HIP(hipMemcpyAsync(d->o_from + lane0, of.data(), count * sizeof(int), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipMemcpyAsync(d->o_to + lane0, ot.data(), count * sizeof(int), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipMemcpyAsync(d->o_br + lane0, ob.data(), count * sizeof(int), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipMemcpyAsync(d->o_y + lane0, oy.data(), count * sizeof(double), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipMemcpyAsync(d->o_sh + lane0, os.data(), count * sizeof(double), hipMemcpyHostToDevice, d->stream));
    if (d->isl) {
        DC_API_HIP(hipMemcpyAsync(d->isl + 4 * lane0, isl.data(), isl.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
        std::copy(isl_m.begin(), isl_m.end(), d->h_isl_m.begin() + lane0);
        d->n_isl = (int)std::count_if(d->h_isl_m.begin(), d->h_isl_m.end(), [](int m) { return m != 0; });
    }
    std::vector<int> list;
    if (d->o2_br) {                                                      // (also a plain jg_dc_set_outages over lanes that held a pair)
        DC_API_HIP(hipMemcpyAsync(d->o2_from + lane0, of2.data(), count * sizeof(int), hipMemcpyHostToDevice, d->stream));
        DC_API_HIP(hipMemcpyAsync(d->o2_to + lane0, ot2.data(), count * sizeof(int), hipMemcpyHostToDevice, d->stream));
        DC_API_HIP(hipMemcpyAsync(d->o2_br + lane0, ob2.data(), count * sizeof(int), hipMemcpyHostToDevice, d->stream));
        DC_API_HIP(hipMemcpyAsync(d->o2_y + lane0, oy2.data(), count * sizeof(double), hipMemcpyHostToDevice, d->stream));
        DC_API_HIP(hipMemcpyAsync(d->o2_sh + lane0, os2.data(), count * sizeof(double), hipMemcpyHostToDevice, d->stream));
        std::copy(ob2.begin(), ob2.end(), d->h_o2.begin() + lane0);
        for (int g = 0; g < d->ld / 64; ++g)
            if (std::any_of(d->h_o2.begin() + g * 64, d->h_o2.begin() + (g + 1) * 64, [](int b) { return b >= 0; })) list.push_back(g);
        d->n_glist2 = (int)list.size();
        if (!list.empty()) DC_API_HIP(hipMemcpyAsync(d->glist2, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
    }
    DC_API_HIP(hipStreamSynchronize(d->stream));                         // the host vectors go out of scope
    d->solved = false;
    return 0;
}

int jg_dc_set_island_mode(int64_t h, int mode) {
    DC_ENTER(h);
    if (mode != 0 && mode != 1) return api_fail(1, "jg_dc_set_island_mode: mode is 0 (a bridge outage is skipped: status 3) or 1 (solved on the slack's island: status 4)");
    if (mode == 1 && !d->nbr) return api_fail(1, "jg_dc_set_island_mode: jg_dc_set_branches first");
    if (mode == 1 && !d->isl) {                                          // the table of the handle's grid and the lanes' records, once
        const size_t n = (size_t)d->n, ld = (size_t)d->ld;
        jg::dc_handle_island_table(d);
        DC_RET(jg::dev_alloc(d, &d->preorder, n, d->h_pre.data()));
        const int chunks = (d->n + 4 * jg::DC_COMBINE_ROWS - 1) / (4 * jg::DC_COMBINE_ROWS) * 4;
        DC_RET(jg::dev_alloc(d, &d->ipart, (size_t)chunks * 2 * ld, (const double*)nullptr, true));
        DC_RET(jg::dev_alloc(d, &d->irec, 3 * ld, (const double*)nullptr, true));
        std::vector<int> none(4 * ld);
        for (size_t s = 0; s < ld; ++s) { none[4 * s] = -1; none[4 * s + 1] = 1; none[4 * s + 2] = 0; none[4 * s + 3] = 0; }
        DC_RET(jg::dev_alloc(d, &d->isl, 4 * ld, none.data()));
        d->h_isl_m.assign(ld, 0);
    }
    d->island_mode = mode;
    return 0;
}

int jg_dc_get_islands(int64_t h, double* rec) {
    DC_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dc_get_islands: jg_dc_solve first");
    if (!rec) return api_fail(1, "jg_dc_get_islands: null pointer");
    std::fill(rec, rec + (size_t)d->batch * 4, 0.0);
    if (!d->n_isl) return 0;
    const size_t ld = (size_t)d->ld;
    const int chunks = (d->n + 4 * jg::DC_COMBINE_ROWS - 1) / (4 * jg::DC_COMBINE_ROWS) * 4;
    hipLaunchKernelGGL(jg::k_dc_island_final, dim3(d->ld / 64), dim3(64), 0, d->stream, d->ipart, d->irec, chunks, d->ld);
    DC_API_HIP(hipGetLastError());
    std::vector<double> t(3 * ld);
    DC_API_HIP(jg::sync_copy(t.data(), d->irec, 3 * ld * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    for (size_t s = 0; s < (size_t)d->batch; ++s)
        if (d->h_isl_m[s]) { rec[4 * s] = t[s]; rec[4 * s + 1] = t[ld + s]; rec[4 * s + 2] = (double)d->h_isl_m[s]; rec[4 * s + 3] = t[2 * ld + s]; }
    return 0;
}

int jg_dc_set_outages(int64_t h, int64_t lane0, int64_t count, const int64_t* branch) {
    DC_ENTER(h);
    return dc_set_lane_outages(d, "jg_dc_set_outages", lane0, count, branch, nullptr);
}

int jg_dc_set_outage_pairs(int64_t h, int64_t lane0, int64_t count, const int64_t* branch_a, const int64_t* branch_b) {
    DC_ENTER(h);
    if (count && !branch_b) return api_fail(1, "jg_dc_set_outage_pairs: null pointer");
    return dc_set_lane_outages(d, "jg_dc_set_outage_pairs", lane0, count, branch_a, branch_b);
}

int jg_dc_solve(int64_t h) {
    DC_ENTER(h);
    if (d->base_dirty) DC_RET(jg::dc_base_solve(d));
    DC_RET(jg::solve_chain(d));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    d->solved = true;
    return 0;
}

int jg_dc_get_angle(int64_t h, double* theta, int32_t* status) {
    DC_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dc_get_angle: jg_dc_solve first");
    const size_t n = (size_t)d->n, ld = (size_t)d->ld;
    if (theta) {
        std::vector<double> t(n * ld);
        DC_API_HIP(jg::sync_copy(t.data(), d->TH, n * ld * sizeof(double), hipMemcpyDeviceToHost, d->stream));
        for (size_t s = 0; s < (size_t)d->batch; ++s)
            for (size_t i = 0; i < n; ++i) theta[s * n + i] = t[i * ld + s];
    }
    if (status) DC_API_HIP(jg::sync_copy(status, d->status, (size_t)d->batch * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    return 0;
}

int jg_dc_angle_device(int64_t h, int64_t* info) {
    DC_ENTER(h);
    if (!info) return api_fail(1, "jg_dc_angle_device: null pointer");
    info[0] = (int64_t)reinterpret_cast<intptr_t>(d->TH); info[1] = d->ld; info[2] = (int64_t)reinterpret_cast<intptr_t>(d->status);
    return 0;
}

int jg_dc_get_flows(int64_t h, double* from) {
    DC_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dc_get_flows: jg_dc_solve first");
    if (!from) return api_fail(1, "jg_dc_get_flows: null pointer");
    DC_RET(jg::launch_flows(d, true));
    const size_t nb = (size_t)d->nbr, ld = (size_t)d->ld;
    std::vector<double> t(nb * ld);
    DC_API_HIP(jg::sync_copy(t.data(), d->flows, nb * ld * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    for (size_t s = 0; s < (size_t)d->batch; ++s)
        for (size_t k = 0; k < nb; ++k) from[s * nb + k] = t[k * ld + s];
    return 0;
}

int jg_dc_screen(int64_t h, double* rec) {
    DC_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dc_screen: jg_dc_solve first");
    if (!rec) return api_fail(1, "jg_dc_screen: null pointer");
    DC_RET(jg::launch_flows(d, false));
    DC_API_HIP(jg::sync_copy(rec, d->screen, (size_t)d->batch * 5 * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    return 0;
}

int jg_dc_screen_device(int64_t h, double* rec_dev) {
    DC_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dc_screen_device: jg_dc_solve first");
    if (!rec_dev) return api_fail(1, "jg_dc_screen_device: null pointer");
    DC_RET(jg::launch_flows(d, false));
    DC_API_HIP(hipMemcpyAsync(rec_dev, d->screen, (size_t)d->batch * 5 * sizeof(double), hipMemcpyDeviceToDevice, d->stream));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    return 0;
}

int jg_dc_pack_results_device(int64_t h, double* dst_dev) {
    DC_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_dc_pack_results_device: jg_dc_solve first");
    if (!dst_dev) return api_fail(1, "jg_dc_pack_results_device: null pointer");
    hipLaunchKernelGGL(jg::k_dc_pack, dim3((d->n + 1 + 3) / 4, d->ld / 64), dim3(64, 4), 0, d->stream, d->TH, d->status, dst_dev, d->n, d->ld, d->batch);
    DC_API_HIP(hipGetLastError());
    DC_API_HIP(hipStreamSynchronize(d->stream));
    return 0;
}

int jg_dc_time_kernel(int64_t h, int kernel, int reps, double* ms) {
    DC_ENTER(h);
    if (!ms || reps < 1 || kernel < 0 || kernel > 3) return api_fail(1, "jg_dc_time_kernel: bad argument");
    if (!d->solved) return api_fail(4, "jg_dc_time_kernel: jg_dc_solve first");
    DC_RET(jg::time_events(d->stream, reps, ms, d->error, [&]() -> int {
        if (kernel == 1) jg::sweep_outages(d);
        else if (kernel == 2) jg::launch_combine(d);
        else {
            if (kernel == 0) { const int rc = jg::solve_chain(d); if (rc) return rc; }
            return jg::launch_flows(d, false);
        }
        return 0;
    }));
    return 0;
}

}  // extern "C"
