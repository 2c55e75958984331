// jg_dc_phi.hip -- the build of the kept outage sensitivities Phi and what the three screens on them share (jg_dc_phi.hpp).
//
// Build: the sweep pair of jg_dc_sweep.hip over the candidates, DC_PAIR_LANES at a time, and k_pair_phi after each batch (the flow kernel's shape: a wave
// is 8 rows x 64 candidates, y_m (z[from_m] - z[to_m]), coalesced stores).  Row flows of right-hand sides (F0 of the series screen, G of the transfer
// screen): the same loop over lane batches of right-hand sides, k_series_f0 after each batch (k_pair_phi's shape: a wave is 8 rows x 64 profiles,
// y_m ((theta[from_m] + slack angle) - (theta[to_m] + slack angle) - shiftAngle_m)).  Every store is a vector store.
#include "jg_dc_phi.hpp"

#include <cmath>
#include <cstdio>

namespace jg {

namespace {

constexpr int PAIR_PHI_ROWS = 8;        // rows of Phi per wave of k_pair_phi

// base-case flows on the rows of Phi, formed as k_dc_flows forms them (the slack angle added to both ends first)
__global__ void k_pair_f0(const double* th0, const int* rbranch, const int* bf, const int* bt, const double* by, const double* bs, double slack_angle,
                          double* f0, int rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int m = rbranch[r];
    f0[r] = by[m] * ((th0[(size_t)bf[m] * 64] + slack_angle) - (th0[(size_t)bt[m] * 64] + slack_angle) - bs[m]);
}
// Phi[r, col0 + lane] = y_m (z[from_m] - z[to_m]) for the candidates of one lane batch
struct PairPhiArgs { const double* Z; const int* rbranch; const int* bf; const int* bt; const double* by; double* Phi; int rows, ldb, ldk, col0; };
__global__ __launch_bounds__(256) void k_pair_phi(PairPhiArgs a) {
    const int wave = uniform(threadIdx.y);
    const int r0 = (blockIdx.x * 4 + wave) * PAIR_PHI_ROWS;
    const size_t ldb = (size_t)a.ldb, bl = (size_t)blockIdx.y * 64 + threadIdx.x;
    const size_t col = (size_t)a.col0 + bl;
    if (col >= (size_t)a.ldk) return;
    for (int r = r0; r < min(r0 + PAIR_PHI_ROWS, a.rows); ++r) {
        const int m = ((CInt)a.rbranch)[r];
        const int f = ((CInt)a.bf)[m], t = ((CInt)a.bt)[m];
        const double y = ((CDbl)a.by)[m];
        a.Phi[(size_t)r * a.ldk + col] = y * (a.Z[(size_t)f * ldb + bl] - a.Z[(size_t)t * ldb + bl]);
    }
}
__global__ void k_pair_cand(const double* Phi, const double* f0, const int* crow, double* cdiag, double* cf0, int nk, int ldk) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ldk) return;
    cdiag[j] = j < nk ? Phi[(size_t)crow[j] * ldk + j] : 0.0;
    cf0[j] = j < nk ? f0[crow[j]] : 0.0;
}
__global__ void k_pair_rinv(const double* rating, const int* rbranch, const int* mon, double* rinv, int rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const double q = rating[rbranch[r]];
    rinv[r] = (mon[r] && q > 0.0) ? 1.0 / q : 0.0;
}

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

// what left m over the bridge before the outage, for the bridge candidates `list` of a block: out[j][t] = s_k F[row of k][t]
__global__ void k_shed_gather(const double* F, const int* crow, const int* cisl, const int* list, double* out, int nb, int ldt, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    for (int j = blockIdx.y; j < nb; j += gridDim.y) {
        const int k = list[j];
        out[(size_t)j * T + t] = (cisl[4 * k] > 0 ? 1.0 : -1.0) * F[(size_t)crow[k] * ldt + t];
    }
}

}  // namespace

std::string dc_bytes_text(size_t b) {
    char t[64];
    snprintf(t, sizeof t, "%zu bytes (%.2f GiB)", b, (double)b / (1024.0 * 1024.0 * 1024.0));
    return t;
}

int dc_phi_build(DcHandle* h, DcPhi* p, const char* who, const std::vector<int>& cand, const std::vector<int>& mon, int64_t budget, size_t extra,
                 const std::string& extra_text, double* info, bool shed) {
    if (h->base_dirty) DC_TRY(dc_base_solve(h));
    const int nk = (int)cand.size(), ldk = (nk + 63) / 64 * 64, n = h->n;
    std::vector<int> rows, pos, flag, crow(ldk, 0), clab(ldk, 0);
    {
        std::vector<char> is_mon(h->nbr, 0);
        std::vector<int> cpos(h->nbr, -1);
        for (int m : mon) is_mon[m] = 1;
        for (int j = 0; j < nk; ++j) cpos[cand[j]] = j;
        for (int m = 0; m < h->nbr; ++m)
            if (is_mon[m] || cpos[m] >= 0) {
                if (cpos[m] >= 0) { crow[cpos[m]] = (int)rows.size(); clab[cpos[m]] = m + 1; }
                rows.push_back(m); pos.push_back(cpos[m]); flag.push_back(is_mon[m]);
            }
    }
    const int nr = (int)rows.size();
    const int ldb = std::min(ldk, DC_PAIR_LANES);
    const size_t phi_bytes = (size_t)nr * ldk * sizeof(double);
    const size_t scratch = ((size_t)2 * n + 1) * ldb * sizeof(double) + (size_t)2 * ldb * sizeof(int) +
                           (shed ? ((size_t)4 * ldk + nr) * sizeof(int) : 0);       // (shed mode: the candidates' intervals and the rows' preorder numbers)
    size_t free_b = 0, total_b = 0;
    DC_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t allowed = budget > 0 ? (size_t)budget : (size_t)(DC_PAIR_BUDGET * (double)free_b);
    info[0] = nr; info[1] = ldk; info[2] = (double)phi_bytes; info[3] = (double)free_b; info[4] = (double)allowed; info[5] = info[6] = info[7] = 0.0;
    if (phi_bytes + scratch + extra > allowed || phi_bytes + scratch + extra > free_b) {
        h->error = std::string(who) + ": Phi needs " + dc_bytes_text(phi_bytes) + " (" + std::to_string(nr) + " rows x " + std::to_string(ldk) + " candidates x 8) and " +
                   dc_bytes_text(scratch) + " of scratch" + extra_text + "; the budget is " + dc_bytes_text(allowed) + ", " + dc_bytes_text(free_b) + " are free: fewer candidates or monitored branches, or a larger budget";
        return 5;
    }
    p->nk = nk; p->ldk = ldk; p->rows = nr; p->h_cand = cand;
    DC_TRY(dev_alloc(h, p->mem, &p->Phi, (size_t)nr * ldk, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, p->mem, &p->row_branch, (size_t)nr, rows.data()));
    DC_TRY(dev_alloc(h, p->mem, &p->row_pos, (size_t)nr, pos.data()));
    DC_TRY(dev_alloc(h, p->mem, &p->row_mon, (size_t)nr, flag.data()));
    DC_TRY(dev_alloc(h, p->mem, &p->row_f0, (size_t)nr, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, p->mem, &p->row_rinv, (size_t)nr, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, p->mem, &p->cand_row, (size_t)ldk, crow.data()));
    DC_TRY(dev_alloc(h, p->mem, &p->cand_label, (size_t)ldk, clab.data()));
    DC_TRY(dev_alloc(h, p->mem, &p->cand_diag, (size_t)ldk, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, p->mem, &p->cand_f0, (size_t)ldk, (const double*)nullptr, true));
    if (shed) {
        dc_handle_island_table(h);
        p->shed = true;
        p->h_side.assign(nk, 0); p->h_lo.assign(nk, 1); p->h_hi.assign(nk, 0);
        std::vector<int> cisl((size_t)4 * ldk, 0), rpre(nr);
        for (int j = 0; j < ldk; ++j) cisl[4 * j + 1] = 1;
        for (int j = 0; j < nk; ++j)
            if (h->h_bside[cand[j]] != 0) {
                p->h_side[j] = cisl[4 * j] = h->h_bside[cand[j]]; p->h_lo[j] = cisl[4 * j + 1] = h->h_blo[cand[j]]; p->h_hi[j] = cisl[4 * j + 2] = h->h_bhi[cand[j]];
            }
        for (int r = 0; r < nr; ++r) rpre[r] = h->h_pre[h->h_from[rows[r]]];
        DC_TRY(dev_alloc(h, p->mem, &p->cand_isl, (size_t)4 * ldk, cisl.data()));
        DC_TRY(dev_alloc(h, p->mem, &p->row_pre, (size_t)nr, rpre.data()));
    }
    // scratch of the build (the state's until it is released below): the lanes' outage buses and one lane batch of the sweeps
    int* of = nullptr; int* ot = nullptr; double* W = nullptr; double* Z = nullptr;
    DC_TRY(dev_alloc(h, p->mem, &of, (size_t)ldb, (const int*)nullptr, false));
    DC_TRY(dev_alloc(h, p->mem, &ot, (size_t)ldb, (const int*)nullptr, false));
    DC_TRY(dev_alloc(h, p->mem, &W, ((size_t)n + 1) * ldb, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, p->mem, &Z, (size_t)n * ldb, (const double*)nullptr, true));
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int rc = 0;
    auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) { rc = 2; h->error = std::string(what) + ": " + hipGetErrorString(e); } return e == hipSuccess; };
    for (auto& e : ev) hip(hipEventCreate(&e), "hipEventCreate");
    hipLaunchKernelGGL(k_pair_f0, dim3((nr + 255) / 256), dim3(256), 0, h->stream, h->th0, p->row_branch, h->b_from, h->b_to, h->b_y, h->b_shift, h->slack_angle, p->row_f0, nr);
    double sweep_ms = 0.0, phi_ms = 0.0;
    std::vector<int> hf(ldb), ht(ldb);
    for (int c0 = 0; c0 < ldk && !rc; c0 += ldb) {
        for (int j = 0; j < ldb; ++j) {
            const int q = c0 + j;
            hf[j] = ht[j] = -1;
            if (q < nk) {
                const int m = cand[q];
                hf[j] = h->h_from[m] == h->slack ? -1 : h->h_from[m];     // the slack's component of a = e_from - e_to is dropped
                ht[j] = h->h_to[m] == h->slack ? -1 : h->h_to[m];
                if (shed && p->h_side[q] != 0) {                 // a bridge: e_m of its end on the slack's side (all zero where that is the slack)
                    if (p->h_side[q] < 0) hf[j] = ht[j];
                    ht[j] = -1;
                }
            }
        }
        if (!hip(sync_copy(of, hf.data(), ldb * sizeof(int), hipMemcpyHostToDevice, h->stream), "upload") ||
            !hip(sync_copy(ot, ht.data(), ldb * sizeof(int), hipMemcpyHostToDevice, h->stream), "upload")) break;
        const int groups = (std::min(ldb, ldk - c0) + 63) / 64;
        hip(hipEventRecord(ev[0], h->stream), "hipEventRecord");
        sweep_pair(h->fac, h->stream, 1, nullptr, of, ot, W, Z, ldb, groups, nullptr);
        hip(hipEventRecord(ev[1], h->stream), "hipEventRecord");
        PairPhiArgs a{Z, p->row_branch, h->b_from, h->b_to, h->b_y, p->Phi, nr, ldb, ldk, c0};
        hipLaunchKernelGGL(k_pair_phi, dim3((nr + 4 * PAIR_PHI_ROWS - 1) / (4 * PAIR_PHI_ROWS), groups), dim3(64, 4), 0, h->stream, a);
        hip(hipEventRecord(ev[2], h->stream), "hipEventRecord");
        hip(hipGetLastError(), "launch");
        if (!hip(hipEventSynchronize(ev[2]), "hipEventSynchronize")) break;
        float t1 = 0.f, t2 = 0.f;
        hip(hipEventElapsedTime(&t1, ev[0], ev[1]), "hipEventElapsedTime");
        hip(hipEventElapsedTime(&t2, ev[1], ev[2]), "hipEventElapsedTime");
        sweep_ms += t1; phi_ms += t2;
    }
    if (!rc) {
        hipLaunchKernelGGL(k_pair_cand, dim3((ldk + 255) / 256), dim3(256), 0, h->stream, p->Phi, p->row_f0, p->cand_row, p->cand_diag, p->cand_f0, nk, ldk);
        hip(hipGetLastError(), "launch");
        hip(hipStreamSynchronize(h->stream), "hipStreamSynchronize");
    }
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    dev_release(h, p->mem, of); dev_release(h, p->mem, ot); dev_release(h, p->mem, W); dev_release(h, p->mem, Z);
    if (rc) return rc;
    p->build_ms[0] = sweep_ms + phi_ms; p->build_ms[1] = sweep_ms; p->build_ms[2] = phi_ms;
    info[5] = p->build_ms[0]; info[6] = sweep_ms; info[7] = phi_ms;
    return 0;
}

void dc_phi_rinv(DcHandle* h, DcPhi* p) {
    hipLaunchKernelGGL(k_pair_rinv, dim3((p->rows + 255) / 256), dim3(256), 0, h->stream, h->b_rating, p->row_branch, p->row_mon, p->row_rinv, p->rows);
}

int dc_phi_lists(DcHandle* d, const std::string& who, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, std::vector<int>& cand,
                 std::vector<int>& mon) {
    cand.assign(nk, 0); mon.clear();
    for (int64_t j = 0; j < nk; ++j) {
        const int64_t m = candidates[j] - 1;
        if (m < 0 || m >= d->nbr) { d->error = who + ": candidate branch out of range"; return 1; }
        if (j && m <= cand[j - 1]) { d->error = who + ": the candidates must ascend strictly (no branch twice)"; return 1; }
        if (d->h_y[m] == 0.0) { d->error = who + ": candidate branch " + std::to_string(m + 1) + " is out of service"; return 1; }
        cand[j] = (int)m;
    }
    if (monitored) {
        for (int64_t j = 0; j < nm; ++j) {
            const int64_t m = monitored[j] - 1;
            if (m < 0 || m >= d->nbr) { d->error = who + ": monitored branch out of range"; return 1; }
            mon.push_back((int)m);
        }
    } else {
        for (int m = 0; m < d->nbr; ++m) if (d->h_y[m] != 0.0) mon.push_back(m);      // every branch in service
    }
    return 0;
}

size_t dc_phi_flows_scratch(const DcHandle* h, int ldt) { return ((size_t)3 * h->n + 1) * std::min(ldt, DC_PAIR_LANES) * sizeof(double); }

// the lane-batch loop of a build: F0 of the series screen with the shift angle, G of the transfer screen without
int dc_phi_row_flows(DcHandle* h, const DcPhi* p, int T, const double* rhs, bool shift, double* F, int ldt, double* ms) {
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

std::vector<int> dc_phi_row_labels(const DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, int ldt, double* info) {
    std::vector<char> in(h->nbr, 0);
    for (int m : mon) in[m] = 1;
    for (int m : cand) in[m] = 1;
    std::vector<int> label;
    for (int m = 0; m < h->nbr; ++m) if (in[m]) label.push_back(m + 1);
    for (int j = 8; j < 12; ++j) info[j] = 0.0;
    info[8] = (double)(label.size() * ldt * sizeof(double));
    return label;
}

int dc_phi_bridges(DcHandle* h, const DcPhi* p, std::vector<char>& bridge) {
    std::vector<double> diag(p->ldk);
    DC_HIP(sync_copy(diag.data(), p->cand_diag, diag.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    bridge.assign(p->nk, 0);
    for (int k = 0; k < p->nk; ++k) bridge[k] = !(p->shed && p->h_side[k] != 0) && std::fabs(1.0 - diag[k]) < DC_SINGULAR;
    return 0;
}

int dc_phi_shed_gather(DcHandle* h, const DcPhi* p, int k0, int k1, const double* F, int ldt, int T, double* out) {
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

int dc_phi_set_island_mode(DcHandle* d, const std::string& screen, int mode, int& flag) {
    const std::string me = "jg_dc_" + screen + "_set_island_mode: ";
    if (mode != 0 && mode != 1) return api_fail(1, me + "mode is 0 (a bridge candidate is skipped: status 3) or 1 (screened on the slack's island)");
    if (mode == 1 && !d->nbr) return api_fail(1, me + "jg_dc_set_branches first");
    flag = mode;
    return 0;
}

int dc_phi_get_shed_table(DcHandle* d, const std::string& screen, const DcPhi* p, int64_t k0, int64_t k1, int64_t* count, int64_t* labels, int64_t* buses,
                          int64_t* m, int64_t* side) {
    const std::string me = "jg_dc_" + screen + "_get_shed_table: ";
    if (!p) return api_fail(4, me + "jg_dc_" + screen + "_build first");
    if (!count || k0 < 0 || k1 < k0 || k1 > p->nk) return api_fail(1, me + "bad argument");
    int nb = 0;
    for (int k = (int)k0; p->shed && k < (int)k1; ++k) {
        if (p->h_side[k] == 0) continue;
        const int br = p->h_cand[k];
        if (labels) labels[nb] = br + 1;
        if (buses) buses[nb] = p->h_hi[k] - p->h_lo[k] + 1;
        if (m) m[nb] = (p->h_side[k] > 0 ? d->h_from[br] : d->h_to[br]) + 1;
        if (side) side[nb] = p->h_side[k];
        ++nb;
    }
    *count = nb;
    return 0;
}

}  // namespace jg
