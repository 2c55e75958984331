// jg_dc_pair.hip -- the DC N-2 screen over all pairs of a candidate list (jg_dc_pair.hpp has the algebra and the reference loop it stands for).
//
// Build: the sweep pair of jg_dc_sweep.hip over the candidates, DC_PAIR_LANES at a time, and k_pair_phi after each batch (the flow kernel's shape: a wave
// is 8 rows x 64 candidates, y_m (z[from_m] - z[to_m]), coalesced stores).  Screen of a row block [k0, k1): k_pair_screen solves the 2 x 2 systems and
// walks the rows of Phi once (a wave = DC_PAIR_TILE candidates k in registers x 64 consecutive l; Phi[m, k..], f0_m, 1 / rating_m through scalar loads,
// Phi[m, l..l+63] one coalesced vector load reused for every k of the tile; nothing is written per m); the records come out of the block's dense result by
// count (k_pair_rows<false>) / prefix sum over the rows (host, a few thousand integers) / ordered scatter (k_pair_rows<true>: ballot ranks, no atomics),
// so the list is sorted by (k, l) and a list that overflows keeps the first.  Every store is a vector store.
#include "jg_dc_pair.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/jgrid.h"
#include "jg_dc.hpp"
#include "jg_dc_abi.hpp"

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

// ---- the screen kernel -------------------------------------------------------------------------------------------------------------------
struct PairScreenArgs {
    const double* Phi; const double* f0; const double* rinv; const int* pos; const int* rbranch;
    const int* crow; const double* cdiag; const double* cf0;
    double* load; int* branch; int* count; double* det;         // [k1 - k0][ldk]; det nullable
    double thr; int rows, ldk, nk, k0, k1, kbase;                // kbase: k0 rounded down to a multiple of the tile (the scalar loads of a tile are 32-byte aligned)
};
__global__ __launch_bounds__(64 * DC_PAIR_WAVES) void k_pair_screen(PairScreenArgs a) {
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
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int k = kt + t;                                    // < ldk: the per-candidate arrays are [ldk], 0 behind nk
        const double dk = ((CDbl)a.cdiag)[k], fk = ((CDbl)a.cf0)[k];
        const int rk = ((CInt)a.crow)[k];
        const double pkl = a.Phi[(size_t)rk * ldk + l];          // Phi[k, l]: a row, coalesced
        const double plk = a.Phi[(size_t)rl * ldk + k];          // Phi[l, k]: a gather, once per pair
        const double a11 = 1.0 - dk, a22 = 1.0 - dl;
        const double det = a11 * a22 - pkl * plk;
        ok[t] = k >= a.k0 && k < a.k1 && lane_ok && l > k;
        sing[t] = fabs(det) < DC_SINGULAR;
        const bool live = ok[t] && !sing[t];
        ck[t] = live ? (a22 * fk + pkl * fl) / det : 0.0;
        cl[t] = live ? (plk * fk + a11 * fl) / det : 0.0;
        dt[t] = det; wl[t] = 0.0; il[t] = -1; cnt[t] = 0;
    }
    const double thr = a.thr;
    auto row = [&](int r, int pk, auto hit_c) {
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
#pragma unroll
        for (int t = 0; t < T; ++t) {
            double v = fma(pt[t], ck[t], fma(pl, cl[t], f0));
            if (HIT && (pk == kt + t || pk == l)) v = 0.0;       // the two outaged branches carry nothing
            const double ld = fabs(v) * ri;
            if (ld > wl[t]) { wl[t] = ld; il[t] = r; }           // rows ascend by branch index, strict comparison: ties go to the lowest branch (k_dc_flows)
            cnt[t] += ld > thr ? 1 : 0;
        }
    };
    for (int r = 0; r < a.rows; ++r) {
        const int pk = ((CInt)a.pos)[r];
        // only a row whose branch is one of this wave's candidates (at most T + 64 of the rows) needs the test per lane
        if ((unsigned)(pk - kt) < (unsigned)T || (unsigned)(pk - l0) < 64u) row(r, pk, std::true_type{});
        else row(r, pk, std::false_type{});
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

// ---- records out of the block's dense result: count, (prefix sum on the host), ordered scatter -----------------------------------------------
struct PairListArgs {
    const double* load; const int* branch; const int* count; const int* clabel;
    int* r_viol; int* r_isl; double* r_max;                      // per row of the block
    const long long* r_off; const long long* r_ioff;             // scatter: the row's first record / islanding entry
    double* rec; long long rec_cap; long long* isl; long long isl_cap;
    double thr; int ldk, nk, k0, k1;
};
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_pair_rows(PairListArgs a) {
    const int wave = uniform(threadIdx.y), lane = threadIdx.x;
    const int i = blockIdx.x * 4 + wave;
    const int k = a.k0 + i;
    if (k >= a.k1) return;
    const size_t ldk = (size_t)a.ldk;
    int nv = 0, ni = 0;
    double mx = 0.0;
    long long vb = SCATTER ? a.r_off[i] : 0, ib = SCATTER ? a.r_ioff[i] : 0;
    const int klab = ((CInt)a.clabel)[k];
    for (int l0 = (k + 1) / 64 * 64; l0 < a.nk; l0 += 64) {
        const int l = l0 + lane;
        const bool valid = l > k && l < a.nk;
        const double v = valid ? a.load[(size_t)i * ldk + l] : 0.0;
        const bool island = valid && v != v, viol = valid && v > a.thr;
        const unsigned long long mv = __ballot(viol), mi = __ballot(island);
        if (SCATTER) {
            const unsigned long long below = (1ull << lane) - 1ull;
            if (viol) {
                const long long at = vb + __popcll(mv & below);
                if (at < a.rec_cap) {
                    double* q = a.rec + at * 5;
                    q[0] = (double)klab; q[1] = (double)a.clabel[l]; q[2] = (double)a.branch[(size_t)i * ldk + l]; q[3] = v; q[4] = (double)a.count[(size_t)i * ldk + l];
                }
            }
            if (island) {
                const long long at = ib + __popcll(mi & below);
                if (at < a.isl_cap) { a.isl[at * 2] = klab; a.isl[at * 2 + 1] = a.clabel[l]; }
            }
            vb += __popcll(mv); ib += __popcll(mi);
        } else {
            nv += __popcll(mv); ni += __popcll(mi);
            if (valid && v > mx) mx = v;                        // (a NaN compares false)
        }
    }
    if (!SCATTER) {
        for (int s = 32; s; s >>= 1) mx = fmax(mx, __shfl_xor(mx, s, 64));
        if (lane == 0) { a.r_viol[i] = nv; a.r_isl[i] = ni; a.r_max[i] = mx; }
    }
}
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

void state_release(DcHandle* h, DcPairState*& slot) {
    DcPairState* p = slot;
    if (!p) return;
    hipStreamSynchronize(h->stream);
    dev_release(h, p->Phi); dev_release(h, p->row_branch); dev_release(h, p->row_pos); dev_release(h, p->row_mon); dev_release(h, p->row_f0);
    dev_release(h, p->row_rinv); dev_release(h, p->cand_row); dev_release(h, p->cand_label); dev_release(h, p->cand_diag); dev_release(h, p->cand_f0);
    dev_release(h, p->b_load); dev_release(h, p->b_branch); dev_release(h, p->b_count); dev_release(h, p->b_det);
    dev_release(h, p->r_viol); dev_release(h, p->r_isl); dev_release(h, p->r_max); dev_release(h, p->r_off); dev_release(h, p->r_ioff);
    dev_release(h, p->c_max); dev_release(h, p->rec); dev_release(h, p->isl); dev_release(h, p->cand_isl); dev_release(h, p->row_pre);
    delete p;
    slot = nullptr;
}
void pair_release(DcHandle* h) { state_release(h, h->pair); }

std::string bytes_text(size_t b) {
    char t[64];
    snprintf(t, sizeof t, "%zu bytes (%.2f GiB)", b, (double)b / (1024.0 * 1024.0 * 1024.0));
    return t;
}

// the build of Phi into `slot` (the pair screen's h->pair, or the state the series screen keeps): `extra` bytes the caller will ask for beside Phi are
// part of the memory question, `extra_text` names them in the refusal
int state_build(DcHandle* h, DcPairState*& slot, const char* who, const std::vector<int>& cand, const std::vector<int>& mon, int64_t budget, size_t extra,
                const std::string& extra_text, double* info, bool shed) {
    state_release(h, slot);
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
        h->error = std::string(who) + ": Phi needs " + bytes_text(phi_bytes) + " (" + std::to_string(nr) + " rows x " + std::to_string(ldk) + " candidates x 8) and " +
                   bytes_text(scratch) + " of scratch" + extra_text + "; the budget is " + bytes_text(allowed) + ", " + bytes_text(free_b) + " are free: fewer candidates or monitored branches, or a larger budget";
        return 5;
    }
    DcPairState* p = new DcPairState();
    slot = p;
    p->nk = nk; p->ldk = ldk; p->rows = nr; p->h_cand = cand;
    DC_TRY(dev_alloc(h, &p->Phi, (size_t)nr * ldk, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &p->row_branch, (size_t)nr, rows.data()));
    DC_TRY(dev_alloc(h, &p->row_pos, (size_t)nr, pos.data()));
    DC_TRY(dev_alloc(h, &p->row_mon, (size_t)nr, flag.data()));
    DC_TRY(dev_alloc(h, &p->row_f0, (size_t)nr, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &p->row_rinv, (size_t)nr, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &p->cand_row, (size_t)ldk, crow.data()));
    DC_TRY(dev_alloc(h, &p->cand_label, (size_t)ldk, clab.data()));
    DC_TRY(dev_alloc(h, &p->cand_diag, (size_t)ldk, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &p->cand_f0, (size_t)ldk, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &p->c_max, (size_t)ldk, (const double*)nullptr, true));
    if (shed) {
        if (h->h_pre.empty()) {                                  // the table of the handle's grid, once (jg_dc_set_island_mode makes the same)
            h->h_pre.resize(n); h->h_blo.resize(h->nbr); h->h_bhi.resize(h->nbr); h->h_bside.resize(h->nbr);
            dc_island_table(n, h->nbr, h->h_from.data(), h->h_to.data(), h->h_y.data(), h->slack, h->h_pre.data(), h->h_blo.data(), h->h_bhi.data(), h->h_bside.data());
        }
        p->shed = true;
        p->h_side.assign(nk, 0); p->h_lo.assign(nk, 1); p->h_hi.assign(nk, 0);
        std::vector<int> cisl((size_t)4 * ldk, 0), rpre(nr);
        for (int j = 0; j < ldk; ++j) cisl[4 * j + 1] = 1;
        for (int j = 0; j < nk; ++j)
            if (h->h_bside[cand[j]] != 0) {
                p->h_side[j] = cisl[4 * j] = h->h_bside[cand[j]]; p->h_lo[j] = cisl[4 * j + 1] = h->h_blo[cand[j]]; p->h_hi[j] = cisl[4 * j + 2] = h->h_bhi[cand[j]];
            }
        for (int r = 0; r < nr; ++r) rpre[r] = h->h_pre[h->h_from[rows[r]]];
        DC_TRY(dev_alloc(h, &p->cand_isl, (size_t)4 * ldk, cisl.data()));
        DC_TRY(dev_alloc(h, &p->row_pre, (size_t)nr, rpre.data()));
    }
    // scratch of the build: the lanes' outage buses and one lane batch of the sweeps
    int* of = nullptr; int* ot = nullptr; double* W = nullptr; double* Z = nullptr;
    DC_TRY(dev_alloc(h, &of, (size_t)ldb, (const int*)nullptr, false));
    DC_TRY(dev_alloc(h, &ot, (size_t)ldb, (const int*)nullptr, false));
    DC_TRY(dev_alloc(h, &W, ((size_t)n + 1) * ldb, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &Z, (size_t)n * ldb, (const double*)nullptr, true));
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
    dev_release(h, of); dev_release(h, ot); dev_release(h, W); dev_release(h, Z);
    if (rc) { const std::string msg = h->error; state_release(h, slot); h->error = msg; return rc; }
    p->build_ms[0] = sweep_ms + phi_ms; p->build_ms[1] = sweep_ms; p->build_ms[2] = phi_ms;
    info[5] = p->build_ms[0]; info[6] = sweep_ms; info[7] = phi_ms;
    return 0;
}

// the block's buffers for `rb` rows (and the determinants, on request); grown, never shrunk
int pair_block(DcHandle* h, int rb, bool want_det, long long rec_cap, long long isl_cap) {
    DcPairState* p = h->pair;
    if (rb > p->blk_rows || (want_det && !p->b_det)) {
        const int rows = std::max(rb, p->blk_rows);
        const bool det = want_det || p->b_det != nullptr;
        const size_t cells = (size_t)rows * p->ldk, need = cells * (det ? 24 : 16);
        dev_release(h, p->b_load); dev_release(h, p->b_branch); dev_release(h, p->b_count); dev_release(h, p->b_det);
        dev_release(h, p->r_viol); dev_release(h, p->r_isl); dev_release(h, p->r_max); dev_release(h, p->r_off); dev_release(h, p->r_ioff);
        p->blk_rows = 0;
        size_t free_b = 0, total_b = 0;
        DC_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b) {
            h->error = "jg_dc_pair_screen: a block of " + std::to_string(rows) + " rows needs " + bytes_text(need) + ", " + bytes_text(free_b) + " are free: screen fewer rows per call";
            return 5;
        }
        DC_TRY(dev_alloc(h, &p->b_load, cells, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &p->b_branch, cells, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &p->b_count, cells, (const int*)nullptr, true));
        if (det) DC_TRY(dev_alloc(h, &p->b_det, cells, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &p->r_viol, (size_t)rows, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &p->r_isl, (size_t)rows, (const int*)nullptr, true));
        DC_TRY(dev_alloc(h, &p->r_max, (size_t)rows, (const double*)nullptr, true));
        DC_TRY(dev_alloc(h, &p->r_off, (size_t)rows, (const long long*)nullptr, true));
        DC_TRY(dev_alloc(h, &p->r_ioff, (size_t)rows, (const long long*)nullptr, true));
        p->blk_rows = rows;
    }
    if (rec_cap > p->rec_cap) { dev_release(h, p->rec); p->rec_cap = 0; DC_TRY(dev_alloc(h, &p->rec, (size_t)rec_cap * 5, (const double*)nullptr, true)); p->rec_cap = rec_cap; }
    if (isl_cap > p->isl_cap) { dev_release(h, p->isl); p->isl_cap = 0; DC_TRY(dev_alloc(h, &p->isl, (size_t)isl_cap * 2, (const long long*)nullptr, true)); p->isl_cap = isl_cap; }
    return 0;
}

PairScreenArgs screen_args(DcHandle* h, int k0, int k1, double thr, bool det) {
    DcPairState* p = h->pair;
    PairScreenArgs a{};
    a.Phi = p->Phi; a.f0 = p->row_f0; a.rinv = p->row_rinv; a.pos = p->row_pos; a.rbranch = p->row_branch;
    a.crow = p->cand_row; a.cdiag = p->cand_diag; a.cf0 = p->cand_f0;
    a.load = p->b_load; a.branch = p->b_branch; a.count = p->b_count; a.det = det ? p->b_det : nullptr;
    a.thr = thr; a.rows = p->rows; a.ldk = p->ldk; a.nk = p->nk; a.k0 = k0; a.k1 = k1; a.kbase = k0 / DC_PAIR_TILE * DC_PAIR_TILE;
    return a;
}
void launch_screen(DcHandle* h, const PairScreenArgs& a) {
    const int tiles = (a.k1 - a.kbase + DC_PAIR_TILE - 1) / DC_PAIR_TILE;
    hipLaunchKernelGGL(k_pair_screen, dim3(a.ldk / 64, (tiles + DC_PAIR_WAVES - 1) / DC_PAIR_WAVES), dim3(64, DC_PAIR_WAVES), 0, h->stream, a);
}
PairListArgs list_args(DcHandle* h, int k0, int k1, double thr, long long rec_cap, long long isl_cap) {
    DcPairState* p = h->pair;
    PairListArgs a{};
    a.load = p->b_load; a.branch = p->b_branch; a.count = p->b_count; a.clabel = p->cand_label;
    a.r_viol = p->r_viol; a.r_isl = p->r_isl; a.r_max = p->r_max; a.r_off = p->r_off; a.r_ioff = p->r_ioff;
    a.rec = p->rec; a.rec_cap = rec_cap; a.isl = p->isl; a.isl_cap = isl_cap;
    a.thr = thr; a.ldk = p->ldk; a.nk = p->nk; a.k0 = k0; a.k1 = k1;
    return a;
}
void launch_stats(DcHandle* h, const PairListArgs& a) {
    DcPairState* p = h->pair;
    hipLaunchKernelGGL((k_pair_rows<false>), dim3((a.k1 - a.k0 + 3) / 4), dim3(64, 4), 0, h->stream, a);
    hipLaunchKernelGGL(k_pair_colmax, dim3((p->ldk + 255) / 256), dim3(256), 0, h->stream, p->b_load, p->c_max, p->ldk, p->nk, a.k0, a.k1);
}

struct PairOut {
    double* records; int64_t* islanding; int64_t* totals; double* worst;
    double* d_load; int32_t* d_branch; int32_t* d_count; double* d_det;
};
// the block's dense result of one quantity on the host: [k1 - k0][nk], 0 where l <= k
template <typename V, typename D>
int pair_dense(DcHandle* h, D* dst, const V* src, int k0, int rb) {
    const int nk = h->pair->nk, ldk = h->pair->ldk;
    std::vector<V> t((size_t)rb * ldk);
    DC_HIP(sync_copy(t.data(), src, t.size() * sizeof(V), hipMemcpyDeviceToHost, h->stream));
    for (int i = 0; i < rb; ++i)
        for (int l = 0; l < nk; ++l) dst[(size_t)i * nk + l] = l > k0 + i ? (D)t[(size_t)i * ldk + l] : D(0);
    return 0;
}
int pair_screen(DcHandle* h, int k0, int k1, double thr, long long rec_cap, long long isl_cap, const PairOut& o) {
    DcPairState* p = h->pair;
    const int rb = k1 - k0, nk = p->nk, ldk = p->ldk;
    DC_TRY(pair_block(h, rb, o.d_det != nullptr, rec_cap, isl_cap));
    dc_pair_state_rinv(h, p);
    launch_screen(h, screen_args(h, k0, k1, thr, o.d_det != nullptr));
    PairListArgs la = list_args(h, k0, k1, thr, rec_cap, isl_cap);
    launch_stats(h, la);
    DC_HIP(hipGetLastError());
    std::vector<int> nv(rb), ni(rb);
    std::vector<double> rmax(rb), cmax(ldk);
    DC_HIP(hipMemcpyAsync(nv.data(), p->r_viol, rb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipMemcpyAsync(ni.data(), p->r_isl, rb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipMemcpyAsync(rmax.data(), p->r_max, rb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    DC_HIP(sync_copy(cmax.data(), p->c_max, ldk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    std::vector<long long> off(rb), ioff(rb);
    long long viol = 0, isl = 0, pairs = 0;
    for (int i = 0; i < rb; ++i) { off[i] = viol; ioff[i] = isl; viol += nv[i]; isl += ni[i]; pairs += nk - 1 - (k0 + i); }
    const long long nrec = std::min(viol, rec_cap), nisl = std::min(isl, isl_cap);
    if (nrec || nisl) {
        DC_HIP(hipMemcpyAsync(p->r_off, off.data(), rb * sizeof(long long), hipMemcpyHostToDevice, h->stream));
        DC_HIP(hipMemcpyAsync(p->r_ioff, ioff.data(), rb * sizeof(long long), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL((k_pair_rows<true>), dim3((rb + 3) / 4), dim3(64, 4), 0, h->stream, la);
        DC_HIP(hipGetLastError());
        if (nrec) DC_HIP(hipMemcpyAsync(o.records, p->rec, (size_t)nrec * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (nisl) DC_HIP(hipMemcpyAsync(o.islanding, p->isl, (size_t)nisl * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        DC_HIP(hipStreamSynchronize(h->stream));                // (off / ioff go out of scope behind it)
    }
    o.totals[0] = pairs; o.totals[1] = viol; o.totals[2] = isl; o.totals[3] = nrec; o.totals[4] = nisl;
    o.totals[5] = (viol > rec_cap ? 1 : 0) | (isl > isl_cap ? 2 : 0);
    if (o.worst)
        for (int j = 0; j < nk; ++j) {
            double w = cmax[j];
            if (j >= k0 && j < k1) w = std::max(w, rmax[j - k0]);
            o.worst[j] = std::max(o.worst[j], w);
        }
    if (o.d_load) DC_TRY(pair_dense(h, o.d_load, (const double*)p->b_load, k0, rb));
    if (o.d_branch) DC_TRY(pair_dense(h, o.d_branch, (const int*)p->b_branch, k0, rb));
    if (o.d_count) DC_TRY(pair_dense(h, o.d_count, (const int*)p->b_count, k0, rb));
    if (o.d_det) DC_TRY(pair_dense(h, o.d_det, (const double*)p->b_det, k0, rb));
    return 0;
}

}  // namespace

void dc_pair_free(DcHandle* h) { pair_release(h); }
void dc_pair_state_free(DcHandle* h, DcPairState*& slot) { state_release(h, slot); }
int dc_pair_state_build(DcHandle* h, DcPairState*& slot, const char* who, const std::vector<int>& cand, const std::vector<int>& mon, int64_t budget,
                        size_t extra, const std::string& extra_text, double* info, bool shed) {
    return state_build(h, slot, who, cand, mon, budget, extra, extra_text, info, shed);
}
void dc_pair_state_rinv(DcHandle* h, DcPairState* p) {
    hipLaunchKernelGGL(k_pair_rinv, dim3((p->rows + 255) / 256), dim3(256), 0, h->stream, h->b_rating, p->row_branch, p->row_mon, p->row_rinv, p->rows);
}
std::string dc_pair_bytes_text(size_t b) { return bytes_text(b); }

int dc_pair_lists(DcHandle* d, const std::string& who, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, std::vector<int>& cand,
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

}  // namespace jg

using jg::DcHandle;

using jg::api_fail;

extern "C" {

int jg_dc_pair_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t budget_bytes, double* info) {
    DC_ENTER(h);
    if (!d->nbr) return api_fail(1, "jg_dc_pair_build: jg_dc_set_branches first");
    if (d->h_rhs.empty()) return api_fail(1, "jg_dc_pair_build: jg_dc_set_rhs first");
    if (nk < 2 || !candidates || !info || nm < 0 || (nm && !monitored)) return api_fail(1, "jg_dc_pair_build: two or more candidates, and info, are needed");
    std::vector<int> cand, mon;
    DC_RET(jg::dc_pair_lists(d, "jg_dc_pair_build", nk, candidates, nm, monitored, cand, mon));
    DC_RET(jg::dc_pair_state_build(d, d->pair, "jg_dc_pair_build", cand, mon, budget_bytes, 0, "", info));
    return 0;
}

int jg_dc_pair_screen(int64_t h, int64_t k0, int64_t k1, double threshold, int64_t capacity, double* records, int64_t island_capacity, int64_t* islanding,
                      int64_t* totals, double* worst, double* dense_load, int32_t* dense_branch, int32_t* dense_count, double* dense_det) {
    DC_ENTER(h);
    if (!d->pair) return api_fail(4, "jg_dc_pair_screen: jg_dc_pair_build first");
    if (!d->b_rating) return api_fail(1, "jg_dc_pair_screen: jg_dc_set_rating first (the loadings are |from| / rating)");
    if (k0 < 0 || k1 <= k0 || k1 > d->pair->nk) return api_fail(1, "jg_dc_pair_screen: rows [k0, k1) out of range");
    if (!(threshold >= 0.0) || capacity < 0 || island_capacity < 0 || (capacity && !records) || (island_capacity && !islanding) || !totals)
        return api_fail(1, "jg_dc_pair_screen: bad argument");
    jg::PairOut o{records, islanding, totals, worst, dense_load, dense_branch, dense_count, dense_det};
    DC_RET(jg::pair_screen(d, (int)k0, (int)k1, threshold, capacity, island_capacity, o));
    return 0;
}

int jg_dc_pair_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms) {
    DC_ENTER(h);
    if (!d->pair) return api_fail(4, "jg_dc_pair_time_kernel: jg_dc_pair_build first");
    if (!ms || reps < 1 || kernel < 0 || kernel > 1 || k0 < 0 || k1 <= k0 || k1 > d->pair->nk) return api_fail(1, "jg_dc_pair_time_kernel: bad argument");
    if (k1 - k0 > d->pair->blk_rows) return api_fail(4, "jg_dc_pair_time_kernel: jg_dc_pair_screen with a block of at least these rows first");
    const jg::PairScreenArgs sa = jg::screen_args(d, (int)k0, (int)k1, 1.0, false);
    const jg::PairListArgs la = jg::list_args(d, (int)k0, (int)k1, 1.0, 0, 0);
    DC_RET(jg::time_events(d->stream, reps, ms, d->error, [&]() -> int {
        if (kernel == 0) jg::launch_screen(d, sa);
        else jg::launch_stats(d, la);
        return 0;
    }));
    return 0;
}

int jg_dc_pair_release(int64_t h) {
    DC_ENTER(h);
    jg::dc_pair_free(d);
    return 0;
}

}  // extern "C"
