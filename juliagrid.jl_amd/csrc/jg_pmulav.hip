// jg_pmulav.hip -- batched PMU least-absolute-value state estimation (jg_pmulav.hpp has the model and the reference lines it stands for).  The iteration
// is jg_dclav.hip's, without a fixed state; here: the polar <-> rectangular passes, the branch and bus quantities from the rectangular estimate, the
// suspect pass, the C ABI.  Indices and coefficients are wave-uniform and go through scalar loads; every store is a vector store.
#include "jg_pmulav.hpp"
#include "jg_dc_abi.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/jgrid.h"
#include "jg_engine.hpp"
#include "jg_pf.hpp"

namespace jg {

namespace {

// ---- readings: (magnitude, angle) of a PMU -> its two rows of Z, scaled ---------------------------------------------------------------------------
struct PmuRectArgs { const double* MAG; const double* ANG; const double* SC; double* Z; int npmu, ld; };
__global__ __launch_bounds__(256) void k_pmu_rect(PmuRectArgs a) {
    const int i = blockIdx.x * 4 + uniform(threadIdx.y);
    if (i >= a.npmu) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(nullptr), o = (size_t)i * ld + bl;
    const double m = a.MAG[o];
    double s, c;
    sincos(a.ANG[o], &s, &c);
    a.Z[(size_t)(2 * i) * ld + bl] = ((CDbl)a.SC)[2 * i] * (m * c);
    a.Z[(size_t)(2 * i + 1) * ld + bl] = ((CDbl)a.SC)[2 * i + 1] * (m * s);
}

// ---- the estimate: (re, im) of a bus -> (magnitude, angle) ----------------------------------------------------------------------------------------
struct PmuPolarArgs { const double* TH; double* VM; double* VA; int nbus, ld; };
__global__ __launch_bounds__(256) void k_pmu_polar(PmuPolarArgs a) {
    const int b = blockIdx.x * 4 + uniform(threadIdx.y);
    if (b >= a.nbus) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(nullptr), o = (size_t)b * ld + bl;
    const double re = a.TH[o], im = a.TH[(size_t)a.nbus * ld + o];
    a.VM[o] = hypot(re, im);
    a.VA[o] = atan2(im, re);
}

// ---- branches: both ends' currents and powers, the series element, the charging power -------------------------------------------------------------
// param [nbr][16] as jg_nr_set_branches: yff, yft, ytf, ytt, y, tij (re, im each), g, b of the charging, 1 / tau.  The voltages are rectangular already, so
// pf::branch_ends takes magnitude 1 with (sin, cos) = (im, re): 1 x v is v to the bit
struct PmuBranchArgs { const double* TH; const int* from; const int* to; const int* on; const double* par; double* OUT; int nbr, nbus, ld; };
__global__ __launch_bounds__(256) void k_pmu_branch(PmuBranchArgs a) {
    const int k = blockIdx.x * 4 + uniform(threadIdx.y);
    if (k >= a.nbr) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(nullptr), plane = (size_t)a.nbr * ld, o = (size_t)k * ld + bl, im0 = (size_t)a.nbus * ld;
    CDbl p = (CDbl)a.par + (size_t)k * 16;
    const int i = ((CInt)a.from)[k], j = ((CInt)a.to)[k];
    const bool on = ((CInt)a.on)[k] == 1;
    const double vir = a.TH[(size_t)i * ld + bl], vii = a.TH[im0 + (size_t)i * ld + bl], vjr = a.TH[(size_t)j * ld + bl], vji = a.TH[im0 + (size_t)j * ld + bl];
    const pf::BranchEnds e = pf::branch_ends(pf::TwoPort{{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]}}, 1.0, 1.0, vii, vir, vji, vjr);
    // Vij = tij Vi - Vj, Is = y Vij; the loss Vij conj(Is); the charging power 0.5 conj(g + jb) (|Vi / tau|^2 + |Vj|^2)
    const double wr = p[10] * vir - p[11] * vii - vjr, wi = p[10] * vii + p[11] * vir - vji;
    const double isr = p[8] * wr - p[9] * wi, isi = p[8] * wi + p[9] * wr;
    const double m = 0.5 * (p[14] * p[14] * (vir * vir + vii * vii) + (vjr * vjr + vji * vji));
    // out of service: exact zeros by a select, whatever the lane's voltages are (a product with 0 would pass a NaN on and store -0)
    double* q = a.OUT + o;
    q[0] = on ? hypot(e.ifr, e.ifi) : 0.0;  q[plane] = on ? atan2(e.ifi, e.ifr) : 0.0;
    q[2 * plane] = on ? hypot(e.itr, e.iti) : 0.0;  q[3 * plane] = on ? atan2(e.iti, e.itr) : 0.0;
    q[4 * plane] = on ? hypot(isr, isi) : 0.0;  q[5 * plane] = on ? atan2(isi, isr) : 0.0;
    q[6 * plane] = on ? e.pf : 0.0;  q[7 * plane] = on ? e.qf : 0.0;
    q[8 * plane] = on ? e.pt : 0.0;  q[9 * plane] = on ? e.qt : 0.0;
    q[10 * plane] = on ? wr * isr + wi * isi : 0.0;  q[11 * plane] = on ? wi * isr - wr * isi : 0.0;
    q[12 * plane] = on ? p[12] * m : 0.0;  q[13 * plane] = on ? -(p[13] * m) : 0.0;
}
// the injection of a bus: its branch ends in list order, then the shunt |V|^2 conj(g + jb)
struct PmuBusArgs { const double* TH; const int* e_ptr; const int* e_idx; const double* sh_g; const double* sh_b; const double* OUT; double* INJ; int nbr, nbus, ld; };
__global__ __launch_bounds__(256) void k_pmu_bus(PmuBusArgs a) {
    const int b = blockIdx.x * 4 + uniform(threadIdx.y);
    if (b >= a.nbus) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(nullptr), plane = (size_t)a.nbr * ld, o = (size_t)b * ld + bl;
    double p = 0.0, q = 0.0;
    for (int t = ((CInt)a.e_ptr)[b]; t < ((CInt)a.e_ptr)[b + 1]; ++t) {
        const int c = ((CInt)a.e_idx)[t];
        const double* s = a.OUT + (size_t)(6 + 2 * (c & 1)) * plane + (size_t)(c >> 1) * ld + bl;
        p += s[0]; q += s[plane];
    }
    const double re = a.TH[o], im = a.TH[(size_t)a.nbus * ld + o], v2 = re * re + im * im;
    a.INJ[o] = p + v2 * ((CDbl)a.sh_g)[b];
    a.INJ[(size_t)a.nbus * ld + o] = q - v2 * ((CDbl)a.sh_b)[b];
}

// ---- suspects: rho per device, the flag, and per chunk of devices the count and the largest rho with its device ------------------------------------
struct PmuSuspectArgs { const double* R; const int* st; const double* SC; double* RHO; int* FLAG; double* part; int* CNT; int* WORST; double threshold; int npmu, ld, n_chunks; };
__global__ __launch_bounds__(256) void k_pmu_suspect(PmuSuspectArgs a) {
    const int chunk = blockIdx.x * 4 + uniform(threadIdx.y);
    const int i0 = chunk * PMULAV_DEVS;
    if (i0 >= a.npmu) return;
    const size_t ld = (size_t)a.ld, bl = lane_of(nullptr);
    double count = 0.0, best = -1.0, who = 0.0;
    for (int i = i0; i < min(i0 + PMULAV_DEVS, a.npmu); ++i) {
        const size_t o = (size_t)i * ld + bl;
        double rho = 0.0;
        if (((CInt)a.st)[2 * i]) rho = hypot(a.R[(size_t)(2 * i) * ld + bl] / ((CDbl)a.SC)[2 * i], a.R[(size_t)(2 * i + 1) * ld + bl] / ((CDbl)a.SC)[2 * i + 1]);
        const int f = rho > a.threshold;
        a.RHO[o] = rho;
        a.FLAG[o] = f;
        count += (double)f;
        if (rho > best) { best = rho; who = (double)i; }
    }
    double* p = a.part + (size_t)chunk * 3 * ld + bl;
    p[0] = count; p[ld] = best; p[2 * ld] = who;
}
__global__ __launch_bounds__(64) void k_pmu_suspect_finish(PmuSuspectArgs a) {
    const size_t ld = (size_t)a.ld, bl = lane_of(nullptr);
    double count = 0.0, best = -1.0, who = 0.0;
    for (int c = 0; c < a.n_chunks; ++c) {
        const double* p = a.part + (size_t)c * 3 * ld + bl;
        count += p[0];
        if (p[ld] > best) { best = p[ld]; who = p[2 * ld]; }
    }
    a.CNT[bl] = (int)count;
    a.WORST[bl] = (int)who;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
inline dim3 by4(int items, int groups) { return dim3((items + 3) / 4, groups); }
#define PMU_LAUNCH(kernel, grid, block, ...) hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, __VA_ARGS__)

void launch_rect(PmulavHandle* h) {
    PMU_LAUNCH(k_pmu_rect, by4(h->npmu, h->ld / 64), dim3(64, 4), PmuRectArgs{h->MAG, h->ANG, h->SC, h->Z, h->npmu, h->ld});
}
void launch_polar(PmulavHandle* h) {
    PMU_LAUNCH(k_pmu_polar, by4(h->nbus, h->ld / 64), dim3(64, 4), PmuPolarArgs{h->TH, h->VM, h->VA, h->nbus, h->ld});
}
void launch_branch(PmulavHandle* h) {
    PMU_LAUNCH(k_pmu_branch, by4(h->nbr, h->ld / 64), dim3(64, 4), PmuBranchArgs{h->TH, h->br_from, h->br_to, h->br_on, h->br_par, h->OUT, h->nbr, h->nbus, h->ld});
    PMU_LAUNCH(k_pmu_bus, by4(h->nbus, h->ld / 64), dim3(64, 4), PmuBusArgs{h->TH, h->e_ptr, h->e_idx, h->sh_g, h->sh_b, h->OUT, h->INJ, h->nbr, h->nbus, h->ld});
}
void launch_suspect(PmulavHandle* h, double threshold) {
    const PmuSuspectArgs a{h->R, h->st, h->SC, h->RHO, h->FLAG, h->spart, h->CNT, h->WORST, threshold, h->npmu, h->ld, h->n_schunks};
    PMU_LAUNCH(k_pmu_suspect, by4(h->n_schunks, h->ld / 64), dim3(64, 4), a);
    PMU_LAUNCH(k_pmu_suspect_finish, dim3(1, h->ld / 64), dim3(64), a);
}

// what this file holds per lane beside the iterates of the shared iteration
size_t pmulav_extra_bytes(size_t nbus, size_t npmu) {
    const size_t chunks = (npmu + PMULAV_DEVS - 1) / PMULAV_DEVS;
    return (2 * npmu + 2 * nbus + npmu + 3 * chunks) * sizeof(double) + (npmu + 2) * sizeof(int);
}

int pmulav_create(PmulavHandle* h, int64_t nbus, int64_t npmu, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, int64_t batch, int device) {
    h->nbus = (int)nbus; h->npmu = (int)npmu; h->n_schunks = (int)((npmu + PMULAV_DEVS - 1) / PMULAV_DEVS);
    std::vector<int32_t> rows(2 * npmu);
    for (int64_t i = 0; i < npmu; ++i) {
        if (status[i] != 0 && status[i] != 1) { h->error = "status must be 0 or 1"; return 1; }
        rows[2 * i] = rows[2 * i + 1] = status[i];
    }
    DC_TRY(lav_create(h, "jg_pmulav_create", pmulav_extra_bytes((size_t)nbus, (size_t)npmu), 2 * nbus, 2 * npmu, rowptr, col, val, rows.data(), batch, device));
    const size_t ld = (size_t)h->ld, P = (size_t)npmu, N = (size_t)nbus;
    h->h_scale.assign(2 * P, 1.0);
    DC_TRY(dev_alloc(h, &h->SC, 2 * P, h->h_scale.data()));
    for (double** p : {&h->MAG, &h->ANG, &h->RHO}) DC_TRY(dev_alloc(h, p, P * ld, (const double*)nullptr, true));
    for (double** p : {&h->VM, &h->VA}) DC_TRY(dev_alloc(h, p, N * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->FLAG, P * ld, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->spart, (size_t)h->n_schunks * 3 * ld, (const double*)nullptr, true));
    for (int** p : {&h->CNT, &h->WORST}) DC_TRY(dev_alloc(h, p, ld, (const int*)nullptr, true));
    return 0;
}

void pmulav_destroy(PmulavHandle* h) {
    lav_release(h);
    delete h;
}

// two planes [rows][ld] on the device -> [batch][rows][2] on the host
int fetch_pairs(PmulavHandle* d, const double* a, const double* b, size_t rows, double* out) {
    std::vector<double> t((size_t)d->batch * rows);
    for (int c = 0; c < 2; ++c) {
        DC_TRY(lav_fetch(d, c ? b : a, rows, t.data()));
        for (size_t k = 0; k < t.size(); ++k) out[2 * k + c] = t[k];
    }
    return 0;
}
int fetch_ints(PmulavHandle* h, const int* dev, size_t rows, int32_t* out) {
    const size_t ld = (size_t)h->ld;
    std::vector<int> t(rows * ld);
    DC_HIP(sync_copy(t.data(), dev, t.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    for (size_t s = 0; s < (size_t)h->batch; ++s)
        for (size_t i = 0; i < rows; ++i) out[s * rows + i] = t[i * ld + s];
    return 0;
}

}  // namespace
}  // namespace jg

using jg::PmulavHandle;
using jg::api_fail;

#define PMU_ENTER(h) DC_API_ENTER(jg::PmulavHandle, "null PMU LAV state estimation handle", h)

extern "C" {

int jg_pmulav_create(int64_t* out, int64_t buses, int64_t pmus, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, int64_t batch,
                     int device) {
    if (!out || !rowptr || !col || !val || !status || buses < 1 || buses > (1 << 23) || pmus < 1 || pmus > (1 << 25) || batch < 1 || batch > (1 << 20))
        return api_fail(1, "jg_pmulav_create: bad argument");
    PmulavHandle* h = new PmulavHandle();
    const int rc = jg::pmulav_create(h, buses, pmus, rowptr, col, val, status, batch, device);
    if (rc) { const std::string msg = h->error; jg::pmulav_destroy(h); *out = 0; return api_fail(rc, msg); }
    *out = (int64_t)reinterpret_cast<intptr_t>(h);
    return 0;
}

void jg_pmulav_destroy(int64_t h) {
    if (h) jg::pmulav_destroy(reinterpret_cast<PmulavHandle*>(static_cast<intptr_t>(h)));
}

int jg_pmulav_dims(int64_t h, int64_t* dims) {
    PMU_ENTER(h);
    if (!dims) return api_fail(1, "jg_pmulav_dims: null pointer");
    const jg::DcFactor& Y = d->fac.sym;
    dims[0] = d->nbus; dims[1] = d->npmu; dims[2] = d->batch; dims[3] = d->ld; dims[4] = d->nnz_gain; dims[5] = Y.n_entries; dims[6] = Y.n_fact_levels;
    dims[7] = (int64_t)Y.fwd.h_lev.size() - 1; dims[8] = (int64_t)Y.bwd.h_lev.size() - 1; dims[9] = (int64_t)(Y.fwd.launches.size() + Y.bwd.launches.size());
    dims[10] = (int64_t)d->bytes_per_lane; dims[11] = d->m_in / 2; dims[12] = d->factorisations; dims[13] = d->last_iterations;
    return 0;
}

int jg_pmulav_set_readings(int64_t h, int64_t lane0, int64_t count, const double* magnitude, const double* angle) {
    PMU_ENTER(h);
    if (lane0 < 0 || count < 1 || lane0 + count > d->batch || !magnitude || !angle) return api_fail(1, "jg_pmulav_set_readings: lanes out of range");
    for (size_t k = 0; k < (size_t)count * d->npmu; ++k)
        if (!std::isfinite(magnitude[k]) || !std::isfinite(angle[k])) return api_fail(1, "jg_pmulav_set_readings: a reading is not finite");
    DC_RET(jg::lav_upload(d, d->MAG, (size_t)d->npmu, magnitude, (size_t)lane0, (size_t)count));
    DC_RET(jg::lav_upload(d, d->ANG, (size_t)d->npmu, angle, (size_t)lane0, (size_t)count));
    d->have_z = true; d->solved = false;
    return 0;
}

int jg_pmulav_set_status(int64_t h, const int32_t* status) {
    PMU_ENTER(h);
    if (!status) return api_fail(1, "jg_pmulav_set_status: null pointer");
    for (int i = 0; i < d->npmu; ++i) if (status[i] != 0 && status[i] != 1) return api_fail(1, "jg_pmulav_set_status: status must be 0 or 1");
    for (int i = 0; i < d->npmu; ++i) d->h_st[2 * i] = d->h_st[2 * i + 1] = status[i];
    DC_RET(jg::lav_set_status(d));
    return 0;
}

int jg_pmulav_set_scale(int64_t h, const double* scale) {
    PMU_ENTER(h);
    if (!scale) return api_fail(1, "jg_pmulav_set_scale: null pointer");
    for (int i = 0; i < d->m; ++i) if (!std::isfinite(scale[i]) || !(scale[i] > 0.0)) return api_fail(1, "jg_pmulav_set_scale: a scale is not positive and finite");
    d->h_scale.assign(scale, scale + d->m);
    DC_API_HIP(jg::sync_copy(d->SC, d->h_scale.data(), (size_t)d->m * sizeof(double), hipMemcpyHostToDevice, d->stream));
    d->solved = false;
    return 0;
}

int jg_pmulav_set_initial(int64_t h, const double* magnitude, const double* angle) {
    PMU_ENTER(h);
    if (!magnitude || !angle) return api_fail(1, "jg_pmulav_set_initial: null pointer");
    const size_t B = (size_t)d->batch, N = (size_t)d->nbus;
    for (size_t k = 0; k < B * N; ++k)
        if (!std::isfinite(magnitude[k]) || !std::isfinite(angle[k])) return api_fail(1, "jg_pmulav_set_initial: a voltage is not finite");
    d->h_theta0.resize(B * 2 * N);
    for (size_t s = 0; s < B; ++s)
        for (size_t b = 0; b < N; ++b) {
            d->h_theta0[s * 2 * N + b] = magnitude[s * N + b] * std::cos(angle[s * N + b]);
            d->h_theta0[s * 2 * N + N + b] = magnitude[s * N + b] * std::sin(angle[s * N + b]);
        }
    d->have_init = true; d->solved = false;
    return 0;
}

int jg_pmulav_solve(int64_t h, int iteration, double tolerance) {
    PMU_ENTER(h);
    if (iteration < 0 || !(tolerance > 0.0)) return api_fail(1, "jg_pmulav_solve: iteration must not be negative, tolerance positive");
    if (!d->have_z) return api_fail(4, "jg_pmulav_solve: jg_pmulav_set_readings first");
    jg::launch_rect(d);
    DC_API_HIP(hipGetLastError());
    DC_RET(jg::lav_run(d, iteration, tolerance));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    d->solved = true; d->have_polar = false; d->have_flows = false;
    return 0;
}

int jg_pmulav_get_voltage(int64_t h, double* magnitude, double* angle, int32_t* status, double* objective, int32_t* iterations) {
    PMU_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_pmulav_get_voltage: jg_pmulav_solve first");
    const size_t B = (size_t)d->batch, ld = (size_t)d->ld, N = (size_t)d->nbus;
    const double nan = std::nan("");
    if (d->unobservable) {
        if (magnitude) std::fill(magnitude, magnitude + B * N, nan);
        if (angle) std::fill(angle, angle + B * N, nan);
        if (objective) std::fill(objective, objective + B, nan);
        if (status) std::fill(status, status + B, 1);
        if (iterations) std::fill(iterations, iterations + B, 0);
        return 0;
    }
    if (magnitude || angle) {
        if (!d->have_polar) { jg::launch_polar(d); DC_API_HIP(hipGetLastError()); d->have_polar = true; }
        if (magnitude) DC_RET(jg::lav_fetch(d, d->VM, N, magnitude));
        if (angle) DC_RET(jg::lav_fetch(d, d->VA, N, angle));
    }
    std::vector<int> t(ld);
    if (status) {
        DC_API_HIP(jg::sync_copy(t.data(), d->lstat, ld * sizeof(int), hipMemcpyDeviceToHost, d->stream));
        std::copy(t.begin(), t.begin() + B, status);
    }
    if (iterations) {
        DC_API_HIP(jg::sync_copy(t.data(), d->liter, ld * sizeof(int), hipMemcpyDeviceToHost, d->stream));
        std::copy(t.begin(), t.begin() + B, iterations);
    }
    if (objective) DC_RET(jg::lav_fetch(d, d->lres, 1, objective));
    return 0;
}

int jg_pmulav_get_residual(int64_t h, double* r) {
    PMU_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_pmulav_get_residual: jg_pmulav_solve first");
    if (!r) return api_fail(1, "jg_pmulav_get_residual: null pointer");
    if (d->unobservable) { std::fill(r, r + (size_t)d->batch * d->m, std::nan("")); return 0; }
    DC_RET(jg::lav_fetch(d, d->R, (size_t)d->m, r));
    return 0;
}

int jg_pmulav_get_dual(int64_t h, double* y, double* gap) {
    PMU_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_pmulav_get_dual: jg_pmulav_solve first");
    if (d->unobservable) {
        if (y) std::fill(y, y + (size_t)d->batch * d->m, std::nan(""));
        if (gap) std::fill(gap, gap + d->batch, std::nan(""));
        return 0;
    }
    if (y) DC_RET(jg::lav_fetch(d, d->Y, (size_t)d->m, y));
    if (gap) DC_RET(jg::lav_fetch(d, d->lres + (size_t)jg::DCLAV_LRES_GAP * d->ld, 1, gap));
    return 0;
}

int jg_pmulav_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const int8_t* status, const double* param, const double* shunt_g,
                           const double* shunt_b) {
    PMU_ENTER(h);
    if (nbr < 1 || nbr > (1 << 26) || !from || !to || !status || !param || !shunt_g || !shunt_b) return api_fail(1, "jg_pmulav_set_branches: bad argument");
    if (d->nbr) return api_fail(1, "jg_pmulav_set_branches: the branch table is already set");
    const int N = d->nbus;
    std::vector<int> f(nbr), t(nbr), on(nbr), e_ptr(N + 1, 0);
    for (int64_t k = 0; k < nbr; ++k) {
        if (from[k] < 1 || from[k] > N || to[k] < 1 || to[k] > N) return api_fail(1, "jg_pmulav_set_branches: bus index out of range");
        f[k] = (int)from[k] - 1; t[k] = (int)to[k] - 1; on[k] = status[k] == 1;
        e_ptr[f[k] + 1]++; e_ptr[t[k] + 1]++;
    }
    for (size_t k = 0; k < (size_t)nbr * 16; ++k) if (!std::isfinite(param[k])) return api_fail(1, "jg_pmulav_set_branches: a parameter is not finite");
    for (int b = 0; b < N; ++b) {
        if (!std::isfinite(shunt_g[b]) || !std::isfinite(shunt_b[b])) return api_fail(1, "jg_pmulav_set_branches: a shunt is not finite");
        e_ptr[b + 1] += e_ptr[b];
    }
    std::vector<int> e_idx(2 * nbr), fill(e_ptr.begin(), e_ptr.end() - 1);
    for (int64_t k = 0; k < nbr; ++k) { e_idx[fill[f[k]]++] = (int)(2 * k); e_idx[fill[t[k]]++] = (int)(2 * k + 1); }
    // the footprint, before anything of it is allocated
    const size_t need = ((size_t)jg::PMULAV_PLANES * nbr + 2 * (size_t)N) * d->ld * sizeof(double);
    size_t free_b = 0, total_b = 0;
    DC_API_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        char text[160];
        snprintf(text, sizeof text, "jg_pmulav_set_branches: %d lanes need %.1f MB of branch and bus results, %.1f MB are free: use a smaller batch", d->ld,
                 (double)need / 1048576.0, (double)free_b / 1048576.0);
        return api_fail(5, text);
    }
    DC_RET(jg::dev_alloc(d, &d->br_from, (size_t)nbr, f.data()));
    DC_RET(jg::dev_alloc(d, &d->br_to, (size_t)nbr, t.data()));
    DC_RET(jg::dev_alloc(d, &d->br_on, (size_t)nbr, on.data()));
    DC_RET(jg::dev_alloc(d, &d->br_par, (size_t)nbr * 16, param));
    DC_RET(jg::dev_alloc(d, &d->e_ptr, e_ptr.size(), e_ptr.data()));
    DC_RET(jg::dev_alloc(d, &d->e_idx, e_idx.size(), e_idx.data()));
    DC_RET(jg::dev_alloc(d, &d->sh_g, (size_t)N, shunt_g));
    DC_RET(jg::dev_alloc(d, &d->sh_b, (size_t)N, shunt_b));
    DC_RET(jg::dev_alloc(d, &d->OUT, (size_t)jg::PMULAV_PLANES * nbr * d->ld, (const double*)nullptr, true));
    DC_RET(jg::dev_alloc(d, &d->INJ, 2 * (size_t)N * d->ld, (const double*)nullptr, true));
    d->nbr = (int)nbr;
    return 0;
}

int jg_pmulav_get_flows(int64_t h, double* from_i, double* to_i, double* series_i, double* from_pq, double* to_pq, double* series_pq, double* charging_pq,
                        double* injection_pq) {
    PMU_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_pmulav_get_flows: jg_pmulav_solve first");
    if (!d->nbr) return api_fail(1, "jg_pmulav_get_flows: jg_pmulav_set_branches first");
    double* host[7] = {from_i, to_i, series_i, from_pq, to_pq, series_pq, charging_pq};
    const size_t B = (size_t)d->batch, nbr = (size_t)d->nbr, N = (size_t)d->nbus, plane = nbr * d->ld;
    if (d->unobservable) {
        for (double* p : host) if (p) std::fill(p, p + B * nbr * 2, std::nan(""));
        if (injection_pq) std::fill(injection_pq, injection_pq + B * N * 2, std::nan(""));
        return 0;
    }
    if (!d->have_flows) { jg::launch_branch(d); DC_API_HIP(hipGetLastError()); d->have_flows = true; }         // one pass per estimate, whoever asks first
    for (int k = 0; k < 7; ++k)
        if (host[k]) DC_RET(jg::fetch_pairs(d, d->OUT + (size_t)(2 * k) * plane, d->OUT + (size_t)(2 * k + 1) * plane, nbr, host[k]));
    if (injection_pq) DC_RET(jg::fetch_pairs(d, d->INJ, d->INJ + N * d->ld, N, injection_pq));
    return 0;
}

int jg_pmulav_suspect(int64_t h, double threshold, double* rho, int32_t* flag, int32_t* count, int32_t* worst) {
    PMU_ENTER(h);
    if (!d->solved) return api_fail(4, "jg_pmulav_suspect: jg_pmulav_solve first");
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) return api_fail(1, "jg_pmulav_suspect: the threshold must not be negative");
    const size_t B = (size_t)d->batch, P = (size_t)d->npmu;
    if (d->unobservable) {
        if (rho) std::fill(rho, rho + B * P, std::nan(""));
        if (flag) std::fill(flag, flag + B * P, 0);
        if (count) std::fill(count, count + B, 0);
        if (worst) std::fill(worst, worst + B, -1);
        return 0;
    }
    jg::launch_suspect(d, threshold);
    DC_API_HIP(hipGetLastError());
    d->threshold = threshold;
    if (rho) DC_RET(jg::lav_fetch(d, d->RHO, P, rho));
    if (flag) DC_RET(jg::fetch_ints(d, d->FLAG, P, flag));
    if (count) DC_RET(jg::fetch_ints(d, d->CNT, 1, count));
    if (worst) DC_RET(jg::fetch_ints(d, d->WORST, 1, worst));
    return 0;
}

int jg_pmulav_time_kernel(int64_t h, int kernel, int reps, double* ms) {
    PMU_ENTER(h);
    if (!ms || reps < 1 || kernel < 0 || kernel > 8) return api_fail(1, "jg_pmulav_time_kernel: bad argument");
    if (!d->solved || d->unobservable) return api_fail(4, "jg_pmulav_time_kernel: jg_pmulav_solve first, on an observable set");
    if (kernel == 7 && !d->nbr) return api_fail(4, "jg_pmulav_time_kernel: jg_pmulav_set_branches first");
    int rc;
    if (kernel <= 4) rc = jg::lav_time(d, kernel, reps, ms);
    else rc = jg::time_events(d->stream, reps, ms, d->error, [&]() -> int {
        // Z, the polar voltages, the branch results and the suspect tables are rewritten with what they hold (the suspect pass at its last threshold): the handle stays solved
        if (kernel == 5) jg::launch_rect(d);
        if (kernel == 6) jg::launch_polar(d);
        if (kernel == 7) jg::launch_branch(d);
        if (kernel == 8) jg::launch_suspect(d, d->threshold);
        return 0;
    });
    return rc ? api_fail(rc, d->error) : 0;
}

}  // extern "C"
