// jg_gs.hip -- Gauss-Seidel AC power flow, one scenario per lane (jg_gs.hpp): the kernels of mismatch!, solve! and powerFlow! and the jg_gs_* exports of
// include/jgrid.h.
#include "jg_gs.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/jgrid.h"
#include "jg_dc_abi.hpp"
#include "jg_engine.hpp"

namespace jg {

namespace {

// Products and sums stay separate roundings, in every kernel alike: the loop of k_gs_run and the single-step kernels then give the same bits whatever
// the compiler would have fused in one place and not in the other, and the sums are the ones the reference forms.
#pragma clang fp contract(off)

struct GsArgs {
    const int* rp; const int* ci; const double* yr; const double* yi;
    const int* pq; const int* pv; const double* vg;
    double* vr; double* vi; const double* P; const double* Q;
    const int* ppos; const double* pdr; const double* pdi;
    int* iteration; int* status; double* stopP; double* stopQ;
    int npq, npv, ld, batch;
};

// what a lane holds in registers: its column and its outage
struct GsLane {
    size_t lane;
    int p[4];
    double dr[4], di[4];
};

__device__ __forceinline__ GsLane gs_lane(const GsArgs& a, int lane) {
    GsLane L;
    L.lane = (size_t)lane;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        L.p[k] = a.ppos[(size_t)k * a.ld + lane];
        L.dr[k] = a.pdr[(size_t)k * a.ld + lane];
        L.di[k] = a.pdi[(size_t)k * a.ld + lane];
    }
    return L;
}

// the lane's value at position j of the walk: the shared one, plus the lane's delta where j is one of its 4 positions
__device__ __forceinline__ void gs_value(const GsArgs& a, const GsLane& L, int j, double& yr, double& yi) {
    yr = ((CDbl)a.yr)[j];
    yi = ((CDbl)a.yi)[j];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (j == L.p[k]) { yr += L.dr[k]; yi += L.di[k]; }
}

// Row current of the lane: I += y v (SUB: I -= y v) over row i in index order, the diagonal value picked up on the way
template <bool SUB>
__device__ __forceinline__ void gs_row(const GsArgs& a, const GsLane& L, int i, double& Ir, double& Ii, double& Yr, double& Yi) {
    const CInt rp = (CInt)a.rp, ci = (CInt)a.ci;
    Yr = 0.0; Yi = 0.0;
    const int j1 = rp[i + 1];
    for (int j = rp[i]; j < j1; ++j) {
        const int row = ci[j];
        double yr, yi;
        gs_value(a, L, j, yr, yi);
        const double vr = a.vr[(size_t)row * a.ld + L.lane], vi = a.vi[(size_t)row * a.ld + L.lane];
        const double tr = yr * vr - yi * vi, ti = yr * vi + yi * vr;
        if (SUB) { Ir -= tr; Ii -= ti; } else { Ir += tr; Ii += ti; }
        if (row == i) { Yr = yr; Yi = yi; }
    }
}

// max that keeps a NaN once it has one, as the reference's max does
__device__ __forceinline__ double gs_max(double m, double x) { return (x > m || x != x) ? x : m; }

__device__ __forceinline__ void gs_div(double ar, double ai, double br, double bi, double& qr, double& qi) {
    const double den = br * br + bi * bi;
    qr = (ar * br + ai * bi) / den;
    qi = (ai * br - ar * bi) / den;
}

// mismatch!(analysis::AcPowerFlow{GaussSeidel}), acPowerFlow.jl:732-764
__device__ __forceinline__ void gs_mismatch(const GsArgs& a, const GsLane& L, double& stopP, double& stopQ) {
    const CInt pq = (CInt)a.pq, pv = (CInt)a.pv;
    stopP = 0.0; stopQ = 0.0;
    for (int k = 0; k < a.npq; ++k) {
        const int i = pq[k];
        double Ir = 0.0, Ii = 0.0, Yr, Yi;
        gs_row<false>(a, L, i, Ir, Ii, Yr, Yi);
        const size_t at = (size_t)i * a.ld + L.lane;
        const double vr = a.vr[at], vi = a.vi[at];
        stopP = gs_max(stopP, fabs((vr * Ir + vi * Ii) - a.P[at]));
        stopQ = gs_max(stopQ, fabs((vi * Ir - vr * Ii) - a.Q[at]));
    }
    for (int k = 0; k < a.npv; ++k) {
        const int i = pv[k];
        double Ir = 0.0, Ii = 0.0, Yr, Yi;
        gs_row<false>(a, L, i, Ir, Ii, Yr, Yi);
        const size_t at = (size_t)i * a.ld + L.lane;
        stopP = gs_max(stopP, fabs((a.vr[at] * Ir + a.vi[at] * Ii) - a.P[at]));
    }
}

// solve!(analysis::AcPowerFlow{GaussSeidel}), acPowerFlow.jl:997-1036: demand buses in place, generator buses in place, then their magnitudes
__device__ __forceinline__ void gs_sweep(const GsArgs& a, const GsLane& L) {
    const CInt pq = (CInt)a.pq, pv = (CInt)a.pv;
    const CDbl vg = (CDbl)a.vg;
    for (int k = 0; k < a.npq; ++k) {
        const int i = pq[k];
        const size_t at = (size_t)i * a.ld + L.lane;
        const double vr = a.vr[at], vi = a.vi[at];
        double Ir, Ii, Yr, Yi, dr, di;
        gs_div(a.P[at], -a.Q[at], vr, -vi, Ir, Ii);                  // (supply - demand)* / conj(v)
        gs_row<true>(a, L, i, Ir, Ii, Yr, Yi);
        gs_div(Ir, Ii, Yr, Yi, dr, di);
        a.vr[at] = vr + dr;
        a.vi[at] = vi + di;
    }
    for (int k = 0; k < a.npv; ++k) {
        const int i = pv[k];
        const size_t at = (size_t)i * a.ld + L.lane;
        const double vr = a.vr[at], vi = a.vi[at];
        double Ir = 0.0, Ii = 0.0, Yr, Yi, sr, si, dr, di;
        gs_row<false>(a, L, i, Ir, Ii, Yr, Yi);
        gs_div(a.P[at], vr * Ii - vi * Ir, vr, -vi, sr, si);         // (P + j imag(conj(v) I)) / conj(v)
        gs_div(sr - Ir, si - Ii, Yr, Yi, dr, di);
        a.vr[at] = vr + dr;
        a.vi[at] = vi + di;
    }
    for (int k = 0; k < a.npv; ++k) {
        const size_t at = (size_t)pv[k] * a.ld + L.lane;
        const double vr = a.vr[at], vi = a.vi[at], m = hypot(vr, vi), g = vg[k];
        a.vr[at] = g * vr / m;
        a.vi[at] = g * vi / m;
    }
}

__global__ __launch_bounds__(64) void k_gs_mismatch(GsArgs a) {
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= a.batch) return;
    const GsLane L = gs_lane(a, lane);
    double sp, sq;
    gs_mismatch(a, L, sp, sq);
    a.stopP[lane] = sp;
    a.stopQ[lane] = sq;
}

__global__ __launch_bounds__(64) void k_gs_sweep(GsArgs a) {
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= a.batch) return;
    const GsLane L = gs_lane(a, lane);
    gs_sweep(a, L);
    a.iteration[lane] += 1;
}

// powerFlow!(analysis; iteration, tolerance), acPowerFlow.jl:1406-1420, for a lane: status 0 converged, 1 the limit, 3 a maximum that is not finite
__global__ __launch_bounds__(64) void k_gs_run(GsArgs a, int limit, double tolerance) {
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= a.batch) return;
    const GsLane L = gs_lane(a, lane);
    int it = 0, st;
    double sp, sq;
    for (;;) {
        gs_mismatch(a, L, sp, sq);
        if (sp < tolerance && sq < tolerance) { st = 0; break; }
        if (!(fabs(sp) <= 1.79769313486231570815e308) || !(fabs(sq) <= 1.79769313486231570815e308)) { st = 3; break; }
        if (it == limit) { st = 1; break; }
        gs_sweep(a, L);
        ++it;
    }
    a.iteration[lane] = it;
    a.status[lane] = st;
    a.stopP[lane] = sp;
    a.stopQ[lane] = sq;
}

GsArgs gs_args(const GsHandle* h) {
    GsArgs a{};
    a.rp = h->rp; a.ci = h->ci; a.yr = h->yr; a.yi = h->yi; a.pq = h->pq; a.pv = h->pv; a.vg = h->vg;
    a.vr = h->vr; a.vi = h->vi; a.P = h->P; a.Q = h->Q; a.ppos = h->ppos; a.pdr = h->pdr; a.pdi = h->pdi;
    a.iteration = h->iteration; a.status = h->status; a.stopP = h->stopP; a.stopQ = h->stopQ;
    a.npq = h->npq; a.npv = h->npv; a.ld = h->ld; a.batch = h->batch;
    return a;
}

void launch_mismatch(GsHandle* h) { hipLaunchKernelGGL(k_gs_mismatch, dim3(h->ld / 64), dim3(64), 0, h->stream, gs_args(h)); }
void launch_sweep(GsHandle* h) { hipLaunchKernelGGL(k_gs_sweep, dim3(h->ld / 64), dim3(64), 0, h->stream, gs_args(h)); }
void launch_run(GsHandle* h, int limit, double tolerance) { hipLaunchKernelGGL(k_gs_run, dim3(h->ld / 64), dim3(64), 0, h->stream, gs_args(h), limit, tolerance); }

// host [count][n] (stride 0: one [n] for every lane of the range) into rows of a [n][ld] device array, lanes lane0 .. lane0 + count - 1
int put_lanes(GsHandle* h, double* dst, int64_t lane0, int64_t count, const double* src, int64_t stride) {
    const size_t n = (size_t)h->n, c = (size_t)count;
    std::vector<double> t(n * c);
    for (size_t s = 0; s < c; ++s)
        for (size_t i = 0; i < n; ++i) t[i * c + s] = src[s * (size_t)stride + i];
    DC_HIP(hipMemcpy2DAsync(dst + lane0, (size_t)h->ld * sizeof(double), t.data(), c * sizeof(double), c * sizeof(double), n, hipMemcpyHostToDevice, h->stream));
    DC_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// [rows][ld] device array -> host [rows][batch]
template <typename T>
int get_rows(GsHandle* h, const T* src, size_t rows, std::vector<T>& out) {
    out.resize(rows * (size_t)h->batch);
    DC_HIP(hipMemcpy2DAsync(out.data(), (size_t)h->batch * sizeof(T), src, (size_t)h->ld * sizeof(T), (size_t)h->batch * sizeof(T), rows, hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int gs_set_setpoint(GsHandle* h, const double* setpoint) {
    std::vector<double> g(h->npv);
    for (int k = 0; k < h->npv; ++k) g[k] = setpoint[h->h_pv[k]];
    if (h->npv) DC_HIP(sync_copy(h->vg, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return 0;
}

int gs_set_ybus(GsHandle* h, const double* yt) {
    std::vector<double> re(h->nnz), im(h->nnz);
    for (int p = 0; p < h->nnz; ++p) { re[p] = yt[2 * p]; im[p] = yt[2 * p + 1]; }
    DC_HIP(sync_copy(h->yr, re.data(), re.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    DC_HIP(sync_copy(h->yi, im.data(), im.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return 0;
}

int gs_create(GsHandle* h, int64_t n64, const int64_t* colptr, const int64_t* rowval, const double* yt, const int8_t* type, int64_t slack, const double* setpoint,
              int64_t batch, int device) {
    const int n = (int)n64;
    h->n = n; h->batch = (int)batch; h->ld = (int)((batch + 63) / 64 * 64); h->device = device;
    if (colptr[0] != 1) { h->error = "colptr is not 1-based"; return 1; }
    for (int j = 0; j < n; ++j)
        if (colptr[j + 1] < colptr[j]) { h->error = "colptr is not monotone"; return 1; }
    if (colptr[n] - 1 > (int64_t)1 << 30) { h->error = "too many stored entries"; return 1; }
    const int nnz = h->nnz = (int)(colptr[n] - 1);
    std::vector<int> rp(n + 1), ci(nnz), pq, pv;
    for (int j = 0; j <= n; ++j) rp[j] = (int)(colptr[j] - 1);
    for (int p = 0; p < nnz; ++p) {
        if (rowval[p] < 1 || rowval[p] > n) { h->error = "rowval: rows must be in 1..n"; return 1; }
        ci[p] = (int)rowval[p] - 1;
    }
    for (int i = 0; i < n; ++i) {
        if (type[i] == 1) pq.push_back(i);
        else if (type[i] == 2) pv.push_back(i);
        else if (type[i] != 3 || i != slack - 1) { h->error = "bus types: 1, 2, and 3 on the slack bus alone"; return 1; }
    }
    if (type[slack - 1] != 3) { h->error = "the slack bus is not of type 3"; return 1; }
    h->npq = (int)pq.size(); h->npv = (int)pv.size(); h->h_pv = pv;
    DC_HIP(hipSetDevice(device));
    DC_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t ld = (size_t)h->ld, cells = (size_t)n * ld;
    DC_TRY(dev_alloc(h, &h->rp, rp.size(), rp.data()));
    DC_TRY(dev_alloc(h, &h->ci, ci.size(), ci.data()));
    DC_TRY(dev_alloc(h, &h->yr, (size_t)nnz, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->yi, (size_t)nnz, (const double*)nullptr, true));
    DC_TRY(gs_set_ybus(h, yt));
    DC_TRY(dev_alloc(h, &h->pq, pq.size(), pq.data()));
    DC_TRY(dev_alloc(h, &h->pv, pv.size(), pv.data()));
    DC_TRY(dev_alloc(h, &h->vg, pv.size(), (const double*)nullptr, true));
    DC_TRY(gs_set_setpoint(h, setpoint));
    DC_TRY(dev_alloc(h, &h->vr, cells, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->vi, cells, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->P, cells, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->Q, cells, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->ppos, 4 * ld, (const int*)nullptr, false));
    DC_HIP(sync_fill(h->ppos, 0xff, 4 * ld * sizeof(int), h->stream));     // -1: no outage
    DC_TRY(dev_alloc(h, &h->pdr, 4 * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->pdi, 4 * ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->iteration, ld, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->status, ld, (const int*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->stopP, ld, (const double*)nullptr, true));
    DC_TRY(dev_alloc(h, &h->stopQ, ld, (const double*)nullptr, true));
    return 0;
}

void gs_destroy(GsHandle* h) {
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void* p : h->allocs) hipFree(p);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

}  // namespace

}  // namespace jg

using jg::api_fail;
using jg::GsHandle;

#define GS_ENTER(h) DC_API_ENTER(jg::GsHandle, "null Gauss-Seidel handle", h)

extern "C" {

int jg_gs_create(int64_t* out, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* yt, const int8_t* type, int64_t slack,
                 const double* setpoint, int64_t batch, int device) {
    if (!out || !colptr || !rowval || !yt || !type || !setpoint || n < 1 || n > (1 << 24) || slack < 1 || slack > n || batch < 1 || batch > (1 << 20))
        return api_fail(1, "jg_gs_create: bad argument");
    GsHandle* h = new GsHandle();
    const int rc = jg::gs_create(h, n, colptr, rowval, yt, type, slack, setpoint, batch, device);
    if (rc) { const std::string msg = h->error; jg::gs_destroy(h); *out = 0; return api_fail(rc, msg); }
    *out = (int64_t)reinterpret_cast<intptr_t>(h);
    return 0;
}

void jg_gs_destroy(int64_t h) {
    if (h) jg::gs_destroy(reinterpret_cast<GsHandle*>(static_cast<intptr_t>(h)));
}

int jg_gs_set_ybus(int64_t h, const double* yt) {
    GS_ENTER(h);
    if (!yt) return api_fail(1, "jg_gs_set_ybus: null pointer");
    DC_RET(jg::gs_set_ybus(d, yt));
    return 0;
}

int jg_gs_set_injection(int64_t h, int64_t lane0, int64_t count, const double* active, const double* reactive, int64_t stride) {
    GS_ENTER(h);
    if (lane0 < 0 || count < 1 || lane0 + count > d->batch || !active || !reactive || (stride != 0 && stride != d->n)) return api_fail(1, "jg_gs_set_injection: bad argument");
    DC_RET(jg::put_lanes(d, d->P, lane0, count, active, stride));
    DC_RET(jg::put_lanes(d, d->Q, lane0, count, reactive, stride));
    return 0;
}

int jg_gs_set_setpoint(int64_t h, const double* setpoint) {
    GS_ENTER(h);
    if (!setpoint) return api_fail(1, "jg_gs_set_setpoint: null pointer");
    DC_RET(jg::gs_set_setpoint(d, setpoint));
    return 0;
}

int jg_gs_set_voltage(int64_t h, const double* magnitude, const double* angle, int64_t stride) {
    GS_ENTER(h);
    if (!magnitude || !angle || (stride != 0 && stride != d->n)) return api_fail(1, "jg_gs_set_voltage: bad argument");
    const size_t m = (size_t)d->n * (stride ? (size_t)d->batch : 1);
    std::vector<double> re(m), im(m);
    for (size_t k = 0; k < m; ++k) { re[k] = magnitude[k] * std::cos(angle[k]); im[k] = magnitude[k] * std::sin(angle[k]); }   // magnitude * cis(angle)
    return jg_gs_set_voltage_rect(h, re.data(), im.data(), stride);
}

int jg_gs_set_voltage_rect(int64_t h, const double* re, const double* im, int64_t stride) {
    GS_ENTER(h);
    if (!re || !im || (stride != 0 && stride != d->n)) return api_fail(1, "jg_gs_set_voltage_rect: bad argument");
    DC_RET(jg::put_lanes(d, d->vr, 0, d->batch, re, stride));
    DC_RET(jg::put_lanes(d, d->vi, 0, d->batch, im, stride));
    return 0;
}

int jg_gs_set_bus_voltage(int64_t h, int64_t bus, const double* magnitude, const double* angle) {
    GS_ENTER(h);
    if (bus < 1 || bus > d->n || !magnitude || !angle) return api_fail(1, "jg_gs_set_bus_voltage: bad argument");
    std::vector<double> re(d->batch), im(d->batch);
    for (int s = 0; s < d->batch; ++s) { re[s] = magnitude[s] * std::cos(angle[s]); im[s] = magnitude[s] * std::sin(angle[s]); }
    const size_t at = (size_t)(bus - 1) * d->ld;
    DC_API_HIP(jg::sync_copy(d->vr + at, re.data(), re.size() * sizeof(double), hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(jg::sync_copy(d->vi + at, im.data(), im.size() * sizeof(double), hipMemcpyHostToDevice, d->stream));
    return 0;
}

int jg_gs_get_voltage(int64_t h, double* magnitude, double* angle, double* re, double* im) {
    GS_ENTER(h);
    if ((magnitude == nullptr) != (angle == nullptr) || (re == nullptr) != (im == nullptr)) return api_fail(1, "jg_gs_get_voltage: magnitude / angle and re / im come in pairs");
    std::vector<double> r, i;
    DC_RET(jg::get_rows(d, d->vr, (size_t)d->n, r));
    DC_RET(jg::get_rows(d, d->vi, (size_t)d->n, i));
    const size_t n = (size_t)d->n, b = (size_t)d->batch;
    for (size_t s = 0; s < b; ++s)
        for (size_t k = 0; k < n; ++k) {
            const double x = r[k * b + s], y = i[k * b + s];
            if (re) { re[s * n + k] = x; im[s * n + k] = y; }
            if (magnitude) { magnitude[s * n + k] = std::hypot(x, y); angle[s * n + k] = std::atan2(y, x); }   // absang
        }
    return 0;
}

int jg_gs_set_outages(int64_t h, int64_t lane0, int64_t count, const int64_t* position, const double* delta) {
    GS_ENTER(h);
    if (lane0 < 0 || count < 1 || lane0 + count > d->batch || !position || !delta) return api_fail(1, "jg_gs_set_outages: bad argument");
    const size_t c = (size_t)count;
    std::vector<int> pos(4 * c);
    std::vector<double> dr(4 * c), di(4 * c);
    for (size_t s = 0; s < c; ++s)
        for (size_t k = 0; k < 4; ++k) {
            const int64_t p = position[4 * s + k];
            if (p < 0 || p > d->nnz) return api_fail(1, "jg_gs_set_outages: position outside the stored pattern");
            pos[k * c + s] = (int)p - 1;
            dr[k * c + s] = p ? delta[2 * (4 * s + k)] : 0.0;
            di[k * c + s] = p ? delta[2 * (4 * s + k) + 1] : 0.0;
        }
    const size_t ld = (size_t)d->ld;
    DC_API_HIP(hipMemcpy2DAsync(d->ppos + lane0, ld * sizeof(int), pos.data(), c * sizeof(int), c * sizeof(int), 4, hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipMemcpy2DAsync(d->pdr + lane0, ld * sizeof(double), dr.data(), c * sizeof(double), c * sizeof(double), 4, hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipMemcpy2DAsync(d->pdi + lane0, ld * sizeof(double), di.data(), c * sizeof(double), c * sizeof(double), 4, hipMemcpyHostToDevice, d->stream));
    DC_API_HIP(hipStreamSynchronize(d->stream));
    return 0;
}

int jg_gs_get_mismatch(int64_t h, double* stop_p, double* stop_q) {
    GS_ENTER(h);
    if (!stop_p || !stop_q) return api_fail(1, "jg_gs_get_mismatch: null pointer");
    DC_API_HIP(jg::sync_copy(stop_p, d->stopP, (size_t)d->batch * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    DC_API_HIP(jg::sync_copy(stop_q, d->stopQ, (size_t)d->batch * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    return 0;
}

int jg_gs_mismatch(int64_t h, double* stop_p, double* stop_q) {
    GS_ENTER(h);
    jg::launch_mismatch(d);
    DC_API_HIP(hipGetLastError());
    return jg_gs_get_mismatch(h, stop_p, stop_q);
}

int jg_gs_solve(int64_t h) {
    GS_ENTER(h);
    jg::launch_sweep(d);
    DC_API_HIP(hipGetLastError());
    DC_API_HIP(hipStreamSynchronize(d->stream));
    return 0;
}

int jg_gs_run(int64_t h, int64_t iteration, double tolerance, int32_t* iterations, int32_t* status) {
    GS_ENTER(h);
    if (iteration < 0 || iteration > INT32_MAX || !iterations || !status) return api_fail(1, "jg_gs_run: bad argument");
    jg::launch_run(d, (int)iteration, tolerance);
    DC_API_HIP(hipGetLastError());
    DC_API_HIP(jg::sync_copy(iterations, d->iteration, (size_t)d->batch * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    DC_API_HIP(jg::sync_copy(status, d->status, (size_t)d->batch * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    return 0;
}

int jg_gs_time_kernel(int64_t h, int kernel, int64_t sweeps, int reps, double* ms) {
    GS_ENTER(h);
    if (kernel < 0 || kernel > 2 || sweeps < 0 || sweeps > INT32_MAX || reps < 1 || !ms) return api_fail(1, "jg_gs_time_kernel: bad argument");
    std::string err;
    const int rc = jg::time_events(d->stream, reps, ms, err, [&]() {
        if (kernel == 0) jg::launch_run(d, (int)sweeps, 0.0);
        else if (kernel == 1) jg::launch_mismatch(d);
        else jg::launch_sweep(d);
        return 0;
    });
    if (rc) return api_fail(rc, err);
    return 0;
}

}  // extern "C"
