// jg_qlim.hip -- reactiveLimit! (acPowerFlow.jl:1081-1155) for every scenario of a batched Newton-Raphson handle, on the device.
//
// Reference behaviour restated (paths relative to the reference tree):
//   reactiveLimit!    src/powerFlow/acPowerFlow.jl:1081-1155   (generator outputs, PV -> PQ with Q at the limit, slack hand-over)
//   generatorPower    src/postprocessing/acAnalysis.jl:538-633 (several generators per bus, infinite limits; restated in power_)
//   setInitialPoint!  src/powerFlow/acPowerFlow.jl:1226-1249   (the start of the newtonRaphson(system) the user builds next)
//   adjustAngle!      src/powerFlow/acPowerFlow.jl:1196-1206
//
// Design: the lane types live in the handle's lane words (2 bits per bus, [ceil(n / 32)][ld], jg_nr.hip: lane_type).  Three launches:
//   1. k_qlim_gen   (generator bus x 64-lane group): the outputs of the bus's generators per lane from the calculated injections of the
//                   mismatch pass ([bus][ld] loads, coalesced), bus.supply of the bus; a PV / slack bus turns PQ with Q at the limit at its first
//                   violating generator (which bus turns PQ does not depend on the order across buses), and records that generator's index.
//   2. k_qlim_walk  (a thread per lane): the order-dependent part of the reference's loop, the slack hand-over -- to the first bus that is PV at
//                   that point of the loop, which may itself turn PQ later in the same loop and hand over again; one ascending pass per lane.
//   3. k_qlim_apply (generator bus x lane): injections supply - demand of the lanes that keep a slack (P only at the bus that was the slack); k_qlim_restart: the lanes with a violation
//                   start again from the container's initial point under their new types; k_qlim_restore: a lane left without a slack gets its
//                   types back (its status becomes 5 on the host side).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "jg_qlim.hpp"

namespace jg {

namespace {

constexpr int NO_CONV = 0x7f7f7f7f;                      // "the bus does not turn PQ" (a byte fill of 0x7f sets it)

__device__ __forceinline__ int lt_get(unsigned long long w, int i) { return (int)((w >> ((i & 31) * 2)) & 3ull); }

struct GenArgs {
    const int* gb_bus; const int* gb_ptr; const int* g_list; const double* g_pg; const double* g_qmin; const double* g_qmax;
    const double* gb_qmins; const double* gb_qmaxs; const double* b_pd; const double* b_qd;
    const double* pq; const unsigned long long* lt_bak; unsigned long long* lt; const int* skip;
    signed char* VO; double* SP; double* SQ; int* conv; int* slack_conv; int* cnt;
    int nbg, ld, batch; double base_mva;
};

// generatorPower (acAnalysis.jl:538-633 as power_ restates it) for the generators of bus gb_bus[blockIdx.x], one lane per thread, and the part of the
// reference's loop (acPowerFlow.jl:1105-1130) that does not depend on the order across buses: a bus that is PV / slack when the call begins turns PQ at
// its FIRST violating generator in label order (a later one finds it PQ) -- the hand-over only turns PV buses into the slack, which is no PQ bus either.
__global__ __launch_bounds__(64) void k_qlim_gen(GenArgs a) {
    const int g = blockIdx.x, grp = blockIdx.y;
    const int b = grp * 64 + threadIdx.x;
    if (g >= a.nbg || b >= a.ld) return;
    const bool real = b < a.batch && !a.skip[b];
    const size_t ld = (size_t)a.ld;
    const int ib = a.gb_bus[g];
    const int k0 = a.gb_ptr[g], k1 = a.gb_ptr[g + 1];
    const double P = a.pq[((size_t)ib * ld + b) * 2], Q = a.pq[((size_t)ib * ld + b) * 2 + 1];
    const int tb = lt_get(a.lt_bak[(size_t)(ib >> 5) * ld + b], ib);
    const bool slack = tb == 3;
    const double pd = a.b_pd[ib], qgen = Q + a.b_qd[ib];
    double sp = 0.0, sq = 0.0, gq_first = 0.0;
    int k_first = -1, v_first = 0;
    if (k1 - k0 == 1) {                                    // one generator: it takes the bus's whole output
        const int k = a.g_list[k0];
        const double gp = slack ? P + pd : a.g_pg[k];
        const double gq = qgen;
        sp += gp; sq += gq;
        const double lo = a.g_qmin[k], hi = a.g_qmax[k];
        const int v = (lo < hi) ? (gq < lo ? -1 : (gq > hi ? 1 : 0)) : 0;
        if (v) { k_first = k; v_first = v; gq_first = gq; }
    } else {
        const double qmins = a.gb_qmins[g], qmaxs = a.gb_qmaxs[g];
        const double big = fabs(qgen) + fabs(qmins) + fabs(qmaxs);
        double qmin_inf = 0.0, qmax_inf = 0.0;
        for (int t = k0; t < k1; ++t) {
            const int j = a.g_list[t];
            const double lo = a.g_qmin[j], hi = a.g_qmax[j];
            if (isinf(lo)) qmin_inf += lo != INFINITY ? -big : big;
            if (isinf(hi)) qmax_inf += hi != -INFINITY ? big : -big;
        }
        const double qmin_sum = qmins + qmin_inf, qmax_sum = qmaxs + qmax_inf;
        const bool prop = a.base_mva * fabs(qmin_sum - qmax_sum) > 10.0 * 2.220446049250313e-16;
        double other_pg = 0.0;                             // the slack's first generator takes what the others do not (sum over idx[1:])
        if (slack) for (int t = k0 + 1; t < k1; ++t) other_pg += a.g_pg[a.g_list[t]];
        for (int t = k0; t < k1; ++t) {
            const int k = a.g_list[t];
            const double lo = a.g_qmin[k], hi = a.g_qmax[k];
            const double qmin_new = isinf(lo) ? (lo != INFINITY ? -big : big) : lo;
            const double qmax_new = isinf(hi) ? (hi != -INFINITY ? big : -big) : hi;
            const double gq = prop ? qmin_new + ((qgen - qmin_sum) / (qmax_sum - qmin_sum)) * (qmax_new - qmin_new)
                                   : qmin_new + (qgen - qmin_sum) / (double)(k1 - k0);
            const double gp = (slack && t == k0) ? P + pd - other_pg : a.g_pg[k];
            sp += gp; sq += gq;
            const int v = (lo < hi) ? (gq < lo ? -1 : (gq > hi ? 1 : 0)) : 0;
            if (v && k_first < 0) { k_first = k; v_first = v; gq_first = gq; }
        }
    }
    int conv = NO_CONV;
    if (real && tb != 1 && k_first >= 0) {                 // :1110-1128: violate, Q pinned at the limit (supply: - old output + new), type PQ
        a.VO[(size_t)k_first * ld + b] = (signed char)v_first;
        sq -= gq_first;
        sq += v_first < 0 ? a.g_qmin[k_first] : a.g_qmax[k_first];
        conv = k_first;
        atomicAdd(&a.cnt[b], 1);
        const int sh = (ib & 31) * 2;                      // other buses of the word belong to other workgroups: two atomics on this bus's field
        atomicAnd(&a.lt[(size_t)(ib >> 5) * ld + b], ~(3ull << sh));
        atomicOr(&a.lt[(size_t)(ib >> 5) * ld + b], 1ull << sh);
        if (slack) a.slack_conv[b] = k_first;              // one slack per lane: one writer
    }
    a.conv[(size_t)g * ld + b] = conv;
    a.SP[(size_t)g * ld + b] = sp;
    a.SQ[(size_t)g * ld + b] = sq;
}

struct WalkArgs {
    const unsigned long long* lt_bak; unsigned long long* lt; const int* conv; const int* slack_conv; const int* b_gbi; const int* skip; int* dead;
    int n, ld, batch;
};

// The slack hand-over of acPowerFlow.jl:1131-1146 per lane: when the slack turns PQ at generator k, the first bus that is PV at that point of the loop
// (PV when the call began, and not turned PQ by a generator before k) becomes the slack; if that bus turns PQ itself later (at generator k' > k), the
// next such bus takes over at k', and so on.  Buses before a chosen one had turned PQ before k already, so ONE ascending pass finds the whole chain.
// Lanes whose slack did not violate (almost all) return at once.
__global__ __launch_bounds__(64) void k_qlim_walk(WalkArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.ld) return;
    const size_t ld = (size_t)a.ld;
    int k = (b < a.batch && !a.skip[b]) ? a.slack_conv[b] : NO_CONV;
    bool has_slack = true;
    if (k != NO_CONV) {
        has_slack = false;
        const int rows = (a.n + 31) / 32;
        for (int r = 0; r < rows && !has_slack; ++r) {
            const unsigned long long x = a.lt_bak[(size_t)r * ld + b];
            unsigned long long pv = (x >> 1) & ~x & 0x5555555555555555ull;      // low bit of every 2-bit field that holds 2 (PV)
            while (pv) {
                const int f = __ffsll((long long)pv) - 1;                         // even: 2 * (bus & 31)
                pv &= pv - 1;
                const int i = r * 32 + f / 2;
                if (i >= a.n) break;
                const int gi = a.b_gbi[i];
                const int c = gi >= 0 ? a.conv[(size_t)gi * ld + b] : NO_CONV;
                if (c <= k) continue;                      // PQ at this point of the loop
                if (c == NO_CONV) {                        // the new slack stays
                    unsigned long long* w = a.lt + (size_t)r * ld + b;
                    *w = (*w & ~(3ull << f)) | (3ull << f);
                    has_slack = true;
                    break;
                }
                k = c;                                     // slack from k on, PQ at c (its type is already 1): the next PV bus takes over at c
            }
        }
    }
    a.dead[b] = has_slack ? 0 : 1;
}

struct ApplyArgs {
    const int* gb_bus; const double* b_pd; const double* b_qd; const double* SP; const double* SQ; const int* skip; const int* dead;
    const unsigned long long* lt_bak; double* p; double* q; int nbg, ld, batch;
};

// Q: bus.supply.reactive - demand at every generator bus (the reference rebuilds the supply from the generator outputs, acPowerFlow.jl:1093-1103).
// P: only where the bus was the slack when the call began -- its generators take the P of the state there (gen.output.active = P_i + pd, :1097); at
// every other bus gen.output.active is what it was, and so is the lane's own P injection (set by the caller, or by an earlier call at a former slack).
// Bus loop strided over gridDim.y (grids of more than 65 535 buses).
__global__ __launch_bounds__(256) void k_qlim_apply(ApplyArgs a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.batch || a.skip[b] || a.dead[b]) return;
    const size_t ld = (size_t)a.ld;
    for (int g = blockIdx.y; g < a.nbg; g += gridDim.y) {
        const int ib = a.gb_bus[g];
        if (lt_get(a.lt_bak[(size_t)(ib >> 5) * ld + b], ib) == 3)
            a.p[(size_t)ib * ld + b] = a.SP[(size_t)g * ld + b] - a.b_pd[ib];   // injection = supply - demand (acPowerFlow.jl:676-680)
        a.q[(size_t)ib * ld + b] = a.SQ[(size_t)g * ld + b] - a.b_qd[ib];
    }
}

// newtonRaphson(system) of the scenarios that had a violation: the start of initializeACPowerFlow under their new types
__global__ __launch_bounds__(256) void k_qlim_restart(const unsigned long long* lt, const double* b_vg, const double* b_vm, const double* b_va, const int* cnt,
                                                      const int* dead, double* vm, double* va, int n, int ld, int batch) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch || cnt[b] == 0 || dead[b]) return;
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const size_t at = (size_t)i * ld + b;
        const int t = lt_get(lt[(size_t)(i >> 5) * ld + b], i);
        vm[at] = t != 1 ? b_vg[i] : b_vm[i];
        va[at] = b_va[i];
    }
}

__global__ __launch_bounds__(256) void k_qlim_restore(const unsigned long long* bak, unsigned long long* lt, const int* dead, int rows, int ld, int batch) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch || !dead[b]) return;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) lt[(size_t)r * ld + b] = bak[(size_t)r * ld + b];
}

__global__ __launch_bounds__(256) void k_angle_shift(const double* va, double* shift, int bus, double angle, int ld, int batch) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    shift[b] = angle - va[(size_t)bus * ld + b];
}

__global__ __launch_bounds__(256) void k_angle_apply(double* va, const double* shift, int n, int ld, int batch) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    const double sh = shift[b];
    for (int i = blockIdx.y; i < n; i += gridDim.y) va[(size_t)i * ld + b] = va[(size_t)i * ld + b] + sh;
}

// rows of a launch whose kernel strides its row loop over gridDim.y (at most 4096 workgroups deep)
unsigned ycap(int rows) { return (unsigned)std::max(1, std::min(rows, 4096)); }

template <class T>
bool up(T** d, const std::vector<T>& h, hipStream_t s) {
    if (hipMalloc((void**)d, std::max<size_t>(h.size(), 1) * sizeof(T)) != hipSuccess) return false;
    if (h.empty()) return true;
    return hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s) == hipSuccess;
}

}  // namespace

void QlimTables::destroy() {
    for (void* p : {(void*)gb_bus, (void*)gb_ptr, (void*)g_list, (void*)g_bus, (void*)g_gbi, (void*)b_gbi, (void*)g_pg, (void*)g_qmin, (void*)g_qmax,
                    (void*)gb_qmins, (void*)gb_qmaxs, (void*)b_vg, (void*)b_vm, (void*)b_va, (void*)b_pd, (void*)b_qd, (void*)conv, (void*)slack_conv,
                    (void*)VO, (void*)SP, (void*)SQ, (void*)cnt, (void*)dead, (void*)lt_bak})
        if (p) hipFree(p);
    *this = QlimTables{};
}

int qlim_setup(QlimTables& t, int n, int ld, int ng, const int64_t* bus, const int8_t* status, const double* pg, const double* qmin, const double* qmax,
               const double* vg, const double* bus_vm, const double* bus_va, const double* pd, const double* qd, double base_mva, hipStream_t s, std::string& msg) {
    t.destroy();
    // per-bus lists of in-service generators in label order (bus.supply.generator) and their finite limit sums
    std::vector<std::vector<int>> at(n);
    for (int k = 0; k < ng; ++k) {
        if (bus[k] < 1 || bus[k] > n) { msg = "jg_nr_set_generators: generator bus out of range"; return 1; }
        if (status[k] == 1) at[bus[k] - 1].push_back(k);
    }
    std::vector<int> gb_bus, gb_ptr{0}, g_list, g_bus(ng), g_gbi(ng, -1), b_gbi(n, -1);
    std::vector<double> qmins, qmaxs, b_vg(bus_vm, bus_vm + n);
    for (int i = 0; i < n; ++i) {
        if (at[i].empty()) continue;
        const int g = (int)gb_bus.size();
        gb_bus.push_back(i);
        b_gbi[i] = g;
        double lo = 0.0, hi = 0.0;                         // sum(qmin[j] for j in idx if not isinf) -- the order of the reference's sums
        for (int k : at[i]) {
            g_list.push_back(k); g_gbi[k] = g;
            if (!std::isinf(qmin[k])) lo += qmin[k];
            if (!std::isinf(qmax[k])) hi += qmax[k];
        }
        gb_ptr.push_back((int)g_list.size());
        qmins.push_back(lo); qmaxs.push_back(hi);
        b_vg[i] = vg[at[i][0]];                            // setInitialPoint!: the first in-service generator's set-point
    }
    for (int k = 0; k < ng; ++k) g_bus[k] = (int)bus[k] - 1;
    t.n = n; t.ng = ng; t.nbg = (int)gb_bus.size(); t.ld = ld; t.base_mva = base_mva;
    const std::vector<double> vpg(pg, pg + ng), vqmin(qmin, qmin + ng), vqmax(qmax, qmax + ng), vvm(bus_vm, bus_vm + n), vva(bus_va, bus_va + n),
        vpd(pd, pd + n), vqd(qd, qd + n);
    const size_t ngl = (size_t)std::max(ng, 1) * ld, nbl = (size_t)std::max(t.nbg, 1) * ld;
    bool ok = up(&t.gb_bus, gb_bus, s) && up(&t.gb_ptr, gb_ptr, s) && up(&t.g_list, g_list, s) && up(&t.g_bus, g_bus, s) && up(&t.g_gbi, g_gbi, s) && up(&t.b_gbi, b_gbi, s) &&
              up(&t.g_pg, vpg, s) && up(&t.g_qmin, vqmin, s) && up(&t.g_qmax, vqmax, s) && up(&t.gb_qmins, qmins, s) && up(&t.gb_qmaxs, qmaxs, s) &&
              up(&t.b_vg, b_vg, s) && up(&t.b_vm, vvm, s) && up(&t.b_va, vva, s) && up(&t.b_pd, vpd, s) && up(&t.b_qd, vqd, s);
    ok = ok && hipMalloc((void**)&t.conv, nbl * 4) == hipSuccess && hipMalloc((void**)&t.slack_conv, (size_t)ld * 4) == hipSuccess && hipMalloc((void**)&t.VO, ngl) == hipSuccess &&
         hipMalloc((void**)&t.SP, nbl * 8) == hipSuccess && hipMalloc((void**)&t.SQ, nbl * 8) == hipSuccess &&
         hipMalloc((void**)&t.cnt, (size_t)ld * 4) == hipSuccess &&
         hipMalloc((void**)&t.dead, (size_t)ld * 4) == hipSuccess && hipMalloc((void**)&t.lt_bak, (size_t)((n + 31) / 32) * ld * 8) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) { t.destroy(); msg = "jg_nr_set_generators: device allocation or upload failed"; return 2; }
    return 0;
}

void qlim_launch(QlimTables& t, const double* pq, unsigned long long* lt, double* p, double* q, double* vm, double* va, const int* skip_dev,
                 int batch, int ld, bool restart, hipStream_t s) {
    const int groups = ld / 64, rows = (t.n + 31) / 32;
    hipMemsetAsync(t.cnt, 0, (size_t)ld * 4, s);
    hipMemsetAsync(t.slack_conv, 0x7f, (size_t)ld * 4, s);                   // NO_CONV: the slack does not turn PQ
    hipMemsetAsync(t.VO, 0, (size_t)std::max(t.ng, 1) * ld, s);
    hipMemcpyAsync(t.lt_bak, lt, (size_t)rows * ld * 8, hipMemcpyDeviceToDevice, s);
    if (t.nbg > 0) {
        GenArgs ga{t.gb_bus, t.gb_ptr, t.g_list, t.g_pg, t.g_qmin, t.g_qmax, t.gb_qmins, t.gb_qmaxs, t.b_pd, t.b_qd, pq, t.lt_bak, lt, skip_dev,
                   t.VO, t.SP, t.SQ, t.conv, t.slack_conv, t.cnt, t.nbg, ld, batch, t.base_mva};
        hipLaunchKernelGGL(k_qlim_gen, dim3((unsigned)t.nbg, (unsigned)groups), dim3(64), 0, s, ga);
    }
    WalkArgs wa{t.lt_bak, lt, t.conv, t.slack_conv, t.b_gbi, skip_dev, t.dead, t.n, ld, batch};
    hipLaunchKernelGGL(k_qlim_walk, dim3((unsigned)groups), dim3(64), 0, s, wa);
    const unsigned bx = (unsigned)((batch + 255) / 256);
    if (t.nbg > 0) {
        ApplyArgs aa{t.gb_bus, t.b_pd, t.b_qd, t.SP, t.SQ, skip_dev, t.dead, t.lt_bak, p, q, t.nbg, ld, batch};
        hipLaunchKernelGGL(k_qlim_apply, dim3(bx, ycap(t.nbg)), dim3(256), 0, s, aa);
    }
    hipLaunchKernelGGL(k_qlim_restore, dim3(bx, ycap(rows)), dim3(256), 0, s, (const unsigned long long*)t.lt_bak, lt, (const int*)t.dead, rows, ld, batch);
    if (restart)
        hipLaunchKernelGGL(k_qlim_restart, dim3(bx, ycap(t.n)), dim3(256), 0, s, (const unsigned long long*)lt, (const double*)t.b_vg, (const double*)t.b_vm,
                           (const double*)t.b_va, (const int*)t.cnt, (const int*)t.dead, vm, va, t.n, ld, batch);
}

void adjust_angle_launch(double* shift, double* va, int n, int ld, int batch, int bus, double angle, hipStream_t s) {
    const unsigned bx = (unsigned)((batch + 255) / 256);
    hipLaunchKernelGGL(k_angle_shift, dim3(bx), dim3(256), 0, s, (const double*)va, shift, bus, angle, ld, batch);
    hipLaunchKernelGGL(k_angle_apply, dim3(bx, ycap(n)), dim3(256), 0, s, va, (const double*)shift, n, ld, batch);
}

}  // namespace jg
