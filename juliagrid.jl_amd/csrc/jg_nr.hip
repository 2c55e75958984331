// jg_nr.hip -- Newton-Raphson AC power flow on MI355X: C ABI (include/jgrid.h) + fused
// mismatch/Jacobian assembly kernel + per-scenario convergence control.
//
// Reference behaviour restated (paths relative to /root/reference):
//   newtonJacobian      src/powerFlow/acPowerFlow.jl:89-175   (index maps, CSC pattern; bit-exact)
//   mismatch!           src/powerFlow/acPowerFlow.jl:645-685  + src/backend/equations.jl:63-103,126-128
//   solve! (fill)       src/powerFlow/acPowerFlow.jl:820-888  + src/backend/equations.jl:105-144
//   solve! (linear)     src/powerFlow/acPowerFlow.jl:890-906  -> jg_engine (device LU / solves / update)
//   powerFlow!          src/powerFlow/acPowerFlow.jl:1389-1433
//
// Design (not a translation): the reference walks Ybus three times per iteration with one sincos
// each (mismatch, off-diagonal partials, diagonal re-sum).  Here ONE pass over bus row i with one
// sincos per stored (i,j) produces f_P, f_Q and the whole 2x2-block Jacobian row; PV / slack rows
// and columns are padded with identity so the Jacobian is an n x n matrix of 2x2 blocks with the
// Ybus pattern -- the layout the block LU engine consumes directly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/jgrid.h"
#include "jg_engine.hpp"
#include "jg_pf.hpp"
#include "jg_comp.hpp"
#include "jg_compact.hpp"
#include "jg_lanes.hpp"
#include "jg_qlim.hpp"

namespace {

thread_local std::string g_error;

int fail(int code, const std::string& msg) { return jg::api_fail(code, msg); }
#define NR_HIP JG_API_HIP
using jg::uniform;
namespace pf = jg::pf;             // the equations of the kernels below

constexpr int ASM_ROWS = 16;   // bus rows per workgroup
constexpr int ASM_WAVES = 4;
constexpr int CH = 4;          // Ybus entries whose gathers are in flight together

struct AsmArgs {
    const int* rowptr; const int* colm; const double2* GB; const int* rowtype;   // colm = col | (mask << 24); rowtype: int per bus (scalar-loadable)
    const int* dst;            // Ybus CSR position -> entry of the LU factor storage: the Jacobian is assembled IN PLACE
    const double* vm; const double* va; const double* p; const double* q;
    const int* ppos; const double* pdg; const double* pdb;
    double* A; double* F; double* part; double* pq_out; jg::GroupSel sel;   // pq_out (nullable): [n][ld][2] calculated injections P_i, Q_i
    double* R; int fd_mode;    // fast decoupled passes (acPowerFlow.jl:687-730, 952-962): 1 = mismatches / V, R = (f_P, 0); 2 = R = (0, f_Q)
    int n; int ld; int mp; int nchunk; int lanes;
    const int* only_if;        // nullable: the launch does nothing unless *only_if != 0 (re-assembly after a lane compaction)
    double* W; int* lu_status; // (lu_status: unused by the kernel -- an atomic there costs 14 VGPRs and a wave per SIMD; a singular level-0 block
                               // turns the row's mismatch into NaN instead, which k_check reports as status 3)
                               // level 0 of the engine's prefactor plan (jg_symbolic.hpp): where rowtype carries (pivot + 1) << 2 the diagonal block
                               // leaves FACTORISED and the mismatch row is also written as the rhs row W[pivot]
    const unsigned long long* lt;   // per-lane bus types (k_assemble<.., LT = true>): [ceil(n / 32)][ld], 2 bits per bus (jg_nr_set_bus_type)
};

// The type of bus i in the lane whose word of row i / 32 is w (2 bits per bus: 1 PQ, 2 PV, 3 slack)
__device__ __forceinline__ int lane_type(unsigned long long w, int i) { return (int)((w >> ((i & 31) * 2)) & 3ull); }

__device__ __forceinline__ void store_vec_nt(double* base, size_t item, size_t b, size_t ld, double v0, double v1) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store(d2{v0, v1}, (d2*)(base + (item * ld + b) * 2));
}

// Fused mismatch + Jacobian assembly. blockDim (64, ASM_WAVES); 1-D grid, scenario group fastest (jg::map_block:
// a group's V/theta gathers stay in one XCD's L2).
// JAC = false: mismatch only (no Jacobian stores) -- the cheap pre-pass that decides which scenarios are still active.
// WAVES: waves of a workgroup (which always takes ASM_ROWS bus rows).  4: a wave walks four rows one after the other -- the throughput form; 16 (round 6, a handful of
// scenarios): one row per wave -- a row is three dependent round trips (row header, Ybus entries, V / theta gathers), and with nothing else on the chip to hide them
// four rows in sequence made the pass of a single instance 23 us long.
// LT = true: the bus types come from the lanes (a.lt) instead of rowtype / the host's existence bits -- a batch whose scenarios have types of their own
// (PV -> PQ after reactive limits, a slack handed over); the 4 existence bits of each entry follow from the lane's types of row i and column j with
// the host's rule (jg_nr_create), the pattern and the plan stay those of the handle.
template <int MP, bool JAC, int WAVES = ASM_WAVES, bool LT = false>
__global__ __launch_bounds__(64 * WAVES) void k_assemble(AsmArgs a) {
    __shared__ double red[2][WAVES][64];
    int grp, bx;
    if (a.only_if && !uniform(*a.only_if)) return;
    if (!jg::map_block(a.sel, a.ld, a.nchunk, grp, bx)) return;   // every scenario of a skipped 64-lane group is finished
    const int lane = threadIdx.x;
    const int wave = uniform(threadIdx.y);
    const size_t ld = (size_t)a.ld;
    const size_t b = (size_t)min(grp * 64 + lane, a.lanes - 1);        // lanes beyond the batch alias its last scenario
    int ppos[MP > 0 ? MP : 1];
#pragma unroll
    for (int m = 0; m < MP; ++m) ppos[m] = a.ppos[(size_t)m * ld + b];
    double maxp = 0.0, maxq = 0.0;
    const int r0 = bx * ASM_ROWS;
    const int r1 = min(r0 + ASM_ROWS, a.n);
    for (int i = r0 + wave; i < r1; i += WAVES) {
        const int p0 = uniform(a.rowptr[i]), p1 = uniform(a.rowptr[i + 1]);
        const int tfull = (int)((unsigned)uniform(a.rowtype[i]));   // bus type | (pivot + 1) << 2 where this pass also finishes the plan's level 0
        int ti = tfull & 3;
        const int pre = tfull >> 2;
        if constexpr (LT) ti = lane_type(a.lt[(size_t)(i >> 5) * ld + b], i);
        const double vi = a.vm[(size_t)i * ld + b];
        const double thi = a.va[(size_t)i * ld + b];
        const double pinj = a.p[(size_t)i * ld + b], qinj = a.q[(size_t)i * ld + b];   // issued early, used after the row
        double s1 = 0.0, s2 = 0.0, gii = 0.0, bii = 0.0;
        int pd = 0;                                        // factor entry of the diagonal block
        // rows are short (3.4 entries on average, <= 19): the cost is the latency of the V/theta gathers,
        // so the loads of four entries are issued together before any of them is consumed
        for (int pc = p0; pc < p1; pc += CH) {
            const int cnt = min(CH, p1 - pc);
            int cm[CH], de[CH]; double2 gb[CH]; double vv[CH], tt[CH];
            unsigned long long lw[LT ? CH : 1];
#pragma unroll
            for (int k = 0; k < CH; ++k) {                       // scalar loads of the whole chunk first ...
                const int p = pc + (k < cnt ? k : 0);
                cm[k] = uniform(a.colm[p]);
                de[k] = JAC ? uniform(a.dst[p]) : 0;
                gb[k] = a.GB[p];
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {                       // ... then all gathers in flight together
                const size_t j = (size_t)(cm[k] & 0xffffff);
                vv[k] = a.vm[j * ld + b];
                tt[k] = a.va[j * ld + b];
                if constexpr (LT) lw[k] = a.lt[(j >> 5) * ld + b];
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                if (k >= cnt) break;
                const int p = pc + k;
                const int j = cm[k] & 0xffffff;
                int mk = cm[k] >> 24;                          // the existence bits of the entry (pf::offdiag)
                if constexpr (LT) {                            // the host's rule (jg_nr_create) on the lane's types
                    const int tj = lane_type(lw[k], j);
                    const int rpm = ti != 3, rq = ti == 1, ct = tj != 3, cv = tj == 1;
                    mk = (rpm & ct) | ((rpm & cv) << 1) | ((rq & ct) << 2) | ((rq & cv) << 3);
                }
                double g = gb[k].x, bb = gb[k].y;
                pf::patched<MP>(p, ppos, a.pdg, a.pdb, ld, b, g, bb);
                const double vj = vv[k];
                double s, c;
                sincos(thi - tt[k], &s, &c);
                const pf::Terms t = pf::entry_terms(g, bb, s, c);
                s1 += vj * t.ac; s2 += vj * t.ad;
                if (j == i) { pd = de[k]; gii = g; bii = bb; continue; }
                if (!JAC) continue;
                // write-once stream (read back by the factorisation only): nontemporal, so the V/theta gathers keep the L2
                const jg::Blk o = pf::offdiag(mk, vi, vj, t.ac, t.ad);
                jg::store_blk_nt(a.A, (size_t)de[k], b, ld, o.v00, o.v01, o.v10, o.v11);
            }
        }
        if (!JAC && a.pq_out) jg::store_vec(a.pq_out, (size_t)i, b, ld, vi * s1, vi * s2);     // PiQi (acAnalysis.jl:891-896)
        pf::Row r = pf::row_closure(vi, s1, s2, gii, bii, pinj, qinj);
        if (!JAC && a.fd_mode) {                           // fast Newton-Raphson: calc - spec / V  (acPowerFlow.jl:720-726, 952-961)
            const double vinv = 1.0 / vi;
            r.fp = s1 - pinj * vinv; r.fq = s2 - qinj * vinv;
        }
        r = pf::pad(ti, 1.0, r);
        if (JAC) {
            if (pre) {                                     // nobody updates this block: its 2x2 LU is the factorisation's whole work on it
                bool bad;
                r.d = jg::diag_lu(r.d, jg::row_max(r.d), bad);
                if (bad) r.fp = __builtin_nan("");         // a singular block marks its scenario through the mismatch (k_check: NaN -> status 3)
                store_vec_nt(a.W, (size_t)pre - 1, b, ld, r.fp, r.fq);   // nontemporal like every other store of this pass: a plain store here
                                                                           // cost 0.09 ms per pass at 512 scenarios (the V / theta gathers lost their L2 lines)
            }
            jg::store_blk_nt(a.A, (size_t)pd, b, ld, r.d.v00, r.d.v01, r.d.v10, r.d.v11);
        }
        if (!JAC && a.fd_mode) {
            if (a.fd_mode == 1) { jg::store_vec(a.F, (size_t)i, b, ld, r.fp, r.fq); jg::store_vec(a.R, (size_t)i, b, ld, r.fp, 0.0); }
            else jg::store_vec(a.R, (size_t)i, b, ld, 0.0, r.fq);
        } else {
            store_vec_nt(a.F, (size_t)i, b, ld, r.fp, r.fq);
        }
        maxp = pf::nanmax(fabs(r.fp), maxp); maxq = pf::nanmax(fabs(r.fq), maxq);
    }
    red[0][wave][lane] = maxp;
    red[1][wave][lane] = maxq;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            maxp = pf::nanmax(red[0][w][lane], maxp); maxq = pf::nanmax(red[1][w][lane], maxq);
        }
        a.part[((size_t)bx * 2) * ld + b] = maxp;
        a.part[((size_t)bx * 2 + 1) * ld + b] = maxq;
    }
}

// The assembly of ONE scenario (round 6): a QUAD of lanes per bus row.  k_assemble gives a wave to a row of 64 scenarios and walks four rows one after the other; with one
// scenario that is four times three dependent round trips per wave (row header, Ybus entries, V / theta gathers) around the work of one lane.  Here lane q of a row's quad
// takes its Ybus entries q, q + 4, ... two at a time (a row of 19 entries is three trips instead of five, and a trip is two sincos per lane instead of four), the row sums
// meet through two shuffles (fixed order), lane 0 finishes the row as k_assemble does (the leaf pivots of a prefactor plan leave factorised, the rhs row with them); the
// chunk maxima of sixteen rows meet through shuffles as well.  Same formulas per entry; the row sums add in another order (V, theta within 1e-10: tests/test_top_variants_gpu.py).
template <int MP, bool JAC>
__global__ __launch_bounds__(256) void k_assemble1(AsmArgs a) {
    int grp, bx;
    if (!jg::map_block(a.sel, a.ld, (a.n + 63) / 64, grp, bx)) return;
    const size_t ld = (size_t)a.ld;
    const size_t b = (size_t)grp * 64;
    const int q = (int)threadIdx.x & 3;
    const int i0 = bx * 64 + ((int)threadIdx.x >> 2);
    const bool live = i0 < a.n;
    const int i = live ? i0 : a.n - 1;
    int ppos[MP > 0 ? MP : 1];
#pragma unroll
    for (int m = 0; m < MP; ++m) ppos[m] = a.ppos[(size_t)m * ld + b];
    const int p0 = a.rowptr[i], p1 = live ? a.rowptr[i + 1] : p0;
    const int tfull = (int)((unsigned)a.rowtype[i]);
    const int ti = tfull & 3, pre = tfull >> 2;
    const double vi = a.vm[(size_t)i * ld + b];
    const double thi = a.va[(size_t)i * ld + b];
    const double pinj = a.p[(size_t)i * ld + b], qinj = a.q[(size_t)i * ld + b];
    double s1 = 0.0, s2 = 0.0, gii = 0.0, bii = 0.0;
    int pd = 0;
    constexpr int C2 = 2;                                         // entries per lane and trip
    for (int pc = p0 + q; pc < p1; pc += 4 * C2) {               // this lane's entries: pc, pc + 4
        int cm[C2], de[C2]; double2 gb[C2]; double vv[C2], tt[C2];
#pragma unroll
        for (int k = 0; k < C2; ++k) {
            const int p = pc + 4 * k < p1 ? pc + 4 * k : pc;
            cm[k] = a.colm[p];
            de[k] = JAC ? a.dst[p] : 0;
            gb[k] = a.GB[p];
        }
#pragma unroll
        for (int k = 0; k < C2; ++k) {
            const size_t j = (size_t)(cm[k] & 0xffffff);
            vv[k] = a.vm[j * ld + b];
            tt[k] = a.va[j * ld + b];
        }
#pragma unroll
        for (int k = 0; k < C2; ++k) {
            const int p = pc + 4 * k;
            if (p < p1) {
                const int j = cm[k] & 0xffffff;
                const int mk = cm[k] >> 24;
                double g = gb[k].x, bb = gb[k].y;
                pf::patched<MP>(p, ppos, a.pdg, a.pdb, ld, b, g, bb);
                const double vj = vv[k];
                double s, c;
                sincos(thi - tt[k], &s, &c);
                const pf::Terms t = pf::entry_terms(g, bb, s, c);
                s1 += vj * t.ac; s2 += vj * t.ad;
                if (j == i) { pd = de[k]; gii = g; bii = bb; }
                else if (JAC) {
                    const jg::Blk o = pf::offdiag(mk, vi, vj, t.ac, t.ad);
                    jg::store_blk(a.A, (size_t)de[k], b, ld, o.v00, o.v01, o.v10, o.v11);
                }
            }
        }
    }
    // the quad's sums; the diagonal entry sat on exactly one lane (the others hold zeros)
#pragma unroll
    for (int d = 1; d <= 2; d <<= 1) {
        s1 += __shfl_xor(s1, d); s2 += __shfl_xor(s2, d);
        gii += __shfl_xor(gii, d); bii += __shfl_xor(bii, d); pd += __shfl_xor(pd, d);
    }
    pf::Row r = pf::pad(ti, 1.0, pf::row_closure(vi, s1, s2, gii, bii, pinj, qinj));
    if (JAC && pre) {
        bool bad;
        r.d = jg::diag_lu(r.d, jg::row_max(r.d), bad);
        if (bad) r.fp = __builtin_nan("");
    }
    if (live && q == 0) {
        if (JAC) {
            if (pre) jg::store_vec(a.W, (size_t)pre - 1, b, ld, r.fp, r.fq);
            jg::store_blk(a.A, (size_t)pd, b, ld, r.d.v00, r.d.v01, r.d.v10, r.d.v11);
        }
        jg::store_vec(a.F, (size_t)i, b, ld, r.fp, r.fq);
    }
    // chunk maxima: ASM_ROWS consecutive rows = 4 ASM_ROWS consecutive lanes = one wave (NaN-propagating: a NaN mismatch must not look converged)
    static_assert(ASM_ROWS == 16, "a chunk of rows is one wave of quads");
    double maxp = live ? fabs(r.fp) : 0.0, maxq = live ? fabs(r.fq) : 0.0;
    for (int d = 4; d < 64; d <<= 1) {
        const double x = __shfl_xor(maxp, d), y = __shfl_xor(maxq, d);
        maxp = pf::nanmax(x, maxp); maxq = pf::nanmax(y, maxq);
    }
    if (live && ((int)threadIdx.x & 63) == 0) {
        const size_t ck = (size_t)(i0 / ASM_ROWS);
        a.part[(ck * 2) * ld + b] = maxp;
        a.part[(ck * 2 + 1) * ld + b] = maxq;
    }
}

// ---- iterative refinement of the Newton step (opt-in, jg_nr_set_refine) ------------------------------------------------
// The reference's default solver refines: UMFPACK's solve runs up to two steps of iterative refinement behind `ldiv!`
// (/root/reference/src/backend/utility.jl:576-586 -> umfpack_solve, UMFPACK_IRSTEP = 2), which is what covers a weak pivot
// of ITS threshold pivoting.  The device keeps a static pivot order, so the same guard is offered here: after the first solve
//   rho = f - J d         (this kernel: J is NOT stored -- the factor overwrote it -- so the product is formed from Ybus
//                          and the unchanged state with the same sincos terms the assembly uses, one pass over the rows)
//   d  += J^-1 rho        (forward-only sweep + backward sweep on the factor that is already there), then x -= d.
struct RefineArgs {
    const int* rowptr; const int* colm; const double2* GB; const int* rowtype;
    const double* vm; const double* va;
    const int* ppos; const double* pdg; const double* pdb;
    const double* F; const double* inc; double* R; jg::GroupSel sel;
    int n; int ld; int mp; int nchunk; int lanes;
};

template <int MP>
__global__ __launch_bounds__(64 * ASM_WAVES) void k_refine_residual(RefineArgs a) {
    int grp, bx;
    if (!jg::map_block(a.sel, a.ld, a.nchunk, grp, bx)) return;
    const int lane = threadIdx.x;
    const int wave = uniform(threadIdx.y);
    const size_t ld = (size_t)a.ld;
    const size_t b = (size_t)min(grp * 64 + lane, a.lanes - 1);
    int ppos[MP > 0 ? MP : 1];
#pragma unroll
    for (int m = 0; m < MP; ++m) ppos[m] = a.ppos[(size_t)m * ld + b];
    const int r0 = bx * ASM_ROWS, r1 = min(r0 + ASM_ROWS, a.n);
    for (int i = r0 + wave; i < r1; i += ASM_WAVES) {
        const int p0 = uniform(a.rowptr[i]), p1 = uniform(a.rowptr[i + 1]);
        const int ti = (int)((unsigned)uniform(a.rowtype[i]));
        const double vi = a.vm[(size_t)i * ld + b], thi = a.va[(size_t)i * ld + b];
        const double2 f = jg::load_vec(a.F, (size_t)i, b, ld);
        const double2 di = jg::load_vec(a.inc, (size_t)i, b, ld);
        double s1 = 0.0, s2 = 0.0, gii = 0.0, bii = 0.0, rp = f.x, rq = f.y;
        for (int p = p0; p < p1; ++p) {
            const int cm = uniform(a.colm[p]);
            const int j = cm & 0xffffff, mk = cm >> 24;
            double2 gb = a.GB[p];
            pf::patched<MP>(p, ppos, a.pdg, a.pdb, ld, b, gb.x, gb.y);
            const double vj = a.vm[(size_t)j * ld + b];
            double s, c;
            sincos(thi - a.va[(size_t)j * ld + b], &s, &c);
            const pf::Terms t = pf::entry_terms(gb.x, gb.y, s, c);
            s1 += vj * t.ac; s2 += vj * t.ad;
            if (j == i) { gii = gb.x; bii = gb.y; continue; }
            const double2 dj = jg::load_vec(a.inc, (size_t)j, b, ld);
            const jg::Blk o = pf::offdiag(mk, vi, vj, t.ac, t.ad);
            rp -= o.v00 * dj.x + o.v01 * dj.y;
            rq -= o.v10 * dj.x + o.v11 * dj.y;
        }
        const pf::Row r = pf::pad(ti, 1.0, pf::row_closure(vi, s1, s2, gii, bii, 0.0, 0.0));     // the block alone: the mismatch came in as F
        rp -= r.d.v00 * di.x + r.d.v01 * di.y;
        rq -= r.d.v10 * di.x + r.d.v11 * di.y;
        jg::store_vec(a.R, (size_t)i, b, ld, rp, rq);
    }
}

// d = d1 + d2 (kept as method.increment), then x -= d on the state components of the scenarios still iterating
__global__ void k_refine_apply(double* inc, const double* inc1, const double* inc2, double* va, double* vm, const signed char* flags, const int* active,
                               const jg::GroupSel sel, int n, int ld, int lanes) {
    int grp, bx;
    if (!jg::map_block(sel, ld, (n + 15) / 16, grp, bx)) return;
    const int i = bx * 16 + threadIdx.y;
    if (i >= n) return;
    const int lb = grp * 64 + threadIdx.x;
    if (lb >= lanes) return;
    const size_t b = (size_t)lb, l = (size_t)ld;
    if (active && !active[b]) return;
    const double2 d1 = jg::load_vec(inc1, (size_t)i, b, l), d2 = jg::load_vec(inc2, (size_t)i, b, l);
    const double dx = d1.x + d2.x, dy = d1.y + d2.y;
    jg::store_vec(inc, (size_t)i, b, l, dx, dy);
    const int fl = flags[i];
    if (fl & 1) va[(size_t)i * l + b] -= dx;
    if (fl & 2) vm[(size_t)i * l + b] -= dy;
}

// ---- post-processing: power!/current! branch quantities (acAnalysis.jl:66-81, 688-701) -------------------------
struct BranchArgs {
    const int* from; const int* to; const signed char* status; const double* param;   // param [nb][16], see jgrid.h
    const double* vm; const double* va; const int* outage;                              // outage [ld]: 1-based branch out in that scenario
    double* from_pq; double* to_pq; double* series_pq; double* charging_pq; double* from_i; double* to_i; double* series_i;
    int nb; int ld; int lanes;
};

// one wave per branch x 64 scenarios, 16 branches per workgroup; the branch table travels through the scalar cache
__global__ __launch_bounds__(1024) void k_branch_quantities(BranchArgs a) {
    typedef const double __attribute__((address_space(4)))* CDbl;
    typedef const int __attribute__((address_space(4)))* CInt;
    const int lane = threadIdx.x;
    const int k = blockIdx.x * 16 + uniform(threadIdx.y);
    if (k >= a.nb) return;
    const size_t ld = (size_t)a.ld;
    const size_t b = (size_t)min((int)blockIdx.y * 64 + lane, a.lanes - 1);
    CDbl p = (CDbl)a.param + (size_t)k * 16;
    const int i = ((CInt)a.from)[k], j = ((CInt)a.to)[k];
    const bool on = a.status[k] == 1 && a.outage[b] != k + 1;
    const double Vi = a.vm[(size_t)i * ld + b], Vj = a.vm[(size_t)j * ld + b];
    double si, ci, sj, cj;
    sincos(a.va[(size_t)i * ld + b], &si, &ci);
    sincos(a.va[(size_t)j * ld + b], &sj, &cj);
    const pf::BranchEnds e = pf::branch_ends(pf::TwoPort{{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]}}, Vi, Vj, si, ci, sj, cj);
    // Vij = tij Vi - Vj (:846-851), Is = y Vij (:929-931)
    const double wr = p[10] * e.vir - p[11] * e.vii - e.vjr, wi = p[10] * e.vii + p[11] * e.vir - e.vji;
    const double isr = p[8] * wr - p[9] * wi, isi = p[8] * wi + p[9] * wr;
    const double z = on ? 1.0 : 0.0;                                         // out of service: zeros, like initialize! (:66, :688)
    if (a.from_pq) jg::store_vec(a.from_pq, (size_t)k, b, ld, z * e.pf, z * e.qf);                                            // Vi conj(Iij)
    if (a.to_pq) jg::store_vec(a.to_pq, (size_t)k, b, ld, z * e.pt, z * e.qt);                                                // Vj conj(Iji)
    if (a.series_pq) jg::store_vec(a.series_pq, (size_t)k, b, ld, z * (wr * isr + wi * isi), z * (wi * isr - wr * isi));      // Vij conj(y Vij)
    if (a.charging_pq) {                                                     // 0.5 conj(g + jb) ((Vi/tau)^2 + Vj^2)  (:910-919)
        const double m = 0.5 * ((p[14] * Vi) * (p[14] * Vi) + Vj * Vj);
        jg::store_vec(a.charging_pq, (size_t)k, b, ld, z * p[12] * m, -z * p[13] * m);
    }
    if (a.from_i) jg::store_vec(a.from_i, (size_t)k, b, ld, z * hypot(e.ifr, e.ifi), on ? atan2(e.ifi, e.ifr) : 0.0);
    if (a.to_i) jg::store_vec(a.to_i, (size_t)k, b, ld, z * hypot(e.itr, e.iti), on ? atan2(e.iti, e.itr) : 0.0);
    if (a.series_i) jg::store_vec(a.series_i, (size_t)k, b, ld, z * hypot(isr, isi), on ? atan2(isi, isr) : 0.0);
}

// ---- contingency screen summary (SURVEY 8f "next"; jgrid.h: jg_nr_screen): worst branch loading, largest flow, lowest / highest voltage per scenario
// Partial maxima per (chunk of 256 branches resp. 1024 buses, scenario), then one reduction per scenario.  Ties go to the lowest index (fixed order).
struct ScreenArgs {
    const int* from; const int* to; const signed char* status; const double* param; const double* rating;   // rating [nb] or null
    const double* vm; const double* va; const int* outage;
    double* part;                  // [chunks][4][ld]: branch chunks {loading, its branch, flow, its branch}, then bus chunks {vmin, its bus, vmax, its bus}
    const int* iters; const int* status_sc;
    double* rec;                   // [batch][10]
    int nb, n, ld, lanes, bchunks, vchunks;
};
constexpr int SCREEN_BR = 256, SCREEN_BUS = 1024;

__global__ __launch_bounds__(1024) void k_screen_partial(ScreenArgs a) {
    typedef const double __attribute__((address_space(4)))* CDbl;
    typedef const int __attribute__((address_space(4)))* CInt;
    __shared__ double red[16][4][64];
    const int lane = threadIdx.x, wave = uniform(threadIdx.y);
    const size_t ld = (size_t)a.ld;
    const size_t b = (size_t)min((int)blockIdx.y * 64 + lane, a.lanes - 1);
    const int c = blockIdx.x;
    double m0, i0, m1, i1;
    if (c < a.bchunks) {                                         // branches: apparent power at both ends (PijQij, PjiQji: acAnalysis.jl:898-904)
        m0 = 0.0; i0 = 0.0; m1 = 0.0; i1 = 0.0;
        const int k0 = c * SCREEN_BR + wave * (SCREEN_BR / 16);
        for (int k = k0; k < min(k0 + SCREEN_BR / 16, a.nb); ++k) {
            if (a.status[k] != 1) continue;
            CDbl p = (CDbl)a.param + (size_t)k * 16;
            const int i = ((CInt)a.from)[k], j = ((CInt)a.to)[k];
            const bool on = a.outage[b] != k + 1;
            const double Vi = a.vm[(size_t)i * ld + b], Vj = a.vm[(size_t)j * ld + b];
            double si, ci, sj, cj;
            sincos(a.va[(size_t)i * ld + b], &si, &ci);
            sincos(a.va[(size_t)j * ld + b], &sj, &cj);
            const pf::BranchEnds e = pf::branch_ends(pf::TwoPort{{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]}}, Vi, Vj, si, ci, sj, cj);
            const double sf = hypot(e.pf, e.qf), st = hypot(e.pt, e.qt);
            const double s = on ? fmax(sf, st) : 0.0;
            if (s > m1) { m1 = s; i1 = (double)(k + 1); }
            const double r = a.rating ? ((CDbl)a.rating)[k] : 0.0;
            if (r > 0.0 && s / r > m0) { m0 = s / r; i0 = (double)(k + 1); }
        }
    } else {                                                     // buses: lowest and highest voltage magnitude
        m0 = 1.0e300; i0 = 0.0; m1 = -1.0e300; i1 = 0.0;
        const int v0 = (c - a.bchunks) * SCREEN_BUS + wave * (SCREEN_BUS / 16);
        for (int i = v0; i < min(v0 + SCREEN_BUS / 16, a.n); ++i) {
            const double v = a.vm[(size_t)i * ld + b];
            if (v < m0) { m0 = v; i0 = (double)(i + 1); }
            if (v > m1) { m1 = v; i1 = (double)(i + 1); }
        }
    }
    red[wave][0][lane] = m0; red[wave][1][lane] = i0; red[wave][2][lane] = m1; red[wave][3][lane] = i1;
    __syncthreads();
    if (wave != 0) return;
    const bool lo = c >= a.bchunks;                              // the first pair of a bus chunk is a MINIMUM
    for (int w = 1; w < 16; ++w) {                               // ascending index order: a strict comparison keeps the lowest index on ties
        const double x0 = red[w][0][lane], x1 = red[w][2][lane];
        if (lo ? x0 < m0 : x0 > m0) { m0 = x0; i0 = red[w][1][lane]; }
        if (x1 > m1) { m1 = x1; i1 = red[w][3][lane]; }
    }
    double* q = a.part + (size_t)c * 4 * ld + b;
    q[0] = m0; q[ld] = i0; q[2 * ld] = m1; q[3 * ld] = i1;
}

__global__ __launch_bounds__(64) void k_screen_final(ScreenArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.lanes) return;
    const size_t ld = (size_t)a.ld;
    double load = 0.0, lidx = 0.0, flow = 0.0, fidx = 0.0, vmin = 1.0e300, vminidx = 0.0, vmax = -1.0e300, vmaxidx = 0.0;
    for (int c = 0; c < a.bchunks; ++c) {
        const double* q = a.part + (size_t)c * 4 * ld + b;
        if (q[0] > load) { load = q[0]; lidx = q[ld]; }
        if (q[2 * ld] > flow) { flow = q[2 * ld]; fidx = q[3 * ld]; }
    }
    for (int c = a.bchunks; c < a.bchunks + a.vchunks; ++c) {
        const double* q = a.part + (size_t)c * 4 * ld + b;
        if (q[0] < vmin) { vmin = q[0]; vminidx = q[ld]; }
        if (q[2 * ld] > vmax) { vmax = q[2 * ld]; vmaxidx = q[3 * ld]; }
    }
    double* r = a.rec + (size_t)b * 10;
    const int st = a.status_sc[b];
    if (st == 3) {                                               //  numeric failure: V is NaN, every comparison above was false -- the sentinels would read
        const double nan = __builtin_nan("");                     // as "nothing overloaded".  The summary of such a scenario is NaN (jgrid.h); rec[8], rec[9] say why.
        load = flow = vmin = vmax = nan; lidx = fidx = vminidx = vmaxidx = 0.0;
    }
    r[0] = load; r[1] = lidx; r[2] = flow; r[3] = fidx; r[4] = vmin; r[5] = vminidx; r[6] = vmax; r[7] = vmaxidx;
    r[8] = (double)a.iters[b]; r[9] = (double)st;
}

struct CheckArgs {
    const double* part; int nchunk; int ld; int batch;
    const double* params;      // [0] tolerance, [1] max iterations
    double* normp; double* normq; int* active; int* iters; int* status; const int* lu_status; int* counter; const int* group;
    int mode;                  // 0 = norms only, 1 = powerFlow! loop control
};

// blockDim (64, 16): one workgroup per 64-scenario group; the 16 waves split the per-chunk partial norms
__global__ __launch_bounds__(1024) void k_check(CheckArgs a) {
    __shared__ double red[2][16][64];
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int b = blockIdx.x * 64 + lane;
    if (a.mode == 1 && a.group && !a.group[blockIdx.x]) return;   // finished group: assembly was skipped, keep its verdict
    double mp = 0.0, mq = 0.0;
    constexpr int CU = 8;
    for (int c0 = wave; c0 < a.nchunk; c0 += 16 * CU) {           // eight chunks per trip: sixteen loads in flight (625 chunks on a 10 000-bus
        double x[CU], y[CU];                                      // grid were 39 dependent round trips per wave, 26 us per verdict)
#pragma unroll
        for (int u = 0; u < CU; ++u) {
            const int c = min(c0 + 16 * u, a.nchunk - 1);         // a repeated chunk changes no maximum
            x[u] = a.part[((size_t)c * 2) * a.ld + b]; y[u] = a.part[((size_t)c * 2 + 1) * a.ld + b];
        }
#pragma unroll
        for (int u = 0; u < CU; ++u) {
            mp = pf::nanmax(x[u], mp); mq = pf::nanmax(y[u], mq);
        }
    }
    red[0][wave][lane] = mp;
    red[1][wave][lane] = mq;
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 16; ++w) {
        mp = pf::nanmax(red[0][w][lane], mp); mq = pf::nanmax(red[1][w][lane], mq);
    }
    a.normp[b] = mp;
    a.normq[b] = mq;
    if (a.mode == 0) return;
    const double tol = a.params[0];
    const int maxit = (int)a.params[1];
    const jg::Verdict v = jg::verdict(mp < tol && mq < tol, a.lu_status[b], mp != mp || mq != mq, a.iters + b, maxit, b < a.batch);
    a.active[b] = v.go ? 1 : 0;
    a.status[b] = v.status;
    if (v.go) { a.iters[b] += 1; atomicAdd(a.counter, 1); }
}

// rows of a result record [.][stride] <- V | theta | iterations | status of lanes lane0 .. lane0 + count - 1 (rows[i] = record row)
__global__ __launch_bounds__(256) void k_pack_rows(const double* vm, const double* va, const int* iters, const int* status, const int* rows,
                                                   double* dst, int n, int ld, int lane0, long long stride) {
    const int i = blockIdx.y;
    const int b = lane0 + i;
    double* out = dst + (size_t)rows[i] * stride;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) { out[j] = vm[(size_t)j * ld + b]; out[n + j] = va[(size_t)j * ld + b]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[2 * n] = (double)iters[b]; out[2 * n + 1] = (double)status[b]; }
}

}  // namespace

namespace jg {
void set_last_error(const std::string& msg) { g_error = msg; }
}

struct jg_nr : jg::Lanes {             // Lanes: stream, batch, ld, the staging buffer of put_rows / get_rows, the pinned verdict word and the wait for it
    int n = 0, nnz = 0, mp = 0, device = 0, nchunk = 0;
    int64_t dimJ = 0, nnzJ = 0, slack = 0;
    std::vector<int64_t> colptr, rowval, pq, pvpq, pcount, jcolptr, jrowval;
    std::vector<int8_t> type;
    std::vector<int> tperm;          // Ybus CSC pointer -> block CSR index of the same (row, col)
    std::vector<int64_t> jmap;       // Jacobian CSC nz -> (factor entry holding the block)*4 + component
    // device
    int* d_rowptr = nullptr; int* d_col = nullptr; double* d_G = nullptr; double* d_B = nullptr; double2* d_GB = nullptr; int* d_rowtype = nullptr; int* d_rowtype_pre = nullptr;   // _pre: type | (pivot + 1) << 2 for the pivots of the plan's level 0
    signed char* d_type = nullptr; signed char* d_flags = nullptr;
    double* d_vm = nullptr; double* d_va = nullptr; double* d_p = nullptr; double* d_q = nullptr;
    int* d_ppos = nullptr; double* d_pdg = nullptr; double* d_pdb = nullptr;
    int* d_dst = nullptr; double* d_F = nullptr; double* d_inc = nullptr; double* d_part = nullptr;
    double* d_normp = nullptr; double* d_normq = nullptr; double* d_params = nullptr;
    double* d_vm0 = nullptr; double* d_va0 = nullptr;   // snapshot of the start point
    int* d_active = nullptr; int* d_iters = nullptr; int* d_status = nullptr; int* d_counter = nullptr; int* d_group = nullptr;
    int* d_lid = nullptr; int* d_dest = nullptr; int* d_cflags = nullptr; int* d_itmp = nullptr; int* d_glist = nullptr;   // scenario compaction (d_vm ... d_glist without d_dst, d_vm0, d_va0: ONE arena, jg_nr_create)
    jg::Compaction cmp{};                             // ... what it works on (jg_compact.hpp), filled once by jg_nr_create
    bool refine = false;                              // one step of iterative refinement per Newton step (jg_nr_set_refine)
    bool keep_inc = true;                             // jg_nr_set_keep_increment: the batched sweeps store method.increment (d_inc, bus order) and the lane moves carry it
    bool inc_fresh = true;                            // ... and d_inc holds what a run with the switch on left (jg_nr_get_increment refuses anything else)
    bool fast = false;                                // fast decoupled mode (jg_nr_fast_setup): constant B', B'' factorised once
    std::vector<double> fast_blk;                     // ... the shared block matrix diag(B', B'') as set up [nnz][4] (engine block order)
    std::vector<int> fp_entry; std::vector<double> fp_dp, fp_dq;   // per-scenario edits of B' / B'' (jg_nr_fast_patch_batch): [FAST_MP][batch] factor entry (-1: none), deltas
    int* d_fp_entry = nullptr; double* d_fp_dp = nullptr; double* d_fp_dq = nullptr;   // ... their device copies (allocated on first use)
    double* d_R = nullptr;                            // rhs of the half-iterations
    double* d_inc2[2] = {nullptr, nullptr};           // increments of the theta / V half-iterations
    const int* fast_mask = nullptr;                   // scenarios that take the update (nullptr: all)
    jg::Graph gFA, gFB;                               // mismatch + verdict / the two half-iterations (jg_nr_fast_run)
    int nb = 0;                                       // post-processing (jg_nr_set_branches)
    int* d_bfrom = nullptr; int* d_bto = nullptr; signed char* d_bstatus = nullptr; double* d_bparam = nullptr; int* d_outage = nullptr;
    double* d_post = nullptr; size_t post_bytes = 0;  // staging for branch / bus quantities, grown on demand
    double* d_rating = nullptr; double* d_screen = nullptr; double* d_screc = nullptr;   // contingency screen: ratings [nb], partial maxima, the record [batch][10]
    jg::Engine eng;
    jg::Graph gA, gB, gBm, gJ;                        // build_graphs; Bm / J: an iteration whose verdict assembles NO Jacobian / the Jacobian alone (run_loop)
    jg::Graph gM; int m_iters = 0;                    // ONE scenario: a whole solve of m_iters iterations as one graph (run_whole)
    int stop_hint = 0, iter_graphs = 0;               // iteration graphs after which the last run of this handle stopped / launched by the current run
    long long last_guess_hit = 0, last_guess_miss = 0;
    bool jac_valid = false;
    bool level0_done = false;        // the Jacobian in the factor storage came from an assembly that finished the plan's level 0
    bool f_stale = false;            // d_F does not hold every scenario's final mismatch yet (see run_finish)
    bool paused = false;             // jg_nr_run_defer stopped with scenarios still active (lanes compacted, not yet sent home)
    int* d_move = nullptr;           // straggler hand-off: map[64] | home[64] | count[1] | source lane[64] (device), home/count mirrored in h_move (pinned)
    int* h_move = nullptr;
    double host_launch_us = 0.0, host_wait_us = 0.0; long long host_iters = 0;   // JG_HOST_TIMING=1: what the host spent in hipGraphLaunch / waiting per iteration of run_loop
    bool res_pinned = false;         // this run's verdicts write iterations | status behind the pinned verdict word (one lane group; run_finish)
    int* h_counter_dev = nullptr;    // device alias of h_counter (pinned, 129 ints: the verdict word, then iterations [64] | status [64] of a handle of one lane group)
    // ---- first iteration on a shared factor (jg_comp.hpp; jg_nr_attach_base) ----
    std::vector<int> csr_row, csr_col;                // Ybus row-CSR position -> (row, column)
    jg_nr_base* base = nullptr;                       // the base case this handle's scenarios start from (nullptr: none attached)
    double* d_cw = nullptr;                           // scratch of the shared-factor sweeps [(n + top rows)][ld][2]
    bool start_is_base = false;                       // V, theta of every lane = the base's start (jg_nr_start_from_base; any other write clears it)
    int first_mode = 1;                               // jg_nr_set_first_iteration: 1 = compensated when the conditions hold, 0 = always refactorise
    std::vector<unsigned char> patch_state;           // [batch] 0 no edit, 1 edits within two adjacent buses (compensable), 2 other
    bool inj_checked = false, inj_equal = false;      // the lanes' injections were compared with the base's / equal it
    int* d_cmp = nullptr;                             // one word: mismatching injections (inj check)
    jg::Graph gA2, gC;                                // build_comp_graphs
    long long first_comp = 0, first_full = 0;         // runs whose first iteration went the one / the other way (jg_nr_first_iteration_counts)
    // ---- bus types per scenario (jg_nr_set_bus_type, jg_nr_reactive_limit) ----
    unsigned long long* d_lt = nullptr;               // [ceil(n / 32)][ld] lane words, 2 bits per bus; moves with the lanes (launch_compact)
    signed char* d_flags_all = nullptr;               // [n] = 3: while types differ per lane every variable is updated (a masked one has an increment of exactly 0)
    std::vector<unsigned char> lt_set;                // [batch] the scenario's types differ from the create-time ones
    std::vector<unsigned char> dead;                  // [batch] the last jg_nr_reactive_limit left the scenario without a slack (status 5)
    bool lt_on = false;                               // some scenario has types of its own: lane-typed assembly, all-variable update, lane words compacted
    jg::QlimTables qt;                                // generator table and initial point (jg_nr_set_generators; jg_qlim.hpp)
    int* d_skip = nullptr;                            // [ld] lanes jg_nr_reactive_limit leaves alone (no slack left)
    double* d_shift = nullptr;                        // [ld] jg_nr_adjust_angle
};

// The base case of a screen: ONE factorisation of the Jacobian at the common start state and what the per-scenario corrections read (jg_comp.hpp).
struct jg_nr_base {
    jg::CompBase cb;
    int n = 0, nnz = 0, device = 0;
    std::vector<int64_t> colptr, rowval;
    std::vector<int8_t> type;
    hipStream_t stream = nullptr;
    std::atomic<int> refs{1};                         // the creator + every attached handle
    double create_ms = 0.0;
};

namespace {

int set_device(jg_nr* h) { NR_HIP(hipSetDevice(h->device)); return 0; }

// What the first iteration on a shared factor may assume of a scenario's Ybus edits (jg_comp.hpp): they lie in the rows / columns of at most two buses,
// and two buses are joined by one of the edited entries (so J_0^-1 has their blocks on the Ybus pattern) -- what a branch outage / parameter change / a
// shunt change produce.  pos: row-CSR positions (-1 = none).
unsigned char classify_patch(const jg_nr* h, const int* pos, int k) {
    int a = -1, b = -1;
    bool any = false, joined = false;
    for (int m = 0; m < k; ++m) {
        if (pos[m] < 0) continue;
        any = true;
        const int ij[2] = {h->csr_row[pos[m]], h->csr_col[pos[m]]};
        for (int q = 0; q < 2; ++q) {
            if (a < 0 || ij[q] == a) a = ij[q];
            else if (b < 0 || ij[q] == b) b = ij[q];
            else return 2;
        }
        if (ij[0] != ij[1]) joined = true;
    }
    if (!any) return 0;
    return (b < 0 || joined) ? 1 : 2;
}

// Where the sweeps of the iteration store the bus-order increment: nowhere while the handle keeps none (a null `out` of BwdArgs / CSweepArgs / CTopArgs).
// The single-instance sweep (k_bwd1_*) always stores.
// (Engine::backsolve takes the single-instance path on single_bwd && jordan and refuses a null out there: deciding on single_bwd alone errs on the storing side,
// and that refusal is what would catch the two conditions drifting apart.)
double* inc_out(jg_nr* h) { return h->keep_inc || h->eng.single_bwd ? h->d_inc : nullptr; }
// The shared-factor step's scratch (d_cw) is read by its own backward rows only: under the conditions of the sweep-only factor the rows nobody names stay unstored
// (JG_SWEEP_DEAD=0: stored; read at every capture)
bool comp_dead_ok(jg_nr* h) { return h->eng.sweep_only && !h->refine && jg::knob("SWEEP_DEAD", 1) != 0; }

jg::GroupSel active_groups(jg_nr* h) { return jg::GroupSel{nullptr, h->d_glist, h->d_cflags + jg::CF_LIST}; }

// The runtime mp (0, 4, anything else = 8) and jac of a launch as template arguments: f(std::integral_constant<int, MP>{}[, std::bool_constant<JAC>{}])
template <class F> void with_mp(int mp, F&& f) {
    switch (mp) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}
template <class F> void with_mp_jac(int mp, bool jac, F&& f) {
    with_mp(mp, [&](auto m) { if (jac) f(m, std::true_type{}); else f(m, std::false_type{}); });
}

// level0: the assembly also finishes level 0 of the engine's plan (factorised diagonal blocks + rhs rows of the pivots nobody
// updates); the factorisation that follows must be told (h->level0_done).  Plain assemblies (getters, jg_nr_mismatch) leave it off.
void launch_assemble(jg_nr* h, const jg::GroupSel& sel = jg::GroupSel{}, bool jac = true, double* pq_out = nullptr, int fd_mode = 0, const int* only_if = nullptr,
                     bool level0 = false) {
    const bool pre = jac && level0 && h->eng.plan->S.prefactor && h->d_rowtype_pre;
    AsmArgs a{h->d_rowptr, h->d_col, h->d_GB, pre ? h->d_rowtype_pre : h->d_rowtype, h->d_dst, h->d_vm, h->d_va, h->d_p, h->d_q,
              h->d_ppos, h->d_pdg, h->d_pdb, h->eng.X, h->d_F, h->d_part, pq_out, sel, fd_mode ? h->d_R : nullptr, fd_mode, h->n, h->ld, h->mp, h->nchunk, h->batch, only_if,
              h->eng.W, h->eng.status, h->lt_on ? h->d_lt : nullptr};
    if (jac && !only_if) h->level0_done = pre;
    const bool lt = h->lt_on;                                     // scenarios with bus types of their own (jg_nr_set_bus_type): the lane-typed variant
    dim3 grid(jg::grid_blocks(h->ld / 64, h->nchunk)), block(64, ASM_WAVES);
    auto go = [&](auto kernel, dim3 g, dim3 b) { hipLaunchKernelGGL(kernel, g, b, 0, h->stream, a); };
    const bool single_env = jg::knob("SINGLE", 1) != 0;           // (read at every capture: bench.py holds the two forms against each other in one process)
    if (h->ld == 64 && h->batch == 1 && !fd_mode && !pq_out && !only_if && single_env) {      // ONE scenario: a quad of lanes per bus row (k_assemble1)
        const dim3 g1(jg::grid_blocks(1, (h->n + 63) / 64));
        with_mp_jac(h->mp, jac, [&](auto m, auto j) { go(k_assemble1<decltype(m)::value, decltype(j)::value>, g1, dim3(256)); });
        return;
    }
    if (h->ld == 64 && h->batch <= 32 && !fd_mode && !pq_out) {      // a handful of scenarios: one row per wave (k_assemble: WAVES = 16); same arithmetic per row, same chunk maxima
        const bool w16 = h->nchunk <= 512;                          // grids whose workgroups are all resident at once: one row per wave; larger ones: two
        const dim3 wide(64, w16 ? 16 : 8);
        with_mp_jac(h->mp, jac, [&](auto m, auto j) {
            constexpr int MP = decltype(m)::value; constexpr bool JAC = decltype(j)::value;
            if (lt) { if (w16) go(k_assemble<MP, JAC, 16, true>, grid, wide); else go(k_assemble<MP, JAC, 8, true>, grid, wide); }
            else { if (w16) go(k_assemble<MP, JAC, 16, false>, grid, wide); else go(k_assemble<MP, JAC, 8, false>, grid, wide); }
        });
        return;
    }
    with_mp_jac(h->mp, jac, [&](auto m, auto j) {
        constexpr int MP = decltype(m)::value; constexpr bool JAC = decltype(j)::value;
        if (lt) go(k_assemble<MP, JAC, ASM_WAVES, true>, grid, block); else go(k_assemble<MP, JAC>, grid, block);
    });
}

// The verdict of a handle of ONE lane group in one launch (round 6): k_check's norms and loop control, then what k_compact comes to when there is nothing to pack --
// the count of active scenarios for the host, the group list of the next launches, iterations | status for jg_nr_run when the last scenario has finished.  Two
// launches (12.5 + 4 us of a single instance's 330 us iteration: five trips of dependent loads over the 625 chunk norms, a launch boundary) become one of two trips.
__global__ __launch_bounds__(1024) void k_verdict64(CheckArgs a, jg::CompactArgs p) {
    __shared__ double red[2][16][64];
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int b = lane;
    // every request of the launch leaves at once: the group flag (a finished group keeps its verdict: its assembly was skipped), what the loop control reads
    // besides the norms, and the chunk maxima -- nothing is asked for behind a branch on something else that was asked for
    const int grp_on = a.group ? a.group[0] : 1;
    const double tol = a.params[0];
    const int maxit = (int)a.params[1];
    const int lus = a.lu_status[b], its = a.iters[b], act0 = a.active[b], st0 = a.status[b];
    double mp = 0.0, mq = 0.0;
    if (a.batch == 1) {
        // ONE scenario: the threads are CHUNKS (scenario 0 of chunk t, t + 1024, ...): one round trip where 16 waves of 64 identical lanes took two to five
        for (int c = wave * 64 + lane; c < a.nchunk; c += 1024) {
            mp = pf::nanmax(a.part[((size_t)c * 2) * a.ld], mp);
            mq = pf::nanmax(a.part[((size_t)c * 2 + 1) * a.ld], mq);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { mp = pf::nanmax(__shfl_xor(mp, d), mp); mq = pf::nanmax(__shfl_xor(mq, d), mq); }
        if (lane < 16) { red[0][wave][0] = mp; red[1][wave][0] = mq; }            // (lanes 0 .. 15 write the same value)
    } else {
        constexpr int CU = 20;
        for (int c0 = wave; c0 < a.nchunk; c0 += 16 * CU) {
            double x[CU], y[CU];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const int c = min(c0 + 16 * u, a.nchunk - 1);     // a repeated chunk changes no maximum
                x[u] = a.part[((size_t)c * 2) * a.ld + b]; y[u] = a.part[((size_t)c * 2 + 1) * a.ld + b];
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) { mp = pf::nanmax(x[u], mp); mq = pf::nanmax(y[u], mq); }
        }
        red[0][wave][lane] = mp;
        red[1][wave][lane] = mq;
    }
    __syncthreads();
    if (wave != 0) return;
    const bool skip = grp_on == 0;
    int act = act0, it_out = its, st_out = st0;
    if (!skip) {
        const int src = a.batch == 1 ? 0 : lane;                  // one scenario: every lane takes its maxima (lanes beyond the batch alias the last scenario)
        for (int w = a.batch == 1 ? 0 : 1; w < 16; ++w) { mp = pf::nanmax(red[0][w][src], mp); mq = pf::nanmax(red[1][w][src], mq); }
        a.normp[b] = mp;
        a.normq[b] = mq;
        const jg::Verdict v = jg::verdict(mp < tol && mq < tol, lus, mp != mp || mq != mq, &its, maxit, b < a.batch);
        act = v.go ? 1 : 0;
        a.active[b] = act;
        st_out = v.status;
        a.status[b] = st_out;
        if (v.go) { it_out = its + 1; a.iters[b] = it_out; atomicAdd(a.counter, 1); }
    }
    const int n_active = __popcll(__ballot(act != 0));
    if (p.host_res && n_active == 0) { p.host_res[lane] = it_out; p.host_res[64 + lane] = st_out; __threadfence_system(); }   // ... ahead of the word the host polls
    if (lane == 0) {
        p.flags[0] = 0; p.flags[1] = n_active; p.flags[4] = 0;
        p.group[0] = n_active > 0 ? 1 : 0;
        if (n_active > 0) p.glist[0] = 0;
        p.flags[3] = n_active > 0 ? 1 : 0;
        if (p.host_count) *p.host_count = n_active;
    }
}

CheckArgs check_args(jg_nr* h, const int* group, int mode) {
    return CheckArgs{h->d_part, h->nchunk, h->ld, h->batch, h->d_params, h->d_normp, h->d_normq, h->d_active, h->d_iters, h->d_status, h->eng.status, h->d_counter, group, mode};
}
void launch_verdict64(jg_nr* h, bool report) {         // (handles of one lane group only)
    hipLaunchKernelGGL(k_verdict64, dim3(1), dim3(64, 16), 0, h->stream, check_args(h, h->d_group, 1), h->cmp.args(0, report));
}

void launch_check(jg_nr* h, int mode, const int* group = nullptr) {
    hipLaunchKernelGGL(k_check, dim3(h->ld / 64), dim3(64, 16), 0, h->stream, check_args(h, group, mode));
}

// pack the active scenarios into the leading lanes (restore = 1: send every lane back home), with everything a scenario owns
void launch_compact(jg_nr* h, int restore, bool report = false) {
    std::vector<jg::LaneRows> rows{{h->d_vm, h->n, 1}, {h->d_va, h->n, 1}, {h->d_p, h->n, 1}, {h->d_q, h->n, 1}};
    if (h->mp > 0) { rows.push_back({h->d_pdg, h->mp, 1}); rows.push_back({h->d_pdb, h->mp, 1}); }
    if (h->keep_inc) rows.push_back({h->d_inc, h->n, 2});   // a finished scenario keeps ITS last increment (method.increment) wherever its lane goes; not kept: nothing to carry
    if (h->lt_on) rows.push_back({(double*)h->d_lt, (h->n + 31) / 32, 1});      // the types of a scenario travel with it (8th and last slot)
    h->cmp.launch_compact(h->stream, restore, report, rows);
}

// solve! numerics on the groups of `sel`: factorise the Jacobian that is in place, solve, update the state (active: nullable)
int newton_step(jg_nr* h, const jg::GroupSel& sel, const int* active) {
    if (int rc = h->eng.factor(h->stream, nullptr, h->d_F, sel, h->level0_done)) return rc;
    if (!h->refine) {
        jg::StateUpdate upd{h->d_va, h->d_vm, h->lt_on ? h->d_flags_all : h->d_flags, active, -1.0};
        return h->eng.backsolve(h->stream, inc_out(h), upd, sel);
    }
    // (a refining handle keeps its increment: jg_nr_set_refine switches jg_nr_set_keep_increment back on -- k_refine_apply writes d_inc)
    // the plain solve goes to a scratch vector: method.increment (d_inc) is written for ACTIVE scenarios only, by k_refine_apply -- a
    // finished scenario of an active lane group keeps its last increment, as without refinement
    jg::StateUpdate none{};
    if (int rc = h->eng.backsolve(h->stream, h->d_inc2[1], none, sel)) return rc;
    RefineArgs a{h->d_rowptr, h->d_col, h->d_GB, h->d_rowtype, h->d_vm, h->d_va, h->d_ppos, h->d_pdg, h->d_pdb,
                 h->d_F, h->d_inc2[1], h->d_R, sel, h->n, h->ld, h->mp, h->nchunk, h->batch};
    dim3 grid(jg::grid_blocks(h->ld / 64, h->nchunk)), block(64, ASM_WAVES);
    with_mp(h->mp, [&](auto m) { hipLaunchKernelGGL((k_refine_residual<decltype(m)::value>), grid, block, 0, h->stream, a); });
    if (int rc = h->eng.forward(h->stream, h->d_R, sel)) return rc;
    if (int rc = h->eng.backsolve(h->stream, h->d_inc2[0], none, sel)) return rc;
    hipLaunchKernelGGL(k_refine_apply, dim3(jg::grid_blocks(h->ld / 64, (h->n + 15) / 16)), dim3(64, 16), 0, h->stream,
                       h->d_inc, h->d_inc2[1], h->d_inc2[0], h->d_va, h->d_vm, h->d_flags, active, sel, h->n, h->ld, h->batch);
    return 0;
}

// A, B, Bm and J are built all or nothing: a failure leaves the four empty and the next call builds again.
int build_graphs(jg_nr* h) {
    if (h->gA) return 0;
    // One pass decides AND prepares: mismatch + Jacobian in one assembly (the Jacobian of a finished batch is the only waste:
    // one write stream per solve, against a second walk over Ybus per iteration), verdict per scenario, compaction of the
    // still-active lanes.  A compaction moves lanes (and stages them in the factor storage), so the assembly is repeated
    // on the packed lanes -- a launch that returns at once unless the compaction flag is set.
    auto check_and_compact = [&]() {
        if (h->ld == 64) { launch_verdict64(h, true); return; }     // one lane group: ONE launch (k_verdict64)
        launch_check(h, 1, h->d_group);
        launch_compact(h, 0, true);                    // also reports the number of active scenarios to the host word
    };
    auto verdict = [&]() {
        launch_assemble(h, active_groups(h), true, nullptr, 0, nullptr, true);
        check_and_compact();
        if (h->ld > 64) launch_assemble(h, active_groups(h), true, nullptr, 0, h->d_cflags + jg::CF_PERMUTE, true);
    };
    auto step = [&]() { const int rc = newton_step(h, active_groups(h), h->d_active); return rc ? fail(rc, h->eng.error) : 0; };
    // graph A: the verdict on the start point
    int rc = h->gA.capture(h->stream, [&] { verdict(); return 0; });
    // graph B: one iteration on the packed lanes (factorise the Jacobian that is already in place, solve, update), then the
    // verdict on the new state
    if (!rc) rc = h->gB.capture(h->stream, [&] { if (int rc = step()) return rc; verdict(); return 0; });
    // graph Bm: the same iteration with a verdict from a MISMATCH-ONLY pass -- for the iteration the handle expects to be the last of its run (run_loop): the
    // Jacobian a verdict assembles is wasted on every scenario that converges (nobody factorises it) and on every scenario that leaves for a pool (jg_nr_resume
    // assembles where they arrive), 0.87 GB of a 512-scenario batch against 0.26 GB for the mismatch pass.  graph J: the Jacobian alone, when the guess was wrong.
    if (!rc) rc = h->gBm.capture(h->stream, [&] {
        if (int rc = step()) return rc;
        launch_assemble(h, active_groups(h), false);
        check_and_compact();
        if (h->ld > 64) launch_assemble(h, active_groups(h), false, nullptr, 0, h->d_cflags + jg::CF_PERMUTE);
        return 0;
    });
    if (!rc) rc = h->gJ.capture(h->stream, [&] { launch_assemble(h, active_groups(h), true, nullptr, 0, nullptr, true); return 0; });
    if (rc) for (jg::Graph* g : {&h->gA, &h->gB, &h->gBm, &h->gJ}) g->reset();
    return rc;
}

void drop_iteration_graphs(jg_nr* h) {
    for (jg::Graph* g : {&h->gA, &h->gB, &h->gBm, &h->gJ, &h->gM}) g->reset();
    h->m_iters = 0;
}

// ONE scenario: the whole solve as ONE graph (round 6).  Every graph costs ~10 us on the device before its first kernel starts (the gap between two iteration graphs in
// the trace; launching the next graph ahead of the verdict did not close it), and a single instance launches one per iteration + one for the verdict on its start: 5 % of
// its solve.  A handle of one scenario that has solved before knows how many iterations to expect (stop_hint); its next solve is the start verdict + that many iterations
// in one graph -- only the LAST verdict reports to the host, from a mismatch-only pass as in graph Bm; an iteration behind the convergence runs as launches that return
// at once (the group list is empty).  Fewer iterations than expected: nothing to do; more: graph J supplies the Jacobian and run_loop carries on.
int build_whole_graph(jg_nr* h, int k) {
    if (h->gM && h->m_iters == k) return 0;
    h->m_iters = 0;
    const int rc = h->gM.capture(h->stream, [&] {
        launch_assemble(h, active_groups(h), true, nullptr, 0, nullptr, true);       // the verdict on the start point (graph A)
        launch_verdict64(h, false);
        for (int it = 1; it <= k; ++it) {
            if (int rc = newton_step(h, active_groups(h), h->d_active)) return fail(rc, h->eng.error);
            if (it < k) { launch_assemble(h, active_groups(h), true, nullptr, 0, nullptr, true); launch_verdict64(h, false); }      // graph B
            else { launch_assemble(h, active_groups(h), false); launch_verdict64(h, true); }                                         // graph Bm: the expected last iteration
        }
        return 0;
    });
    if (!rc) h->m_iters = k;
    return rc;
}

void drop_comp_graphs(jg_nr* h) { h->gA2.reset(); h->gC.reset(); }

void release_base(jg_nr_base* b) {
    if (!b) return;
    if (b->refs.fetch_sub(1) == 1) {
        hipSetDevice(b->device);
        b->cb.destroy();
        if (b->stream) hipStreamDestroy(b->stream);
        delete b;
    }
}

void detach_base(jg_nr* h) {
    if (!h->base) return;
    if (h->stream) hipStreamSynchronize(h->stream);
    drop_comp_graphs(h);
    h->release(&h->d_cw);
    release_base(h->base);
    h->base = nullptr;
    h->start_is_base = false;
}

// The two graphs of a compensated start (jg_comp.hpp).  A2: the verdict on the start point from a MISMATCH-ONLY pass (no Jacobian is assembled: nobody
// factorises it).  C: the first iteration -- per-scenario correction of the right-hand side, ONE sweep pair on the base's factor with the state update
// fused in, then the usual verdict on the new state (which assembles the Jacobian the second iteration factorises).
int build_comp_graphs(jg_nr* h) {
    if (h->gC) return 0;
    const jg::CompBase& cb = h->base->cb;
    int rc = h->gA2.capture(h->stream, [&] {
        launch_assemble(h, active_groups(h), false);
        launch_check(h, 1, h->d_group);
        launch_compact(h, 0, true);
        if (h->ld > 64) launch_assemble(h, active_groups(h), false, nullptr, 0, h->d_cflags + jg::CF_PERMUTE);      // lanes moved: their mismatch rows again
        return 0;
    });
    if (!rc) rc = h->gC.capture(h->stream, [&] {
        jg::CompFixArgs fa{h->d_ppos, h->d_pdg, h->d_pdb, h->mp, cb.rowptr, cb.colm, cb.posrow, cb.rowtype, cb.v0, cb.th0, cb.y0, cb.Zc,
                           h->d_F, h->eng.status, h->d_active, h->ld, h->batch};
        if (h->mp > 0) jg::launch_comp_fix(fa, h->stream);
        jg::StateUpdate upd{h->d_va, h->d_vm, h->d_flags, h->d_active, -1.0};
        if (int rc = cb.solve(cb.split, h->stream, h->d_F, h->d_cw, inc_out(h), h->ld, h->batch, upd, active_groups(h), comp_dead_ok(h))) return fail(rc, "the shared-factor sweep could not be captured");
        launch_assemble(h, active_groups(h), true, nullptr, 0, nullptr, true);
        launch_check(h, 1, h->d_group);
        launch_compact(h, 0, true);
        if (h->ld > 64) launch_assemble(h, active_groups(h), true, nullptr, 0, h->d_cflags + jg::CF_PERMUTE, true);
        return 0;
    });
    if (rc) drop_comp_graphs(h);
    return rc;
}

// mismatching injections between the lanes and the base (one word)
__global__ void k_cmp_injection(const double* p, const double* q, const double* p0, const double* q0, int n, int ld, int batch, int* count) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    int bad = 0;
    for (int i = blockIdx.y; i < n; i += gridDim.y) bad += (p[(size_t)i * ld + b] != p0[i]) || (q[(size_t)i * ld + b] != q0[i]);
    if (bad) atomicAdd(count, bad);
}

// Does the next run start with the compensated iteration?  (every condition the algebra of jg_comp.hpp rests on)
int comp_ready(jg_nr* h, bool& ready) {
    ready = false;
    if (!h->base || !h->first_mode || !h->start_is_base || h->refine || h->fast || h->lt_on) return 0;   // (the base's factor has the create-time types)
    bool patched = false;
    for (unsigned char c : h->patch_state) { if (c == 2) return 0; patched |= c == 1; }
    if (patched) {                                               // an outage moves the mismatch of its two buses only if the injections are the base's
        if (!h->inj_checked) {
            NR_HIP(hipMemsetAsync(h->d_cmp, 0, sizeof(int), h->stream));
            hipLaunchKernelGGL(k_cmp_injection, dim3((h->batch + 255) / 256, 64), dim3(256), 0, h->stream, h->d_p, h->d_q, h->base->cb.p0, h->base->cb.q0, h->n, h->ld, h->batch, h->d_cmp);
            int bad = 0;
            NR_HIP(jg::sync_copy(&bad, h->d_cmp, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            h->inj_checked = true; h->inj_equal = bad == 0;
        }
        if (!h->inj_equal) return 0;
    }
    if (int rc = build_comp_graphs(h)) return rc;
    ready = true;
    return 0;
}


// ---- bus types per scenario (jg_nr_set_bus_type, jg_nr_reactive_limit) -------------------------------------------------------------------
int lt_rows(const jg_nr* h) { return (h->n + 31) / 32; }

// 2 bits per bus, 32 buses per word (row r holds buses 32 r .. 32 r + 31); a bus beyond n is 0
void pack_types(const int8_t* type, int n, unsigned long long* words, int rows, size_t stride) {
    for (int r = 0; r < rows; ++r) {
        unsigned long long w = 0;
        for (int q = 0; q < 32 && r * 32 + q < n; ++q) w |= (unsigned long long)(type[r * 32 + q] & 3) << (2 * q);
        words[(size_t)r * stride] = w;
    }
}

// the lane words exist (every lane: the create-time types) and so does the all-variable update flag array
int ensure_lane_types(jg_nr* h) {
    if (h->d_lt) return 0;
    const int rows = lt_rows(h);
    std::vector<unsigned long long> one(rows), all((size_t)rows * h->ld);
    pack_types(h->type.data(), h->n, one.data(), rows, 1);
    for (int r = 0; r < rows; ++r) for (int b = 0; b < h->ld; ++b) all[(size_t)r * h->ld + b] = one[r];
    if (h->upload(&h->d_lt, all) || h->upload(&h->d_flags_all, std::vector<signed char>(h->n, 3))) return 2;
    h->lt_set.assign(h->batch, 0);
    h->dead.assign(h->batch, 0);
    return 0;
}

// the assembly, the compaction and the state update are captured for one choice: a change of it drops the graphs
void set_lane_types_on(jg_nr* h) {
    bool on = false;
    for (unsigned char c : h->lt_set) on |= c != 0;
    if (on != h->lt_on) {
        hipStreamSynchronize(h->stream);
        drop_iteration_graphs(h);
        drop_comp_graphs(h);
    }
    h->lt_on = on;
}

// a scenario that jg_nr_reactive_limit left without a slack reports status 5 (the reference's errorSlackDefinition) on the host and on the device
int mark_dead(jg_nr* h, int32_t* status) {
    if (h->dead.empty()) return 0;
    const int five = 5;
    for (int b = 0; b < h->batch; ++b) {
        if (!h->dead[b]) continue;
        if (status) status[b] = 5;
        NR_HIP(hipMemcpyAsync(h->d_status + b, &five, sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

}  // namespace

extern "C" {

const char* jg_last_error(void) { return g_error.c_str(); }

void jg_plan_cache_clear(void) { jg::clear_plan_cache(); }

int jg_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return -1;
    return c;
}

int jg_nr_create(jg_nr** out, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* y_reim,
                 const double* yt_reim, const int8_t* type, int64_t slack, int64_t batch, int64_t max_patch,
                 int device) {
    if (batch > 65472) return fail(1, "jg_nr_create: at most 65 472 scenarios per handle (lane bookkeeping of the compaction: 16-bit counts)");
    if (!out || n < 1 || !colptr || !rowval || !y_reim || !yt_reim || !type || batch < 1 || max_patch < 0 || max_patch > 8)
        return fail(1, "jg_nr_create: bad argument");
    if (slack < 1 || slack > n || type[slack - 1] != 3) return fail(1, "The slack bus is missing.");
    int ndev = 0;
    NR_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(1, "jg_nr_create: no such HIP device");
    const double tc0 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
    jg_nr* h = new jg_nr();
    h->n = (int)n; h->batch = (int)batch; h->ld = (int)((batch + 63) / 64 * 64);
    h->mp = max_patch == 0 ? 0 : (max_patch <= 4 ? 4 : 8);
    h->device = device; h->slack = slack;
    h->nnz = (int)(colptr[n] - 1);
    h->colptr.assign(colptr, colptr + n + 1);
    h->rowval.assign(rowval, rowval + h->nnz);
    h->type.assign(type, type + n);
    const int nnz = h->nnz;
    if (n >= (1 << 24)) { delete h; return fail(1, "jg_nr_create: more than 2^24 buses"); }
    for (int c = 0; c < n; ++c) {
        if (colptr[c + 1] < colptr[c] || colptr[c] < 1 || colptr[c + 1] - 1 > nnz) { delete h; return fail(1, "jg_nr_create: malformed column pointers"); }
        for (int64_t p = colptr[c] - 1; p < colptr[c + 1] - 1; ++p)
            if (rowval[p] < 1 || rowval[p] > n) { delete h; return fail(1, "jg_nr_create: row index out of range"); }
    }
    // The symbolic analysis of the block LU (or its look-up in the plan cache), the upload of its tables and the factor storage need the pattern
    // and nothing else: they run on a thread of their own while this one builds the reference's maps, uploads the model and allocates the state
    // (round 4: what a first power flow on a grid waits for is the analysis -- 19 of 30 ms on the 10 000-bus grid -- not analysis + the rest).
    int rc = set_device(h);
    if (rc) { delete h; return rc; }
    std::vector<int> rp(n + 1), cl(nnz);
    for (int i = 0; i <= n; ++i) rp[i] = (int)(colptr[i] - 1);
    for (int p = 0; p < nnz; ++p) cl[p] = (int)(rowval[p] - 1);
    // in place: the assembly kernel writes into the factor storage; bit 2: it also finishes the plan's level 0 (jg_symbolic.hpp: prefactor)
    // bit 49: Jordan rows for the pivots of the top tasks (jg_symbolic.hpp): the backward sweep over the top of the tree is a handful of
    // plain levels instead of sequential chains (refined steps and fast Newton-Raphson switch the engine back: Engine::jordan)
    h->eng.lanes = h->batch;                                    // (known before the plan is chosen: a handful of scenarios gets a deeper top)
    int eng_rc = 0;
    std::atomic<int> stream_state{0};                           // 1: h->stream exists, -1: its creation failed (the analysis thread creates it first)
    auto eng_work = [&] {
        if (hipSetDevice(h->device) != hipSuccess) { h->eng.error = "hipSetDevice failed on the analysis thread"; eng_rc = 2; stream_state = -1; return; }
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->eng.error = "jg_nr_create: stream creation failed"; eng_rc = 2; stream_state = -1; return; }
        stream_state = 1;
        eng_rc = h->eng.create((int)n, rp.data(), cl.data(), h->ld, (jg::knob_set("NO_PREFACTOR") ? 1LL : 1LL | 4) | 1LL << 49, h->stream);
    };
    std::thread eng_thread;
    try { eng_thread = std::thread(eng_work); } catch (const std::system_error&) { eng_work(); }     // no thread to be had: the analysis first, then the rest
    // every failure from here on waits for the analysis thread, then the half-built handle goes
    struct Unwind { jg_nr* h; std::thread& t; ~Unwind() { if (t.joinable()) t.join(); if (h) jg_nr_destroy(h); } } unwind{h, eng_thread};
    h->csr_col = cl;
    h->csr_row.assign(nnz, 0);
    for (int i = 0; i < n; ++i) for (int p = rp[i]; p < rp[i + 1]; ++p) h->csr_row[p] = i;
    h->patch_state.assign((size_t)batch, 0);
    // transpose permutation of the (structurally symmetric) pattern: tperm[p of (r,c)] = pointer of (c,r)
    h->tperm.assign(nnz, -1);
    for (int c = 0; c < n; ++c)
        for (int64_t p = colptr[c] - 1; p < colptr[c + 1] - 1; ++p) {
            const int64_t r = rowval[p] - 1;
            int64_t lo = colptr[r] - 1, hi = colptr[r + 1] - 2, q = -1;
            while (lo <= hi) { int64_t m = (lo + hi) >> 1; if (rowval[m] - 1 < c) lo = m + 1; else if (rowval[m] - 1 > c) hi = m - 1; else { q = m; break; } }
            if (q < 0) return fail(1, "jg_nr_create: Ybus pattern is not structurally symmetric");
            h->tperm[p] = (int)q;
        }
    // ---- newtonJacobian (acPowerFlow.jl:89-175), integer only -------------------------------
    h->pq.assign(n, 0); h->pvpq.assign(n, 0); h->pcount.assign(n, 0);
    int64_t pvpqNum = 0, pqNum = 0;
    for (int i = 0; i < n; ++i) {
        if (type[i] == 1) { pqNum++; h->pq[i] = pqNum + n - 1; }
        if (type[i] != 3) { pvpqNum++; h->pvpq[i] = pvpqNum; }
    }
    h->dimJ = n + pqNum - 1;
    std::vector<int64_t> colcount(h->dimJ, 0), qcount(n, 0);
    for (int i = 0; i < n; ++i) {
        if (i + 1 == slack) continue;
        for (int64_t p = colptr[i] - 1; p < colptr[i + 1] - 1; ++p) {
            const int8_t tr = type[rowval[p] - 1];
            if (tr != 3) h->pcount[i]++;
            if (tr == 1) qcount[i]++;
        }
        colcount[h->pvpq[i] - 1] = h->pcount[i] + qcount[i];
        if (type[i] == 1) colcount[h->pq[i] - 1] = h->pcount[i] + qcount[i];
    }
    h->jcolptr.assign(h->dimJ + 1, 1);
    for (int64_t c = 0; c < h->dimJ; ++c) h->jcolptr[c + 1] = h->jcolptr[c] + colcount[c];
    h->nnzJ = h->jcolptr[h->dimJ] - 1;
    h->jrowval.assign(h->nnzJ, 0);
    h->jmap.assign(h->nnzJ, 0);
    for (int i = 0; i < n; ++i) {
        if (i + 1 == slack) continue;
        const bool isPQ = type[i] == 1;
        int64_t pA = h->jcolptr[h->pvpq[i] - 1], qA = pA + h->pcount[i];
        int64_t pM = isPQ ? h->jcolptr[h->pq[i] - 1] : 0, qM = isPQ ? pM + h->pcount[i] : 0;
        for (int64_t p = colptr[i] - 1; p < colptr[i + 1] - 1; ++p) {
            const int64_t row = rowval[p] - 1;
            const int8_t tr = type[row];
            const int64_t blk = (int64_t)h->tperm[p] * 4;      // block (row, i) in row-CSR order
            if (tr != 3) {
                h->jrowval[pA - 1] = h->pvpq[row]; h->jmap[pA - 1] = blk + 0; pA++;
                if (isPQ) { h->jrowval[pM - 1] = h->pvpq[row]; h->jmap[pM - 1] = blk + 1; pM++; }
            }
            if (tr == 1) {
                h->jrowval[qA - 1] = h->pq[row]; h->jmap[qA - 1] = blk + 2; qA++;
                if (isPQ) { h->jrowval[qM - 1] = h->pq[row]; h->jmap[qM - 1] = blk + 3; qM++; }
            }
        }
    }
    // ---- device upload ----------------------------------------------------------------------
    while (stream_state.load() == 0) std::this_thread::yield();
    if (stream_state.load() < 0) return fail(2, h->eng.error);
    if (jg::knob_set("PLAN_TIMING")) fprintf(stderr, "[jg nr create] reference maps done at                  %6.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() - tc0);
    std::vector<double> G(nnz), B(nnz);
    for (int p = 0; p < nnz; ++p) { G[p] = yt_reim[2 * p]; B[p] = yt_reim[2 * p + 1]; }
    std::vector<int> colm(nnz);                 // column | existence mask of the 2x2 block entries (row i, col j types)
    for (int i = 0; i < n; ++i)
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            const int j = cl[p];
            const int rpm = type[i] != 3, rq = type[i] == 1, ct = type[j] != 3, cv = type[j] == 1;
            colm[p] = j | (((rpm & ct) | ((rpm & cv) << 1) | ((rq & ct) << 2) | ((rq & cv) << 3)) << 24);
        }
    std::vector<double2> GBv(nnz);
    for (int p = 0; p < nnz; ++p) GBv[p] = double2{G[p], B[p]};
    // consistency of the two value arrays the reference keeps (T1): yT[p] must equal y[tperm[p]]
    for (int p = 0; p < nnz; ++p)
        if (y_reim[2 * (size_t)h->tperm[p]] != yt_reim[2 * p] || y_reim[2 * (size_t)h->tperm[p] + 1] != yt_reim[2 * p + 1])
            return fail(4, "jg_nr_create: nodalMatrix and nodalMatrixTranspose disagree (stale model)");
    std::vector<signed char> flags(n);
    for (int i = 0; i < n; ++i) flags[i] = (signed char)((type[i] != 3 ? 1 : 0) | (type[i] == 1 ? 2 : 0));
    std::vector<signed char> tp(type, type + n);
    if (h->upload(&h->d_rowptr, rp) || h->upload(&h->d_col, colm) || h->upload(&h->d_G, G) || h->upload(&h->d_B, B) || h->upload(&h->d_GB, GBv) ||
        h->upload(&h->d_rowtype, std::vector<int>(type, type + n)) || h->upload(&h->d_type, tp) || h->upload(&h->d_flags, flags)) return 2;
    h->nchunk = (h->n + ASM_ROWS - 1) / ASM_ROWS;
    const size_t ld = h->ld;
    // the per-handle state as ONE allocation and ONE fill (round 4: 23 x (hipMalloc + fill + stream synchronisation) were 2 of the 4 ms a handle on a
    // cached plan costs); every array starts on a 256-byte boundary
    const size_t mpn = h->mp > 0 ? h->mp : 1;
    const hipError_t arena_err = h->arena({
        {&h->d_vm, n * ld * 8}, {&h->d_va, n * ld * 8}, {&h->d_p, n * ld * 8}, {&h->d_q, n * ld * 8},
        {&h->d_ppos, mpn * ld * 4}, {&h->d_pdg, mpn * ld * 8}, {&h->d_pdb, mpn * ld * 8},
        {&h->d_F, n * 2 * ld * 8}, {&h->d_inc, n * 2 * ld * 8}, {&h->d_part, (size_t)h->nchunk * 2 * ld * 8},
        {&h->d_normp, ld * 8}, {&h->d_normq, ld * 8}, {&h->d_params, 4 * 8}, {&h->d_active, ld * 4},
        {&h->d_iters, ld * 4}, {&h->d_status, ld * 4}, {&h->d_counter, 4}, {&h->d_group, (ld / 64) * 4},
        {&h->d_lid, ld * 4}, {&h->d_dest, ld * 4}, {&h->d_cflags, 32}, {&h->d_itmp, ld * 4},
        {&h->d_glist, std::max<size_t>(ld / 64, 8) * 4}});    // map_block reads the first eight entries in one scalar load
    if (arena_err != hipSuccess) return fail(2, "jg_nr_create: device allocation failed");
    if (jg::sync_fill(h->d_ppos, 0xff, mpn * ld * 4, h->stream) != hipSuccess ||     // -1 = no patch
        h->pin(&h->h_counter, 129) != hipSuccess)                                    // the verdict word + iterations | status of one lane group (k_compact: host_res)
        return fail(2, "jg_nr_create: pinned allocation failed");
    if (hipHostGetDevicePointer((void**)&h->h_counter_dev, h->h_counter, 0) != hipSuccess) return fail(2, "jg_nr_create: pinned host word is not device-visible");
    const bool timing = jg::knob_set("PLAN_TIMING");
    auto tnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    if (timing) fprintf(stderr, "[jg nr create] maps, model upload, state arena done at %6.1f ms\n", tnow() - tc0);
    if (eng_thread.joinable()) eng_thread.join();
    if (timing) fprintf(stderr, "[jg nr create] engine joined at                        %6.1f ms\n", tnow() - tc0);
    if (eng_rc) return fail(eng_rc, h->eng.error);
    // Every reader of this handle's factor other than the Jordan sweep -- forward() of a refined or fast step, the compact factor of jg_nr_base_create -- switches
    // Engine::jordan off for its factorisation, and with it this flag: the iteration graphs then leave the top tasks' dead entries unstored (JG_SWEEP_ONLY=0: stored)
    h->eng.sweep_only = jg::knob("SWEEP_ONLY", 1) != 0;
    if (int rc = h->upload(&h->d_dst, h->eng.plan->S.src_entry)) return rc;
    if (h->eng.plan->S.prefactor) {                            // the row table of the assemblies that also finish the plan's level 0
        std::vector<int> rt(type, type + n);
        for (int k = 0; k < (int)n; ++k) if (h->eng.plan->S.pre_pivot[k]) rt[h->eng.plan->S.perm[k]] |= (k + 1) << 2;
        if (int rc = h->upload(&h->d_rowtype_pre, rt)) return rc;
    }
    h->eng.lanes = h->batch;
    h->cmp = jg::Compaction{h->d_active, h->d_iters, h->d_status, h->eng.status, h->d_lid, h->d_ppos, h->d_dest, h->d_group, h->d_glist, h->d_cflags, h->d_itmp,
                            h->mp, h->ld, h->d_params, h->h_counter_dev, h->eng.X, h->eng.factor_bytes()};
    if (!h->cmp.fits(2 * (size_t)n)) return fail(1, "jg_nr_create: the factor storage does not hold one increment (the staging area of the lane moves)");
    for (int64_t k = 0; k < h->nnzJ; ++k) h->jmap[k] = (int64_t)h->eng.plan->S.src_entry[h->jmap[k] >> 2] * 4 + (h->jmap[k] & 3);
    if (timing) fprintf(stderr, "[jg nr create] done at                                 %6.1f ms\n", tnow() - tc0);
    unwind.h = nullptr;
    *out = h;
    return 0;
}

void jg_nr_destroy(jg_nr* h) {
    if (h && jg::knob_set("HOST_TIMING") && h->host_iters > 0)
        fprintf(stderr, "[jg host timing] %d lanes: %lld iterations, hipGraphLaunch %.1f us, wait for the verdict %.1f us per iteration; last iteration guessed right %lld times, wrong %lld\n", h->ld, h->host_iters,
                h->host_launch_us / h->host_iters, h->host_wait_us / h->host_iters, h->last_guess_hit, h->last_guess_miss);
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    detach_base(h);
    h->eng.destroy();
    h->qt.destroy();
    drop_iteration_graphs(h);
    drop_comp_graphs(h);
    h->gFA.reset(); h->gFB.reset();
    h->release_all();
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int jg_nr_dims(jg_nr* h, int64_t* dims) {
    if (!h || !dims) return fail(1, "jg_nr_dims: bad argument");
    dims[0] = h->dimJ; dims[1] = h->nnzJ; dims[2] = h->eng.plan->S.n_entries; dims[3] = h->eng.plan->S.n_sched_terms;
    dims[4] = (int64_t)(h->eng.fact.size() + h->eng.plan->S.top_launch.size());      // dependent launches of one factorisation
    dims[5] = (int64_t)(h->eng.jordan ? h->eng.bwdj.size() : h->eng.bwd.size());     // ... of the backward sweep the handle runs (Jordan rows or plain)
    return 0;
}

int jg_nr_set_injection(jg_nr* h, const double* p, const double* q, int64_t stride) {
    if (!h || !p || !q || stride < 0) return fail(1, "jg_nr_set_injection: bad argument");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    if (int rc = h->put_rows(h->d_p, p, stride, h->n)) return rc;
    if (int rc = h->put_rows(h->d_q, q, stride, h->n)) return rc;
    h->jac_valid = false;
    h->inj_checked = false;                                      // compared with the base's again before the next compensated start
    return 0;
}

int jg_nr_set_voltage(jg_nr* h, const double* vm, const double* va, int64_t stride) {
    if (!h || !vm || !va || stride < 0) return fail(1, "jg_nr_set_voltage: bad argument");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    if (int rc = h->put_rows(h->d_vm, vm, stride, h->n)) return rc;
    if (int rc = h->put_rows(h->d_va, va, stride, h->n)) return rc;
    h->jac_valid = false;
    h->start_is_base = false;
    return 0;
}

int jg_nr_get_voltage(jg_nr* h, double* vm, double* va) {
    if (!h || !vm || !va) return fail(1, "jg_nr_get_voltage: bad argument");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    if (int rc = h->get_rows(h->d_vm, vm, h->n)) return rc;
    return h->get_rows(h->d_va, va, h->n);
}

int jg_nr_snapshot_voltage(jg_nr* h) {
    if (!h) return fail(1, "jg_nr_snapshot_voltage: bad argument");
    if (int rc = set_device(h)) return rc;
    return h->snapshot(h->d_vm, h->d_va, &h->d_vm0, &h->d_va0, h->n);
}

int jg_nr_restore_voltage(jg_nr* h) {
    if (!h || !h->d_vm0) return fail(1, "jg_nr_restore_voltage: no snapshot");
    if (int rc = set_device(h)) return rc;
    h->jac_valid = false;
    h->start_is_base = false;
    return h->restore(h->d_vm, h->d_va, h->d_vm0, h->d_va0, h->n);
}

int jg_nr_get_voltage_device(jg_nr* h, double* vm_dev, double* va_dev) {
    if (!h || !vm_dev || !va_dev) return fail(1, "jg_nr_get_voltage_device: bad argument");
    if (int rc = set_device(h)) return rc;
    h->collect(h->d_vm, vm_dev, h->n);
    h->collect(h->d_va, va_dev, h->n);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int jg_nr_pack_results_device(jg_nr* h, double* dst_dev) {
    if (!h || !dst_dev) return fail(1, "jg_nr_pack_results_device: bad argument");
    if (int rc = set_device(h)) return rc;
    const long long stride = 2LL * h->n + 2;
    h->collect2(h->d_vm, h->d_va, dst_dev, h->n, stride);
    h->pack_tail(h->d_iters, h->d_status, nullptr, dst_dev, stride, 2 * h->n);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int jg_nr_allgather_results(jg_nr* h, jg_comm* c, double* dst_dev) {
    if (!h || !c || !dst_dev) return fail(1, "jg_nr_allgather_results: bad argument");
    if (jg::comm_device(c) != h->device) return fail(1, "jg_nr_allgather_results: communicator and handle live on different devices");
    if (int rc = set_device(h)) return rc;
    const long long stride = 2LL * h->n + 2;
    const size_t count = (size_t)h->batch * stride;
    double* mine = dst_dev + (size_t)jg::comm_rank(c) * count;   // in-place all-gather: this rank's record sits in its own block
    h->collect2(h->d_vm, h->d_va, mine, h->n, stride);
    h->pack_tail(h->d_iters, h->d_status, nullptr, mine, stride, 2 * h->n);
    NR_HIP(hipGetLastError());
    if (int rc = jg::comm_allgather(c, mine, dst_dev, count, h->stream)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int jg_nr_patch_ybus(jg_nr* h, int64_t scenario, int64_t k, const int64_t* ptr, const double* dy) {
    if (!h || scenario < 0 || scenario >= h->batch || k < 0 || k > h->mp || (k > 0 && (!ptr || !dy)))
        return fail(1, "jg_nr_patch_ybus: bad argument (scenario / entry count beyond max_patch)");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    int allpos[8];
    for (int m = 0; m < 8; ++m) allpos[m] = -1;
    for (int m = 0; m < h->mp; ++m) {
        int pos = -1; double g = 0.0, b = 0.0;
        if (m < k) {
            if (ptr[m] < 1 || ptr[m] > h->nnz) return fail(1, "jg_nr_patch_ybus: pointer out of range");
            pos = h->tperm[ptr[m] - 1]; g = dy[2 * m]; b = dy[2 * m + 1];
            for (int mm = 0; mm < m; ++mm) if (ptr[mm] == ptr[m]) return fail(1, "jg_nr_patch_ybus: duplicate pointer");
        }
        allpos[m] = pos;
        const size_t off = (size_t)m * h->ld + scenario;
        NR_HIP(jg::sync_copy(h->d_ppos + off, &pos, sizeof(int), hipMemcpyHostToDevice, h->stream));
        NR_HIP(jg::sync_copy(h->d_pdg + off, &g, sizeof(double), hipMemcpyHostToDevice, h->stream));
        NR_HIP(jg::sync_copy(h->d_pdb + off, &b, sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    h->patch_state[(size_t)scenario] = classify_patch(h, allpos, h->mp);
    h->jac_valid = false;
    return 0;
}

int jg_nr_patch_ybus_batch(jg_nr* h, int64_t scenario0, int64_t count, int64_t k, const int64_t* ptr, const double* dy) {
    if (!h || scenario0 < 0 || count < 1 || scenario0 + count > h->batch || k < 0 || k > h->mp || (k > 0 && (!ptr || !dy)))
        return fail(1, "jg_nr_patch_ybus_batch: bad argument (scenario range / entry count beyond max_patch)");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    // A whole batch (what a screen uploads per job): the three slot arrays travel as ONE copy each -- [mp][ld] is contiguous -- instead of 3 x mp
    // copies with a stream synchronisation apiece (a job of the pipeline pays this inside the timed region)
    const bool whole = scenario0 == 0 && count == h->batch;
    const size_t wld = whole ? (size_t)h->ld : (size_t)count;
    std::vector<int> pos((size_t)h->mp * wld, -1), allpos((size_t)count * 8, -1);
    std::vector<double> g((size_t)h->mp * wld, 0.0), b((size_t)h->mp * wld, 0.0);
    for (int m = 0; m < h->mp; ++m) {
        int* pm = pos.data() + (size_t)m * wld; double* gm = g.data() + (size_t)m * wld; double* bm = b.data() + (size_t)m * wld;
        for (int64_t s = 0; s < count; ++s) {
            if (m < k && ptr[s * k + m] != 0) {
                const int64_t p = ptr[s * k + m];
                if (p < 1 || p > h->nnz) return fail(1, "jg_nr_patch_ybus_batch: pointer out of range");
                for (int mm = 0; mm < m; ++mm) if (ptr[s * k + mm] == p) return fail(1, "jg_nr_patch_ybus_batch: duplicate pointer");
                pm[s] = h->tperm[p - 1]; gm[s] = dy[2 * (s * k + m)]; bm[s] = dy[2 * (s * k + m) + 1];
            }
            allpos[(size_t)s * 8 + m] = pm[s];
        }
    }
    if (whole) {
        NR_HIP(hipMemcpyAsync(h->d_ppos, pos.data(), pos.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        NR_HIP(hipMemcpyAsync(h->d_pdg, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        NR_HIP(hipMemcpyAsync(h->d_pdb, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        NR_HIP(hipStreamSynchronize(h->stream));
    } else
    for (int m = 0; m < h->mp; ++m) {
        const size_t off = (size_t)m * h->ld + scenario0;
        NR_HIP(jg::sync_copy(h->d_ppos + off, pos.data() + (size_t)m * wld, (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
        NR_HIP(jg::sync_copy(h->d_pdg + off, g.data() + (size_t)m * wld, (size_t)count * sizeof(double), hipMemcpyHostToDevice, h->stream));
        NR_HIP(jg::sync_copy(h->d_pdb + off, b.data() + (size_t)m * wld, (size_t)count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    for (int64_t s = 0; s < count; ++s) h->patch_state[(size_t)(scenario0 + s)] = classify_patch(h, &allpos[(size_t)s * 8], h->mp);
    h->jac_valid = false;
    return 0;
}

int jg_nr_set_ybus(jg_nr* h, const double* y_reim, const double* yt_reim) {
    if (!h || !y_reim || !yt_reim) return fail(1, "jg_nr_set_ybus: bad argument");
    if (int rc = set_device(h)) return rc;
    std::vector<double> G(h->nnz), B(h->nnz);
    for (int p = 0; p < h->nnz; ++p) {
        G[p] = yt_reim[2 * p]; B[p] = yt_reim[2 * p + 1];
        if (y_reim[2 * (size_t)h->tperm[p]] != G[p] || y_reim[2 * (size_t)h->tperm[p] + 1] != B[p])
            return fail(4, "jg_nr_set_ybus: nodalMatrix and nodalMatrixTranspose disagree (stale model)");
    }
    NR_HIP(hipStreamSynchronize(h->stream));
    std::vector<double2> GBv(h->nnz);
    for (int p = 0; p < h->nnz; ++p) GBv[p] = double2{G[p], B[p]};
    NR_HIP(jg::sync_copy(h->d_GB, GBv.data(), GBv.size() * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    h->jac_valid = false;
    detach_base(h);                                              // an attached base was factorised for the old nodal matrix
    return 0;
}

int jg_nr_mismatch(jg_nr* h, double* max_p, double* max_q) {
    if (!h) return fail(1, "jg_nr_mismatch: bad argument");
    if (h->fast) return fail(1, "jg_nr_mismatch: this handle runs fast Newton-Raphson (its factor storage holds B', B''); use jg_nr_fast_mismatch");
    if (int rc = set_device(h)) return rc;
    launch_assemble(h);
    launch_check(h, 0);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    h->jac_valid = true;
    h->f_stale = false;
    if (max_p) NR_HIP(jg::sync_copy(max_p, h->d_normp, (size_t)h->batch * 8, hipMemcpyDeviceToHost, h->stream));
    if (max_q) NR_HIP(jg::sync_copy(max_q, h->d_normq, (size_t)h->batch * 8, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

int jg_nr_solve(jg_nr* h) {
    if (!h) return fail(1, "jg_nr_solve: bad argument");
    if (h->fast) return fail(1, "jg_nr_solve: this handle runs fast Newton-Raphson; use jg_nr_fast_solve");
    if (int rc = set_device(h)) return rc;
    if (!h->jac_valid) launch_assemble(h);
    h->start_is_base = false;
    h->f_stale = false;                                          // method.mismatch = the mismatch this step started from, for every scenario
    NR_HIP(hipMemsetAsync(h->eng.status, 0, (size_t)h->ld * 4, h->stream));
    if (int rc = newton_step(h, jg::GroupSel{}, nullptr)) return fail(rc, h->eng.error);
    if (h->keep_inc) h->inc_fresh = true;
    h->add_iter(h->d_iters);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    h->jac_valid = false;
    std::vector<int> st(h->ld);
    NR_HIP(jg::sync_copy(st.data(), h->eng.status, (size_t)h->ld * 4, hipMemcpyDeviceToHost, h->stream));
    for (int b = 0; b < h->batch; ++b) if (st[b] & 4) return fail(3, "jg_nr_solve: zero or non-finite pivot (singular Jacobian)");
    return 0;
}

int jg_nr_set_refine(jg_nr* h, int mode) {
    if (!h || mode < 0 || mode > 1) return fail(1, "jg_nr_set_refine: bad argument");
    if (h->fast) return fail(1, "jg_nr_set_refine: fast Newton-Raphson solves with constant matrices");
    if (mode && !h->keep_inc && h->paused) return fail(1, "jg_nr_set_refine: the handle is paused (jg_nr_run_defer) and keeps no increment (jg_nr_set_keep_increment); finish it first");
    if (mode && h->lt_on) return fail(1, "jg_nr_set_refine: scenarios have bus types of their own (jg_nr_set_bus_type / jg_nr_reactive_limit); the refinement residual reads the create-time types");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    if (mode && !h->d_R) {
        for (double** p : {&h->d_R, &h->d_inc2[0], &h->d_inc2[1]}) NR_HIP(h->alloc(p, (size_t)h->n * 2 * h->ld, true));
    }
    if ((mode != 0) != h->refine) {                              // the iteration graph is captured for one mode
        drop_iteration_graphs(h);
    }
    if (mode && !h->keep_inc) {                                  // k_refine_apply writes method.increment: a refining handle keeps it
        if (int rc = jg_nr_set_keep_increment(h, 1)) return rc;
    }
    h->refine = mode != 0;
    // a refined step runs forward() + backsolve() on the factor of the step: plain rows (Engine::jordan); back on when refinement goes off
    h->eng.jordan = !h->refine && h->eng.plan->S.jordan && jg::knob("JORDAN", 1) != 0;
    return 0;
}

int jg_nr_set_keep_increment(jg_nr* h, int mode) {
    if (!h || mode < 0 || mode > 1) return fail(1, "jg_nr_set_keep_increment: bad argument");
    if (mode == 0 && h->refine) return fail(1, "jg_nr_set_keep_increment: iterative refinement (jg_nr_set_refine) writes the increment; switch it off first");
    if (h->paused) return fail(1, "jg_nr_set_keep_increment: the handle is paused (jg_nr_run_defer); finish it first");
    if ((mode != 0) == h->keep_inc) return 0;
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    drop_iteration_graphs(h);                                    // the sweeps' `out` and the row set of the lane moves are captured
    drop_comp_graphs(h);
    if (mode) NR_HIP(jg::sync_fill(h->d_inc, 0, (size_t)h->n * 2 * h->ld * 8, h->stream));   // as a new handle's: nothing a run before the switch left
    h->keep_inc = mode != 0;
    h->inc_fresh = false;                                        // until the next run (jg_nr_get_increment never returns an older run's values)
    return 0;
}

int jg_nr_set_shared(jg_nr* h, int mode) {
    if (!h || mode < 0 || mode > 1) return fail(1, "jg_nr_set_shared: bad argument");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    if ((mode != 0) != h->eng.shared) {                          // the iteration graph holds the launches of the other choice
        drop_iteration_graphs(h);
    }
    h->eng.shared = mode != 0;
    return 0;
}

namespace {

// Start of a batched solve: every real scenario active, lanes in home order, all groups in use.  keep_iters: the lanes carry
// their iteration counts (a pool of moved scenarios, jg_nr_resume).
// ONE launch (round 6): until then three values, two fills and five small arrays went to the device through eight stream operations and a synchronise --
// ~90 us on the host's side of every solve, 7 % of a single instance's.
int run_setup(jg_nr* h, int64_t max_iter, double tol, int lanes, bool keep_iters, int defer_at = 0) {
    if (int rc = build_graphs(h)) return rc;
    if (h->keep_inc) h->inc_fresh = true;
    h->cmp.run_setup(h->stream, tol, (double)max_iter, (double)defer_at, lanes, keep_iters);      // defer_at: see jg::CompactArgs
    NR_HIP(hipGetLastError());
    h->res_pinned = h->ld == 64;
    return 0;
}

// The iteration loop: one graph per iteration until no scenario is active (the iteration limit itself is kept on the device,
// k_check) -- or, defer_at > 0, until at most defer_at (<= 64) scenarios are: they stay in their lanes, listed for the hand-off (k_compact: hold).
int run_loop(jg_nr* h, int64_t max_iter, int defer_at) {
    const bool trace = jg::knob_set("TRACE");
    auto now_us = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    for (int64_t it = h->iter_graphs; it <= max_iter && *h->h_counter != 0; ++it) {
        if (defer_at > 0 && *h->h_counter <= defer_at) break;
        h->iter_graphs += 1;
        // The iteration after which this handle's LAST run stopped is expected to end this one too (the batches of a screen behave alike): its verdict comes from a
        // mismatch-only pass (graph Bm, build_graphs).  A wrong guess costs one more launch -- the Jacobian alone (graph J) -- before the next iteration.
        const bool guess_last = h->stop_hint > 0 && h->iter_graphs == h->stop_hint;
        const double tc = now_us();
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (trace) { hipEventCreate(&e0); hipEventCreate(&e1); hipEventRecord(e0, h->stream); }
        if (!trace) h->arm();
        NR_HIP((guess_last ? h->gBm : h->gB).launch(h->stream));  // solve!, then mismatch! and the verdict on the new state
        const double tl = now_us();
        if (trace) hipEventRecord(e1, h->stream);
        NR_HIP(trace ? hipStreamSynchronize(h->stream) : h->wait());
        h->host_launch_us += tl - tc; h->host_wait_us += now_us() - tl; h->host_iters += 1;     // JG_HOST_TIMING: printed when the handle goes
        if (guess_last) {
            const bool stops = *h->h_counter == 0 || (defer_at > 0 && *h->h_counter <= defer_at) || it + 1 > max_iter;
            if (stops) h->last_guess_hit += 1;
            else { h->last_guess_miss += 1; NR_HIP(h->gJ.launch(h->stream)); }     // the scenarios that go on need their Jacobian after all
        }
        if (trace) {
            float ms = 0.f; hipEventElapsedTime(&ms, e0, e1); fprintf(stderr, "[jg_nr_run] graph on the device: %.1f us\n", 1e3 * ms); hipEventDestroy(e0); hipEventDestroy(e1);
            int cf[4];
            jg::sync_copy(cf, h->d_cflags, sizeof(cf), hipMemcpyDeviceToHost, h->stream);
            fprintf(stderr, "[jg_nr_run] iteration %lld: %.1f us, %d scenarios still active, %d of %d lane groups in use%s%s\n", (long long)it + 1,
                    now_us() - tc, *h->h_counter, cf[jg::CF_GROUPS], h->ld / 64, cf[jg::CF_PERMUTE] ? " (compacted)" : "", guess_last ? " (verdict without a Jacobian)" : "");
        }
    }
    h->stop_hint = h->iter_graphs;
    return 0;
}

// The verdict on the start point and -- when every scenario starts from the attached base case (comp_ready) -- the first iteration on the base's
// shared factor instead of a batched refactorisation (jg_comp.hpp).  The loop (run_loop) continues with refactorising iterations either way.
int run_start(jg_nr* h, int64_t max_iter) {
    bool comp = false;
    if (int rc = comp_ready(h, comp)) return rc;
    h->start_is_base = false;                                                  // whatever follows moves the state
    h->iter_graphs = 0;
    h->arm();
    NR_HIP((comp ? h->gA2 : h->gA).launch(h->stream));
    NR_HIP(h->wait());
    if (!comp) { h->first_full += 1; return 0; }
    h->first_comp += 1;
    if (max_iter < 1 || *h->h_counter == 0) {                                  // nothing to iterate: the Jacobian getters find no assembly in place
        h->jac_valid = false;
        return 0;
    }
    const bool trace = jg::knob_set("TRACE");
    const double t0 = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    h->arm();
    NR_HIP(h->gC.launch(h->stream));
    NR_HIP(h->wait());
    h->iter_graphs = 1;
    if (trace) fprintf(stderr, "[jg_nr_run] iteration 1 on the shared base factor: %.1f us, %d scenarios still active\n",
                       std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0, *h->h_counter);
    return 0;
}

// ONE scenario whose last run iterated: start verdict + that many iterations as one graph (build_whole_graph).  -1: the handle does not qualify (run_start / run_loop).
int run_whole(jg_nr* h, int64_t max_iter) {
    const bool on = jg::knob("SINGLE", 1) == 1 && h->eng.single_bwd;   // (the handle was created as a single instance: JG_SINGLE at its creation)
    const int k = h->stop_hint;
    if (!on || h->ld != 64 || h->batch != 1 || k < 1 || k > 12 || (int64_t)k > max_iter || h->refine || jg::knob_set("TRACE") || jg::knob_set("HOST_TIMING")) return -1;
    bool comp = false;
    if (int rc = comp_ready(h, comp)) return rc;
    if (comp) return -1;                                         // a base case is attached: the compensated start (run_start)
    if (int rc = build_whole_graph(h, k)) return rc;
    h->start_is_base = false;
    h->first_full += 1;
    h->arm();
    NR_HIP(h->gM.launch(h->stream));
    NR_HIP(h->wait(true));
    h->iter_graphs = k;
    if (*h->h_counter != 0) {                                    // more iterations than the last run took: the Jacobian of the new state, then the loop
        h->last_guess_miss += 1;
        NR_HIP(h->gJ.launch(h->stream));
        return run_loop(h, max_iter, 0);
    }
    h->last_guess_hit += 1;
    h->stop_hint = std::max(1, (int)h->h_counter[1]);            // the iterations this solve took (pinned: k_verdict64) -- fewer than k: the next solve's graph shrinks
    return 0;
}

// End of a batched solve: lanes back to their home order, method.mismatch of every scenario at its final state, outputs.
int run_finish(jg_nr* h, int32_t* iters, int32_t* status) {
    if (h->ld == 64 && *h->h_counter == 0 && h->res_pinned) {                  // one lane group, every scenario finished: the last verdict (k_compact) has left iterations
        h->f_stale = false;                                                    // and status in pinned host memory, the lanes never left their home order, and what
        h->jac_valid = false;                                                  // k_compact's restore pass resets is rewritten by the next run_setup: no launch, no
        h->paused = false;                                                     // blocking copies (the stream orders whatever follows behind the last graph)
        h->res_pinned = false;
        if (iters) std::memcpy(iters, h->h_counter + 1, (size_t)h->batch * 4);
        if (status) std::memcpy(status, h->h_counter + 65, (size_t)h->batch * 4);
        return 0;
    }
    launch_compact(h, 1);                                                      // lanes back to their home order
    h->f_stale = h->ld > 64;                                                   // method.mismatch of every scenario at its final state: groups that dropped
                                                                               // out early hold other scenarios' rows after a compaction -- one mismatch-only
                                                                               // pass, run when jg_nr_get_mismatch asks for it (0.1 ms per batch of 512)
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    h->jac_valid = false;
    h->paused = false;
    if (iters) NR_HIP(jg::sync_copy(iters, h->d_iters, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
    if (status) NR_HIP(jg::sync_copy(status, h->d_status, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace


// ---- first iteration of a common-start batch on ONE shared factor (jg_comp.hpp) -------------------------------------------------------
__global__ void k_lane0(const double* src, double* dst, int n, int ld, int elem) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < elem; ++c) dst[(size_t)i * elem + c] = src[((size_t)i * ld) * elem + c];
}
__global__ void k_broadcast(const double* src, double* dst, int n, int ld) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (b < ld) dst[(size_t)i * ld + b] = src[i];
}

int jg_nr_base_create(jg_nr_base** out, jg_nr* s, int64_t top_cap) {
    if (!out || !s) return fail(1, "jg_nr_base_create: bad argument");
    if (s->fast || s->refine) return fail(1, "jg_nr_base_create: the single-instance handle must run plain Newton-Raphson");
    if (s->batch != 1) return fail(1, "jg_nr_base_create: pass a single-instance handle (batch = 1) that holds the base case's grid, injections and start state");
    if (int rc = set_device(s)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    NR_HIP(hipStreamSynchronize(s->stream));
    // ONE factorisation of the Jacobian at the start state, plain rows (the compact factor is read from the entries), and y0 = J_0^-1 f_0
    const bool jordan = s->eng.jordan;
    s->eng.jordan = false;
    NR_HIP(hipMemsetAsync(s->eng.status, 0, (size_t)s->ld * 4, s->stream));
    launch_assemble(s, jg::GroupSel{}, true, nullptr, 0, nullptr, true);
    int rc = s->eng.factor(s->stream, nullptr, s->d_F, jg::GroupSel{}, s->level0_done);
    if (!rc) rc = s->eng.backsolve(s->stream, s->d_inc, jg::StateUpdate{}, jg::GroupSel{});
    s->eng.jordan = jordan;
    s->jac_valid = false;
    if (rc) return fail(rc, s->eng.error);
    NR_HIP(hipStreamSynchronize(s->stream));
    int st0 = 0;
    NR_HIP(jg::sync_copy(&st0, s->eng.status, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    if (st0 & 4) return fail(3, "jg_nr_base_create: zero or non-finite pivot (the Jacobian of the base case is singular)");
    jg_nr_base* b = new jg_nr_base();
    b->n = s->n; b->nnz = s->nnz; b->device = s->device;
    b->colptr = s->colptr; b->rowval = s->rowval; b->type = s->type;
    jg::CompBase& cb = b->cb;
    cb.nnz = s->nnz;
    auto bail = [&](int code, const std::string& m) { release_base(b); return fail(code, m); };
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) return bail(2, "jg_nr_base_create: stream creation failed");
    const int n = s->n, nnz = s->nnz;
    std::string err;
    {   // the Ybus pattern as the correction kernel reads it: row of a position, position of the transposed entry
        std::vector<int> rp(n + 1), tp(nnz, -1);
        for (int i = 0; i <= n; ++i) rp[i] = (int)(s->colptr[i] - 1);
        for (int p = 0; p < nnz; ++p) {
            const int i = s->csr_row[p], j = s->csr_col[p];
            const int* lo = s->csr_col.data() + rp[j]; const int* hi = s->csr_col.data() + rp[j + 1];
            const int* q = std::lower_bound(lo, hi, i);
            tp[p] = (int)(q - s->csr_col.data());
        }
        if (jg::upload(&cb.rowptr, rp, err, b->stream) || jg::upload(&cb.posrow, s->csr_row, err, b->stream) || jg::upload(&cb.tpos, tp, err, b->stream)) return bail(2, err);
        hipError_t e = hipMalloc((void**)&cb.colm, (size_t)nnz * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void**)&cb.rowtype, (size_t)n * sizeof(int));
        if (e == hipSuccess) e = jg::sync_copy(cb.colm, s->d_col, (size_t)nnz * sizeof(int), hipMemcpyDeviceToDevice, b->stream);
        if (e == hipSuccess) e = jg::sync_copy(cb.rowtype, s->d_rowtype, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, b->stream);
        for (double** q : {&cb.v0, &cb.th0, &cb.p0, &cb.q0}) if (e == hipSuccess) e = hipMalloc((void**)q, (size_t)n * sizeof(double));
        for (double** q : {&cb.f0, &cb.y0}) if (e == hipSuccess) e = hipMalloc((void**)q, (size_t)n * 2 * sizeof(double));
        if (e != hipSuccess) return bail(2, std::string("jg_nr_base_create: ") + hipGetErrorString(e));
        const dim3 g((n + 255) / 256), t(256);
        hipLaunchKernelGGL(k_lane0, g, t, 0, b->stream, (const double*)s->d_vm, cb.v0, n, s->ld, 1);
        hipLaunchKernelGGL(k_lane0, g, t, 0, b->stream, (const double*)s->d_va, cb.th0, n, s->ld, 1);
        hipLaunchKernelGGL(k_lane0, g, t, 0, b->stream, (const double*)s->d_p, cb.p0, n, s->ld, 1);
        hipLaunchKernelGGL(k_lane0, g, t, 0, b->stream, (const double*)s->d_q, cb.q0, n, s->ld, 1);
        hipLaunchKernelGGL(k_lane0, g, t, 0, b->stream, (const double*)s->d_F, cb.f0, n, s->ld, 2);
        hipLaunchKernelGGL(k_lane0, g, t, 0, b->stream, (const double*)s->d_inc, cb.y0, n, s->ld, 2);
        if (hipStreamSynchronize(b->stream) != hipSuccess) return bail(2, "jg_nr_base_create: copy of the base state failed");
    }
    // default top: what keeps the dense product near the cost of the level launches it replaces (10 000-bus grid: 502 pivots = the levels above the 11th)
    const int cap = top_cap < 0 ? -1 : (top_cap == 0 ? 512 : (int)std::min<int64_t>(top_cap, 4096));
    if (int rc2 = cb.create(s->eng.plan->S, s->eng.X, s->eng.ld, cap, b->stream)) return bail(rc2, "jg_nr_base_create: " + cb.error);
    if (int rc2 = jg::comp_form_z(cb, b->stream)) return bail(rc2, "jg_nr_base_create: " + cb.error);
    b->create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = b;
    return 0;
}

void jg_nr_base_destroy(jg_nr_base* b) { release_base(b); }

int jg_nr_base_info(jg_nr_base* b, int64_t* info) {
    if (!b || !info) return fail(1, "jg_nr_base_info: bad argument");
    const jg::CompBase& cb = b->cb;
    info[0] = cb.split.T.n_top; info[1] = cb.split.T.split; info[2] = (int64_t)cb.split.fwd.size(); info[3] = (int64_t)cb.split.bwd.size();
    info[4] = (int64_t)cb.full.fwd.size(); info[5] = (int64_t)cb.full.bwd.size(); info[6] = (int64_t)(b->create_ms * 1000.0); info[7] = b->refs.load() - 1;
    return 0;
}

int jg_nr_base_get(jg_nr_base* b, int which, double* out, int64_t cap) {
    if (!b || !out) return fail(1, "jg_nr_base_get: bad argument");
    const jg::CompBase& cb = b->cb;
    const double* src = nullptr; size_t count = 0;
    switch (which) {
        case 0: src = cb.Zc; count = (size_t)cb.nnz * 4; break;                                  // J_0^-1 on the Ybus pattern, row-CSR order
        case 1: src = cb.y0; count = (size_t)cb.n * 2; break;
        case 2: src = cb.f0; count = (size_t)cb.n * 2; break;
        case 3: src = cb.Sinv; count = cb.Sinv ? (size_t)((2 * cb.split.T.n_top + 15) / 16) * cb.lds * 64 : 0; break;   // MFMA fragment order (jg_comp.hip: k_ctop)
        case 4: src = cb.Mc; count = (size_t)cb.n_entries * 4; break;
        default: return fail(1, "jg_nr_base_get: which = 0 (inverse on the pattern) | 1 (J0^-1 f0) | 2 (f0) | 3 (dense top inverse) | 4 (compact factor)");
    }
    if ((int64_t)count > cap) return fail(1, "jg_nr_base_get: buffer too small");
    NR_HIP(hipSetDevice(b->device));
    if (count) NR_HIP(jg::sync_copy(out, src, count * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    return 0;
}

int jg_nr_attach_base(jg_nr* h, jg_nr_base* b) {
    if (!h) return fail(1, "jg_nr_attach_base: bad argument");
    if (int rc = set_device(h)) return rc;
    detach_base(h);
    if (!b) return 0;
    if (h->fast) return fail(1, "jg_nr_attach_base: fast Newton-Raphson factorises constant matrices once anyway");
    if (b->device != h->device || b->n != h->n || b->nnz != h->nnz || b->colptr != h->colptr || b->rowval != h->rowval || b->type != h->type)
        return fail(1, "jg_nr_attach_base: the base was built for another grid (pattern, bus types) or device");
    NR_HIP(h->alloc(&h->d_cw, b->cb.scratch_rows(b->cb.split) * (size_t)h->ld * 2, true));
    if (!h->d_cmp) NR_HIP(h->alloc(&h->d_cmp, 1));
    b->refs.fetch_add(1);
    h->base = b;
    h->inj_checked = false;
    return 0;
}

int jg_nr_start_from_base(jg_nr* h) {
    if (!h || !h->base) return fail(1, "jg_nr_start_from_base: no base attached (jg_nr_attach_base)");
    if (int rc = set_device(h)) return rc;
    const dim3 g((h->ld + 255) / 256, h->n), t(256);
    hipLaunchKernelGGL(k_broadcast, g, t, 0, h->stream, (const double*)h->base->cb.v0, h->d_vm, h->n, h->ld);
    hipLaunchKernelGGL(k_broadcast, g, t, 0, h->stream, (const double*)h->base->cb.th0, h->d_va, h->n, h->ld);
    NR_HIP(hipGetLastError());
    h->jac_valid = false;
    h->start_is_base = true;
    return 0;
}

int jg_nr_set_first_iteration(jg_nr* h, int mode) {
    if (!h || mode < 0 || mode > 1) return fail(1, "jg_nr_set_first_iteration: mode = 0 (always refactorise) | 1 (shared base factor when the conditions hold)");
    h->first_mode = mode;
    return 0;
}

int jg_nr_first_iteration_counts(jg_nr* h, int64_t* compensated, int64_t* refactorised) {
    if (!h) return fail(1, "jg_nr_first_iteration_counts: bad argument");
    if (compensated) *compensated = h->first_comp;
    if (refactorised) *refactorised = h->first_full;
    return 0;
}

int jg_nr_run(jg_nr* h, int64_t max_iter, double tol, int32_t* iters, int32_t* status) {
    if (!h || max_iter < 0 || !(tol > 0.0)) return fail(1, "jg_nr_run: bad argument");
    if (h->fast) return fail(1, "jg_nr_run: this handle runs fast Newton-Raphson; use jg_nr_fast_run");
    if (int rc = set_device(h)) return rc;
    if (int rc = run_setup(h, max_iter, tol, h->batch, false)) return rc;
    const int rw = run_whole(h, max_iter);                                     // ONE scenario that has solved before: the whole solve as one graph; -1: not such a handle
    if (rw > 0) return rw;
    if (rw < 0) {
        if (int rc = run_start(h, max_iter)) return rc;                        // acPowerFlow.jl:1406: mismatch!, verdict (+ a compensated first iteration)
        if (int rc = run_loop(h, max_iter, 0)) return rc;
    }
    if (int rc = run_finish(h, iters, status)) return rc;
    return mark_dead(h, status);
}

int jg_nr_run_defer(jg_nr* h, int64_t max_iter, double tol, int64_t defer_at, int32_t* n_left) {
    if (!h || max_iter < 0 || !(tol > 0.0) || defer_at < 0 || defer_at > 64 || !n_left) return fail(1, "jg_nr_run_defer: bad argument (defer_at in 0..64)");
    if (h->fast) return fail(1, "jg_nr_run_defer: this handle runs fast Newton-Raphson");
    if (int rc = set_device(h)) return rc;
    if (int rc = run_setup(h, max_iter, tol, h->batch, false, h->ld > 64 ? (int)defer_at : 0)) return rc;
    if (int rc = run_start(h, max_iter)) return rc;
    if (int rc = run_loop(h, max_iter, h->ld > 64 ? (int)defer_at : 0)) return rc;   // one lane group: lanes are never packed, nothing to hand off
    *n_left = *h->h_counter;
    h->paused = true;
    return 0;
}

int jg_nr_finish(jg_nr* h, int32_t* iters, int32_t* status) {
    if (!h || !h->paused) return fail(1, "jg_nr_finish: the handle is not paused (jg_nr_run_defer)");
    if (int rc = set_device(h)) return rc;
    if (int rc = run_finish(h, iters, status)) return rc;
    return mark_dead(h, status);
}

int jg_nr_move_lanes(jg_nr* dst, int64_t dst_lane0, jg_nr* src, int32_t* home, int32_t* count) {
    if (!dst || !src || dst == src || !home || !count || dst_lane0 < 0) return fail(1, "jg_nr_move_lanes: bad argument");
    if (src->lt_on || dst->lt_on) return fail(1, "jg_nr_move_lanes: scenarios with bus types of their own (jg_nr_set_bus_type / jg_nr_reactive_limit) do not move between handles");
    if (!src->paused) return fail(1, "jg_nr_move_lanes: the source is not paused (jg_nr_run_defer)");
    if (dst->device != src->device || dst->n != src->n || dst->nnz != src->nnz || dst->mp != src->mp || dst->fast || src->fast)
        return fail(1, "jg_nr_move_lanes: the two handles must hold the same grid on the same device");
    //  the factorisation plan -- where the top starts, front caps, tasks or wave records: the summation order -- is chosen by the class of
    // batch a handle was created for (Engine::create, by the lane count PADDED to a multiple of 64: 64 with at most 32 scenarios, 64, 128 / 192, 256 and more).  A straggler that finishes under another
    // plan is no longer bitwise the scenario of a lockstep batch, silently: refuse the hand-off instead.
    if (dst->eng.plan && src->eng.plan && dst->eng.plan->policy != src->eng.plan->policy)
        return fail(1, "jg_nr_move_lanes: the pool runs another factorisation plan than the batch (create both for the same class of batch: "
                       "1-32 scenarios, 33-64, 65-192, 193 and more = padded lane count 64 with at most 32 scenarios, 64, 128 / 192, 256 and more)");
    if (int rc = set_device(dst)) return rc;
    for (jg_nr* h : {dst, src})
        if (!h->d_move) {
            NR_HIP(h->alloc(&h->d_move, jg::MOVE_WORDS));
            NR_HIP(h->pin(&h->h_move, 65));
        }
    NR_HIP(hipStreamSynchronize(src->stream));
    src->cmp.launch_move_plan(dst->stream, dst->cmp, dst->d_move, (int)dst_lane0, dst->batch);
    std::vector<jg::LanePair> rows{{src->d_vm, dst->d_vm, src->n}, {src->d_va, dst->d_va, src->n}, {src->d_p, dst->d_p, src->n}, {src->d_q, dst->d_q, src->n}};
    if (src->mp > 0) { rows.push_back({src->d_pdg, dst->d_pdg, src->mp}); rows.push_back({src->d_pdb, dst->d_pdb, src->mp}); }
    src->cmp.launch_move_rows(dst->stream, dst->cmp, dst->d_move, rows);
    NR_HIP(hipGetLastError());
    NR_HIP(hipMemcpyAsync(dst->h_move, dst->d_move + jg::MOVE_HOME, 65 * sizeof(int), hipMemcpyDeviceToHost, dst->stream));
    NR_HIP(hipStreamSynchronize(dst->stream));
    const int c = dst->h_move[64];
    if (c < 0) return fail(1, "jg_nr_move_lanes: the destination has not enough free lanes");
    for (int i = 0; i < c; ++i) home[i] = dst->h_move[i];
    *count = c;
    *src->h_counter = 0;
    src->res_pinned = false;                                    // (the source's last verdict saw active scenarios: nothing stands behind its pinned word -- jg_nr_finish copies)
    dst->jac_valid = false;
    dst->start_is_base = false;                                 // its lanes hold the states of the moved scenarios, not the base's
    return 0;
}

int jg_nr_resume(jg_nr* h, int64_t lanes, int64_t max_iter, double tol, int32_t* iters, int32_t* status) {
    if (!h || lanes < 0 || lanes > h->batch || max_iter < 0 || !(tol > 0.0)) return fail(1, "jg_nr_resume: bad argument");
    if (h->fast) return fail(1, "jg_nr_resume: this handle runs fast Newton-Raphson");
    if (int rc = set_device(h)) return rc;
    // lanes [0, lanes) hold moved scenarios (active, their iteration counts with them); the others are idle
    if (int rc = run_setup(h, max_iter, tol, (int)lanes, true)) return rc;
    h->start_is_base = false;                                                  // the iterations below move the state
    if (lanes < h->ld) {
        NR_HIP(hipMemsetAsync(h->d_active + lanes, 0, (size_t)(h->ld - lanes) * 4, h->stream));
        NR_HIP(hipMemsetAsync(h->eng.status + lanes, 0, (size_t)(h->ld - lanes) * 4, h->stream));
        NR_HIP(hipMemsetD32Async((hipDeviceptr_t)(h->d_iters + lanes), (int)max_iter, (size_t)(h->ld - lanes), h->stream));   // idle lanes: at the limit, never picked up by a verdict
    }
    launch_compact(h, 0, true);                                                // groups in use (the lanes are already packed)
    launch_assemble(h, active_groups(h), true, nullptr, 0, nullptr, true);     // the Jacobian of the state they arrived with; NO verdict:
    NR_HIP(hipStreamSynchronize(h->stream));                                   // theirs was taken (and counted) where they came from
    h->iter_graphs = 0;
    if (int rc = run_loop(h, max_iter, 0)) return rc;
    h->paused = true;
    if (int rc = run_finish(h, nullptr, nullptr)) return rc;
    if (iters) NR_HIP(jg::sync_copy(iters, h->d_iters, (size_t)lanes * 4, hipMemcpyDeviceToHost, h->stream));
    if (status) NR_HIP(jg::sync_copy(status, h->d_status, (size_t)lanes * 4, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

int jg_nr_pack_rows_device(jg_nr* h, double* dst_dev, int64_t lane0, int64_t count, const int32_t* rows) {
    if (!h || !dst_dev || !rows || lane0 < 0 || count < 0 || lane0 + count > h->batch || count > h->ld) return fail(1, "jg_nr_pack_rows_device: bad argument");
    if (count == 0) return 0;
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipMemcpyAsync(h->d_itmp, rows, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)std::min((h->n + 255) / 256, 64), (unsigned)count), dim3(256), 0, h->stream,
                       h->d_vm, h->d_va, h->d_iters, h->d_status, h->d_itmp, dst_dev, h->n, h->ld, (int)lane0, 2LL * h->n + 2);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// device [n][ld][2] (per bus: the theta / P and the V / Q component) -> host [batch][dimJ] in the reference's order: the pvpq rows, then the pq rows
static int get_scattered(jg_nr* h, const double* src, double* out) {
    std::vector<double> t((size_t)h->n * 2 * h->batch);
    if (int rc = h->get_rows2(src, t.data(), h->n)) return rc;
    for (int b = 0; b < h->batch; ++b) {
        const double* s = t.data() + (size_t)b * h->n * 2;
        double* d = out + (size_t)b * h->dimJ;
        for (int i = 0; i < h->n; ++i) {
            if (h->pvpq[i]) d[h->pvpq[i] - 1] = s[2 * i];
            if (h->pq[i]) d[h->pq[i] - 1] = s[2 * i + 1];
        }
    }
    return 0;
}

int jg_nr_get_mismatch(jg_nr* h, double* mism) {
    if (!h || !mism) return fail(1, "jg_nr_get_mismatch: bad argument");
    if (h->lt_on) return fail(1, "jg_nr_get_mismatch: scenarios have bus types of their own; the reference layout depends on the types");
    if (int rc = set_device(h)) return rc;
    if (h->f_stale) { launch_assemble(h, jg::GroupSel{}, false); NR_HIP(hipGetLastError()); h->f_stale = false; }
    NR_HIP(hipStreamSynchronize(h->stream));
    return get_scattered(h, h->d_F, mism);
}

int jg_nr_get_increment(jg_nr* h, double* incr) {
    if (!h || !incr) return fail(1, "jg_nr_get_increment: bad argument");
    if (h->lt_on) return fail(1, "jg_nr_get_increment: scenarios have bus types of their own; the reference layout depends on the types");
    if (!h->keep_inc) return fail(1, "jg_nr_get_increment: this handle keeps no bus-order increment (jg_nr_set_keep_increment(h, 0)); switch it on and run again");
    if (!h->inc_fresh) return fail(1, "jg_nr_get_increment: jg_nr_set_keep_increment was switched on after the last run; the increment is there after the next one");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    return get_scattered(h, h->d_inc, incr);
}

int jg_nr_get_jacobian(jg_nr* h, double* nzval) {
    if (!h || !nzval) return fail(1, "jg_nr_get_jacobian: bad argument");
    if (h->lt_on) return fail(1, "jg_nr_get_jacobian: scenarios have bus types of their own; the reference layout depends on the types");
    if (h->fast) return fail(1, "jg_nr_get_jacobian: this handle runs fast Newton-Raphson: the factor storage holds the factorised B', B'', assembling the full Jacobian there would destroy them");
    if (int rc = set_device(h)) return rc;
    if (!h->jac_valid) { launch_assemble(h); h->jac_valid = true; }      // Jacobian at the current state
    NR_HIP(hipStreamSynchronize(h->stream));
    std::vector<double> t((size_t)h->eng.plan->S.n_entries * 4 * h->ld);     // the factor storage holds the Jacobian until the next factorisation
    NR_HIP(jg::sync_copy(t.data(), h->eng.X, t.size() * 8, hipMemcpyDeviceToHost, h->stream));
    for (int b = 0; b < h->batch; ++b)
        for (int64_t k = 0; k < h->nnzJ; ++k) nzval[(size_t)b * h->nnzJ + k] = t[(((size_t)(h->jmap[k] >> 2) * 2 + ((h->jmap[k] >> 1) & 1)) * h->ld + b) * 2 + (h->jmap[k] & 1)];
    return 0;
}

int jg_nr_get_maps(jg_nr* h, int64_t* pq, int64_t* pvpq, int64_t* pcount, int64_t* jcolptr, int64_t* jrowval) {
    if (!h) return fail(1, "jg_nr_get_maps: bad argument");
    if (h->lt_on) return fail(1, "jg_nr_get_maps: scenarios have bus types of their own; the reference layout depends on the types");
    if (pq) std::memcpy(pq, h->pq.data(), h->pq.size() * 8);
    if (pvpq) std::memcpy(pvpq, h->pvpq.data(), h->pvpq.size() * 8);
    if (pcount) std::memcpy(pcount, h->pcount.data(), h->pcount.size() * 8);
    if (jcolptr) std::memcpy(jcolptr, h->jcolptr.data(), h->jcolptr.size() * 8);
    if (jrowval) std::memcpy(jrowval, h->jrowval.data(), h->jrowval.size() * 8);
    return 0;
}

int jg_nr_get_iteration(jg_nr* h, int32_t* iters) {
    if (!h || !iters) return fail(1, "jg_nr_get_iteration: bad argument");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    NR_HIP(jg::sync_copy(iters, h->d_iters, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

// ---- fast decoupled Newton-Raphson (fastNewtonRaphsonBX / XB, acPowerFlow.jl:215-537, 687-730, 913-983) ---------------
constexpr int FAST_MP = 4;                            // edits per scenario: a branch touches (i,i), (j,j), (i,j), (j,i) of B' and of B''
// X[entry] += diag(dp, dq) for the scenario of the lane: the matrices of a batch differ from the shared ones in a handful of entries
__global__ void k_fast_patch(double* X, const int* entry, const double* dp, const double* dq, int ld, int batch) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (b >= batch) return;
    const int e = entry[(size_t)m * batch + b];
    if (e < 0) return;
    double* x = X + ((size_t)e * 2 * ld + b) * 2;                 // block row 0: (v00, v01); block row 1 sits ld * 2 doubles further
    x[0] += dp[(size_t)m * batch + b];
    x[(size_t)ld * 2 + 1] += dq[(size_t)m * batch + b];
}

// shared matrices + every scenario's edits into the factor storage, then ONE factorisation for the whole batch (fastNewtonRaphson factorises
// once per matrix, acPowerFlow.jl:923-927; after updateBranch! the reference calls lu! again, :476-537).  A scenario whose B' or B'' is singular
// (an islanding outage) keeps status bit 2 in eng.status: jg_nr_fast_run reports it as status 3, its neighbours are untouched.
static int fast_refactor(jg_nr* h) {
    if (int rc = h->eng.set_shared_matrix(h->stream, h->fast_blk.data())) return fail(rc, h->eng.error);
    bool any = false;
    for (int e : h->fp_entry) any = any || e >= 0;
    if (any) {
        //  the edit tables live in buffers of the handle: three hipMalloc / hipFree pairs per call were device-wide synchronisations that could stall
        // other pipeline threads in the middle of a graph capture
        const size_t cnt = h->fp_entry.size();
        if (!h->d_fp_entry) {
            NR_HIP(h->alloc(&h->d_fp_entry, cnt));
            NR_HIP(h->alloc(&h->d_fp_dp, cnt));
            NR_HIP(h->alloc(&h->d_fp_dq, cnt));
        }
        NR_HIP(hipMemcpyAsync(h->d_fp_entry, h->fp_entry.data(), cnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
        NR_HIP(hipMemcpyAsync(h->d_fp_dp, h->fp_dp.data(), cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
        NR_HIP(hipMemcpyAsync(h->d_fp_dq, h->fp_dq.data(), cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_fast_patch, dim3((h->batch + 255) / 256, FAST_MP), dim3(256), 0, h->stream, h->eng.X, (const int*)h->d_fp_entry, (const double*)h->d_fp_dp,
                           (const double*)h->d_fp_dq, h->ld, h->batch);
        NR_HIP(hipStreamSynchronize(h->stream));
    }
    NR_HIP(hipMemsetAsync(h->eng.status, 0, (size_t)h->ld * 4, h->stream));
    h->eng.jordan = false;                                       // factor once, then forward() + backsolve() per half iteration: plain rows
    if (int rc = h->eng.factor(h->stream, nullptr, h->d_R, jg::GroupSel{})) return fail(rc, h->eng.error);   // ONCE (lu(jacobian), utility.jl:470-476)
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

static int fast_half(jg_nr* h, int pass) {
    // pass 1: rhs = (f_P / V, 0) is already in d_R (written by the mismatch pass); pass 2: Q mismatches at the new angles first
    if (pass == 2) launch_assemble(h, jg::GroupSel{}, false, nullptr, 2);
    if (int rc = h->eng.forward(h->stream, h->d_R, jg::GroupSel{})) return fail(rc, h->eng.error);
    jg::StateUpdate upd{h->d_va, h->d_vm, h->d_flags, h->fast_mask, +1.0};            // theta += / V += (:946-950, 966-970)
    if (int rc = h->eng.backsolve(h->stream, h->d_inc2[pass - 1], upd, jg::GroupSel{})) return fail(rc, h->eng.error);
    return 0;
}

int jg_nr_fast_setup(jg_nr* h, const double* bp, const double* bq) {
    if (!h || !bp || !bq) return fail(1, "jg_nr_fast_setup: bad argument");
    if (h->lt_on) return fail(1, "jg_nr_fast_setup: scenarios have bus types of their own (jg_nr_set_bus_type); fast Newton-Raphson keeps the create-time types");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    // block (r, c) of the shared matrix = diag(B'[r,c], B''[r,c]); the caller pads slack / PV rows and columns with identity
    if (h->refine) return fail(1, "jg_nr_fast_setup: the handle is set up for refined full Newton-Raphson steps");
    h->fast_blk.assign((size_t)h->nnz * 4, 0.0);
    for (int p = 0; p < h->nnz; ++p) { h->fast_blk[(size_t)h->tperm[p] * 4] = bp[p]; h->fast_blk[(size_t)h->tperm[p] * 4 + 3] = bq[p]; }
    // (engine block q sits at row = the column that pointer q belongs to, col = rowval[q]; tperm[p of (r, c)] = pointer of (c, r))
    h->fp_entry.assign((size_t)FAST_MP * h->batch, -1); h->fp_dp.assign((size_t)FAST_MP * h->batch, 0.0); h->fp_dq.assign((size_t)FAST_MP * h->batch, 0.0);   // new matrices: no edits
    const size_t vec = (size_t)h->n * 2 * h->ld * 8;
    for (double** p : {&h->d_R, &h->d_inc2[0], &h->d_inc2[1]}) if (!*p) NR_HIP(h->alloc(p, vec / 8));
    NR_HIP(jg::sync_fill(h->d_R, 0, vec, h->stream));
    if (int rc = fast_refactor(h)) return rc;
    std::vector<int> st(h->ld);
    NR_HIP(jg::sync_copy(st.data(), h->eng.status, (size_t)h->ld * 4, hipMemcpyDeviceToHost, h->stream));
    for (int b = 0; b < h->batch; ++b) if (st[b] & 4) return fail(3, "jg_nr_fast_setup: zero or non-finite pivot (singular B matrix)");
    h->fast = true;
    h->jac_valid = false;
    return 0;
}

int jg_nr_fast_patch_batch(jg_nr* h, int64_t scenario0, int64_t count, int64_t k, const int64_t* ptr, const double* dbp, const double* dbq) {
    if (!h || !h->fast) return fail(1, "jg_nr_fast_patch_batch: call jg_nr_fast_setup first");
    if (scenario0 < 0 || count < 1 || scenario0 + count > h->batch || k < 0 || k > FAST_MP || (k > 0 && (!ptr || !dbp || !dbq)))
        return fail(1, "jg_nr_fast_patch_batch: bad argument (scenario range / more than 4 entries per scenario)");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    const jg::BlockSymbolic& S = h->eng.plan->S;
    for (int64_t sc = 0; sc < count; ++sc)                       // the whole call is checked before a single edit is recorded: a refused call changes nothing
        for (int64_t m = 0; m < k; ++m) {
            const int64_t p = ptr[sc * k + m];
            if (p == 0) continue;
            if (p < 1 || p > h->nnz) return fail(1, "jg_nr_fast_patch_batch: pointer out of range");
            for (int64_t mm = 0; mm < m; ++mm) if (ptr[sc * k + mm] == p) return fail(1, "jg_nr_fast_patch_batch: duplicate pointer");
        }
    for (int64_t sc = 0; sc < count; ++sc)
        for (int m = 0; m < FAST_MP; ++m) {
            const size_t at = (size_t)m * h->batch + scenario0 + sc;
            h->fp_entry[at] = -1; h->fp_dp[at] = 0.0; h->fp_dq[at] = 0.0;
            if (m >= k || ptr[sc * k + m] == 0) continue;
            const int64_t p = ptr[sc * k + m];
            h->fp_entry[at] = S.src_entry[h->tperm[p - 1]];
            h->fp_dp[at] = dbp[sc * k + m]; h->fp_dq[at] = dbq[sc * k + m];
        }
    return fast_refactor(h);
}

int jg_nr_fast_mismatch(jg_nr* h, double* max_p, double* max_q) {
    if (!h || !h->fast) return fail(1, "jg_nr_fast_mismatch: call jg_nr_fast_setup first");
    if (int rc = set_device(h)) return rc;
    launch_assemble(h, jg::GroupSel{}, false, nullptr, 1);
    launch_check(h, 0);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    if (max_p) NR_HIP(jg::sync_copy(max_p, h->d_normp, (size_t)h->batch * 8, hipMemcpyDeviceToHost, h->stream));
    if (max_q) NR_HIP(jg::sync_copy(max_q, h->d_normq, (size_t)h->batch * 8, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

int jg_nr_fast_solve(jg_nr* h) {
    if (!h || !h->fast) return fail(1, "jg_nr_fast_solve: call jg_nr_fast_setup first");
    if (int rc = set_device(h)) return rc;
    launch_assemble(h, jg::GroupSel{}, false, nullptr, 1);                      // solve! uses the mismatches of the current state
    h->fast_mask = nullptr;
    if (int rc = fast_half(h, 1)) return rc;
    if (int rc = fast_half(h, 2)) return rc;
    h->add_iter(h->d_iters);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int jg_nr_fast_get_increment(jg_nr* h, double* incr) {
    if (!h || !h->fast || !incr) return fail(1, "jg_nr_fast_get_increment: bad argument");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    std::vector<double> t0((size_t)h->n * 2 * h->batch), t1((size_t)h->n * 2 * h->batch);
    if (int rc = h->get_rows2(h->d_inc2[0], t0.data(), h->n)) return rc;
    if (int rc = h->get_rows2(h->d_inc2[1], t1.data(), h->n)) return rc;
    for (int b = 0; b < h->batch; ++b) {                          // [active.increment (pvpq order) | reactive.increment (pq order)]
        double* d = incr + (size_t)b * h->dimJ;
        for (int i = 0; i < h->n; ++i) {
            if (h->pvpq[i]) d[h->pvpq[i] - 1] = t0[((size_t)b * h->n + i) * 2];
            if (h->pq[i]) d[h->pq[i] - 1] = t1[((size_t)b * h->n + i) * 2 + 1];
        }
    }
    return 0;
}

int jg_nr_fast_run(jg_nr* h, int64_t max_iter, double tol, int32_t* iters, int32_t* status) {
    if (!h || !h->fast || max_iter < 0 || !(tol > 0.0)) return fail(1, "jg_nr_fast_run: bad argument (or jg_nr_fast_setup missing)");
    if (int rc = set_device(h)) return rc;
    if (!h->gFA) {
        int rc = h->gFA.capture(h->stream, [&] {
            hipMemsetAsync(h->d_counter, 0, sizeof(int), h->stream);
            launch_assemble(h, jg::GroupSel{}, false, nullptr, 1);                  // mismatch! (:687-730)
            launch_check(h, 1);                                                     // powerFlow! accounting (:1406-1420)
            hipMemcpyAsync(h->h_counter, h->d_counter, sizeof(int), hipMemcpyDeviceToHost, h->stream);
            return 0;
        });
        if (!rc) rc = h->gFB.capture(h->stream, [&] {
            h->fast_mask = h->d_active;                                             // solve! (:913-983) on the scenarios still iterating
            if (int rc = fast_half(h, 1)) return rc;
            return fast_half(h, 2);
        });
        if (rc) { h->gFA.reset(); return rc; }
    }
    const double params[2] = {tol, (double)max_iter};
    NR_HIP(hipMemcpyAsync(h->d_params, params, sizeof(params), hipMemcpyHostToDevice, h->stream));
    NR_HIP(hipMemsetAsync(h->d_iters, 0, (size_t)h->ld * 4, h->stream));
    // (eng.status is NOT cleared: nothing is factorised inside this loop -- the pivot flags of the batch's ONE factorisation, jg_nr_fast_setup /
    // jg_nr_fast_patch_batch, are what the verdict of a scenario with a singular B' or B'' must see)
    {
        std::vector<int> act(h->ld, 0);
        for (int b = 0; b < h->batch; ++b) act[b] = 1;
        NR_HIP(hipMemcpyAsync(h->d_active, act.data(), (size_t)h->ld * 4, hipMemcpyHostToDevice, h->stream));
        NR_HIP(hipStreamSynchronize(h->stream));
    }
    for (int64_t it = 0; it <= max_iter; ++it) {
        NR_HIP(h->gFA.launch(h->stream));
        NR_HIP(hipStreamSynchronize(h->stream));
        if (*h->h_counter == 0) break;
        NR_HIP(h->gFB.launch(h->stream));
    }
    NR_HIP(hipStreamSynchronize(h->stream));
    if (iters) NR_HIP(jg::sync_copy(iters, h->d_iters, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
    if (status) NR_HIP(jg::sync_copy(status, h->d_status, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

int jg_nr_set_branches(jg_nr* h, int64_t nb, const int64_t* from, const int64_t* to, const int8_t* status, const double* param) {
    if (!h || nb < 1 || !from || !to || !status || !param) return fail(1, "jg_nr_set_branches: bad argument");
    if (int rc = set_device(h)) return rc;
    std::vector<int> f(nb), t(nb);
    for (int64_t k = 0; k < nb; ++k) {
        if (from[k] < 1 || from[k] > h->n || to[k] < 1 || to[k] > h->n) return fail(1, "jg_nr_set_branches: bus index out of range");
        f[k] = (int)(from[k] - 1); t[k] = (int)(to[k] - 1);
    }
    NR_HIP(hipStreamSynchronize(h->stream));
    if (h->upload(&h->d_bfrom, f) || h->upload(&h->d_bto, t) || h->upload(&h->d_bstatus, std::vector<signed char>(status, status + nb)) ||
        h->upload(&h->d_bparam, std::vector<double>(param, param + nb * 16))) return 2;
    if (!h->d_outage) NR_HIP(h->alloc(&h->d_outage, (size_t)h->ld, true));
    if ((int)nb != h->nb)                                        //  the screen's partial maxima are sized by the branch count and a rating
        for (double** p : {&h->d_screen, &h->d_screc, &h->d_rating}) h->release(p);   // belongs to the branch table it was installed for: both go with the old table
    h->nb = (int)nb;
    return 0;
}

int jg_nr_set_outage_labels(jg_nr* h, const int64_t* label) {
    if (!h || !label) return fail(1, "jg_nr_set_outage_labels: bad argument");
    if (!h->d_outage) return fail(1, "jg_nr_set_outage_labels: call jg_nr_set_branches first");
    if (int rc = set_device(h)) return rc;
    std::vector<int> v(h->ld, 0);
    for (int b = 0; b < h->batch; ++b) {
        if (label[b] < 0 || label[b] > h->nb) return fail(1, "jg_nr_set_outage_labels: label out of range");
        v[b] = (int)label[b];
    }
    NR_HIP(hipStreamSynchronize(h->stream));
    NR_HIP(jg::sync_copy(h->d_outage, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

static int post_staging(jg_nr* h, size_t bytes) {
    if (bytes <= h->post_bytes) return 0;
    h->post_bytes = 0;
    NR_HIP(h->alloc(&h->d_post, (bytes + sizeof(double) - 1) / sizeof(double)));
    h->post_bytes = bytes;
    return 0;
}

int jg_nr_branch_quantities(jg_nr* h, double* from_pq, double* to_pq, double* series_pq, double* charging_pq,
                            double* from_i, double* to_i, double* series_i) {
    if (!h) return fail(1, "jg_nr_branch_quantities: bad argument");
    if (!h->d_bparam) return fail(1, "jg_nr_branch_quantities: call jg_nr_set_branches first");
    if (int rc = set_device(h)) return rc;
    double* host[7] = {from_pq, to_pq, series_pq, charging_pq, from_i, to_i, series_i};
    const size_t one = (size_t)h->nb * h->ld * 2 * sizeof(double);
    int want = 0;
    for (double* p : host) want += p != nullptr;
    if (!want) return 0;
    if (int rc = post_staging(h, one * want)) return rc;
    double* dev[7];
    int q = 0;
    for (int k = 0; k < 7; ++k) dev[k] = host[k] ? h->d_post + (size_t)(q++) * (one / sizeof(double)) : nullptr;
    BranchArgs a{h->d_bfrom, h->d_bto, h->d_bstatus, h->d_bparam, h->d_vm, h->d_va, h->d_outage,
                 dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], h->nb, h->ld, h->batch};
    hipLaunchKernelGGL(k_branch_quantities, dim3((h->nb + 15) / 16, h->ld / 64), dim3(64, 16), 0, h->stream, a);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 7; ++k)
        if (host[k]) if (int rc = h->get_rows2(dev[k], host[k], (size_t)h->nb)) return rc;
    return 0;
}

int jg_nr_bus_injection(jg_nr* h, double* inj_pq) {
    if (!h || !inj_pq) return fail(1, "jg_nr_bus_injection: bad argument");
    if (int rc = set_device(h)) return rc;
    if (int rc = post_staging(h, (size_t)h->n * h->ld * 2 * sizeof(double))) return rc;
    launch_assemble(h, jg::GroupSel{}, false, h->d_post);          // the mismatch pass of the assembly kernel: one Ybus row walk, patches applied
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    h->jac_valid = false;
    return h->get_rows2(h->d_post, inj_pq, (size_t)h->n);
}

int jg_nr_set_screen(jg_nr* h, const double* rating) {
    if (!h) return fail(1, "jg_nr_set_screen: bad argument");
    if (!h->d_bparam) return fail(1, "jg_nr_set_screen: call jg_nr_set_branches first");
    if (int rc = set_device(h)) return rc;
    h->release(&h->d_rating);
    if (rating) {
        for (int k = 0; k < h->nb; ++k) if (!(rating[k] >= 0.0)) return fail(1, "jg_nr_set_screen: a rating is negative or not a number (0 = no limit)");
        if (int rc = h->upload(&h->d_rating, std::vector<double>(rating, rating + h->nb))) return rc;
    }
    return 0;
}

static int screen_launch(jg_nr* h) {
    if (!h->d_bparam) return fail(1, "jg_nr_screen: call jg_nr_set_branches first");
    const int bchunks = (h->nb + SCREEN_BR - 1) / SCREEN_BR, vchunks = (h->n + SCREEN_BUS - 1) / SCREEN_BUS;
    if (!h->d_screen) {
        NR_HIP(h->alloc(&h->d_screen, (size_t)(bchunks + vchunks) * 4 * h->ld));
        NR_HIP(h->alloc(&h->d_screc, (size_t)h->ld * 10));
    }
    ScreenArgs a{h->d_bfrom, h->d_bto, h->d_bstatus, h->d_bparam, h->d_rating, h->d_vm, h->d_va, h->d_outage, h->d_screen, h->d_iters, h->d_status,
                 h->d_screc, h->nb, h->n, h->ld, h->batch, bchunks, vchunks};
    hipLaunchKernelGGL(k_screen_partial, dim3(bchunks + vchunks, h->ld / 64), dim3(64, 16), 0, h->stream, a);
    hipLaunchKernelGGL(k_screen_final, dim3(h->ld / 64), dim3(64), 0, h->stream, a);
    NR_HIP(hipGetLastError());
    return 0;
}

int jg_nr_screen(jg_nr* h, double* rec) {
    if (!h || !rec) return fail(1, "jg_nr_screen: bad argument");
    if (int rc = set_device(h)) return rc;
    if (int rc = screen_launch(h)) return rc;
    NR_HIP(jg::sync_copy(rec, h->d_screc, (size_t)h->batch * 10 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return 0;
}

int jg_nr_screen_device(jg_nr* h, double* rec_dev) {
    if (!h || !rec_dev) return fail(1, "jg_nr_screen_device: bad argument");
    if (int rc = set_device(h)) return rc;
    if (int rc = screen_launch(h)) return rc;
    NR_HIP(hipMemcpyAsync(rec_dev, h->d_screc, (size_t)h->batch * 10 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// rows of a summary record from a range of lanes (the stragglers a pool finished: jg_nr_pack_rows_device's counterpart)
__global__ void k_screen_rows(const double* screc, const int* rows, double* dst, int lane0, int count) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * 10) return;
    const int i = t / 10, c = t - i * 10;
    dst[(size_t)rows[i] * 10 + c] = screc[(size_t)(lane0 + i) * 10 + c];
}

int jg_nr_screen_rows_device(jg_nr* h, double* rec_dev, int64_t lane0, int64_t count, const int32_t* rows) {
    if (!h || !rec_dev || !rows || lane0 < 0 || count < 0 || lane0 + count > h->batch) return fail(1, "jg_nr_screen_rows_device: bad argument");
    if (count == 0) return 0;
    if (int rc = set_device(h)) return rc;
    if (int rc = screen_launch(h)) return rc;
    NR_HIP(hipMemcpyAsync(h->d_itmp, rows, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_screen_rows, dim3((unsigned)((count * 10 + 255) / 256)), dim3(256), 0, h->stream, h->d_screc, h->d_itmp, rec_dev, (int)lane0, (int)count);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}


// ---- bus types per scenario and reactiveLimit! on a batch (jg_qlim.hip) -------------------------------------------------------------------
int jg_nr_set_bus_type(jg_nr* h, int64_t scenario0, int64_t count, const int8_t* type) {
    if (!h || scenario0 < 0 || count < 0 || scenario0 + count > (int64_t)h->batch) return fail(1, "jg_nr_set_bus_type: bad argument");
    if (h->fast) return fail(1, "jg_nr_set_bus_type: a fast Newton-Raphson handle keeps its create-time types");
    if (h->batch < 2) return fail(1, "jg_nr_set_bus_type: a handle of one scenario keeps its create-time types (the single-instance path)");
    if (h->refine) return fail(1, "jg_nr_set_bus_type: iterative refinement (jg_nr_set_refine) reads the create-time types");
    if (h->paused) return fail(1, "jg_nr_set_bus_type: the handle is paused (jg_nr_run_defer)");
    const int n = h->n;
    if (type)
        for (int64_t s = 0; s < count; ++s) {
            int slacks = 0;
            for (int i = 0; i < n; ++i) {
                const int8_t t = type[s * n + i];
                if (t < 1 || t > 3) return fail(1, "jg_nr_set_bus_type: a bus type is 1 (PQ), 2 (PV) or 3 (slack)");
                slacks += t == 3;
            }
            if (slacks != 1) return fail(1, "jg_nr_set_bus_type: scenario " + std::to_string(scenario0 + s) + " does not have exactly one slack bus");
        }
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    if (int rc = ensure_lane_types(h)) return rc;
    if (count == 0) return 0;
    const int rows = lt_rows(h);
    std::vector<unsigned long long> w((size_t)rows * count);
    for (int64_t s = 0; s < count; ++s) {
        const int8_t* t = type ? type + s * n : h->type.data();
        pack_types(t, n, w.data() + s, rows, (size_t)count);
        h->lt_set[scenario0 + s] = type && std::memcmp(t, h->type.data(), (size_t)n) != 0;
        h->dead[scenario0 + s] = 0;
    }
    NR_HIP(hipMemcpy2DAsync(h->d_lt + scenario0, (size_t)h->ld * 8, w.data(), (size_t)count * 8, (size_t)count * 8, (size_t)rows, hipMemcpyHostToDevice, h->stream));
    NR_HIP(hipStreamSynchronize(h->stream));
    h->start_is_base = false;                                    // the next run refactorises (the base's factor has the create-time types)
    h->jac_valid = false;
    set_lane_types_on(h);
    return 0;
}

int jg_nr_get_bus_type(jg_nr* h, int8_t* type, int64_t* slack) {
    if (!h) return fail(1, "jg_nr_get_bus_type: bad argument");
    if (int rc = set_device(h)) return rc;
    const int n = h->n, rows = lt_rows(h);
    std::vector<unsigned long long> w;
    if (h->d_lt) {
        w.resize((size_t)rows * h->ld);
        NR_HIP(jg::sync_copy(w.data(), h->d_lt, w.size() * 8, hipMemcpyDeviceToHost, h->stream));
    }
    for (int b = 0; b < h->batch; ++b) {
        int64_t sl = 0;
        for (int i = 0; i < n; ++i) {
            const int t = h->d_lt ? (int)((w[(size_t)(i >> 5) * h->ld + b] >> ((i & 31) * 2)) & 3) : h->type[i];
            if (type) type[(size_t)b * n + i] = (int8_t)t;
            if (t == 3 && sl == 0) sl = i + 1;
        }
        if (slack) slack[b] = sl;
    }
    return 0;
}

int jg_nr_set_generators(jg_nr* h, int64_t ng, const int64_t* bus, const int8_t* status, const double* pg, const double* qmin, const double* qmax,
                         const double* vg, const double* bus_vm, const double* bus_va, const double* pd, const double* qd, double base_mva) {
    if (!h || ng < 0 || (ng > 0 && (!bus || !status || !pg || !qmin || !qmax || !vg)) || !bus_vm || !bus_va || !pd || !qd || !(base_mva > 0.0))
        return fail(1, "jg_nr_set_generators: bad argument");
    if (h->fast) return fail(1, "jg_nr_set_generators: reactive limits are not available for fast Newton-Raphson");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    std::string msg;
    if (int rc = jg::qlim_setup(h->qt, h->n, h->ld, (int)ng, bus, status, pg, qmin, qmax, vg, bus_vm, bus_va, pd, qd, base_mva, h->stream, msg)) return fail(rc, msg);
    return 0;
}

int jg_nr_reactive_limit(jg_nr* h, int flags, int8_t* violate, int32_t* count) {
    if (!h || flags < 0 || flags > 1) return fail(1, "jg_nr_reactive_limit: bad argument (flags: 0 or 1 = restart the scenarios with a violation)");
    if (h->fast) return fail(1, "jg_nr_reactive_limit: reactive limits are not available for fast Newton-Raphson");
    if (h->batch < 2) return fail(1, "jg_nr_reactive_limit: a handle of one scenario (the single-instance path keeps its create-time types)");
    if (h->refine) return fail(1, "jg_nr_reactive_limit: iterative refinement (jg_nr_set_refine) reads the create-time types");
    if (h->paused) return fail(1, "jg_nr_reactive_limit: the handle is paused (jg_nr_run_defer)");
    if (!h->qt.ready()) return fail(1, "jg_nr_reactive_limit: no generator table (jg_nr_set_generators)");
    if (int rc = set_device(h)) return rc;
    NR_HIP(hipStreamSynchronize(h->stream));
    if (int rc = ensure_lane_types(h)) return rc;
    if (!h->d_skip) NR_HIP(h->alloc(&h->d_skip, (size_t)h->ld));
    std::vector<int> skip(h->ld, 0);
    for (int b = 0; b < h->batch; ++b) skip[b] = h->dead[b];
    NR_HIP(hipMemcpyAsync(h->d_skip, skip.data(), skip.size() * 4, hipMemcpyHostToDevice, h->stream));
    // P_i, Q_i of every lane at its current state (the mismatch pass of its own types) into the factor storage, which holds nothing live between runs
    launch_assemble(h, jg::GroupSel{}, false, h->eng.X);
    h->jac_valid = false;
    h->f_stale = true;                                           // injections, types and (restart) state change below: method.mismatch is re-assembled on demand
    jg::qlim_launch(h->qt, h->eng.X, h->d_lt, h->d_p, h->d_q, h->d_vm, h->d_va, h->d_skip, h->batch, h->ld, (flags & 1) != 0, h->stream);
    NR_HIP(hipGetLastError());
    std::vector<int> cnt(h->ld), dead(h->ld);
    NR_HIP(jg::sync_copy(cnt.data(), h->qt.cnt, (size_t)h->ld * 4, hipMemcpyDeviceToHost, h->stream));
    NR_HIP(jg::sync_copy(dead.data(), h->qt.dead, (size_t)h->ld * 4, hipMemcpyDeviceToHost, h->stream));
    if (violate) {
        const int ng = h->qt.ng;
        std::vector<signed char> v((size_t)std::max(ng, 1) * h->ld);
        NR_HIP(jg::sync_copy(v.data(), h->qt.VO, v.size(), hipMemcpyDeviceToHost, h->stream));
        for (int b = 0; b < h->batch; ++b)
            for (int k = 0; k < ng; ++k) violate[(size_t)b * ng + k] = v[(size_t)k * h->ld + b];
    }
    for (int b = 0; b < h->batch; ++b) {
        if (count) count[b] = cnt[b];
        if (dead[b]) h->dead[b] = 1;
        else if (cnt[b] > 0) h->lt_set[b] = 1;
    }
    h->start_is_base = false;
    h->inj_checked = false;
    set_lane_types_on(h);
    return 0;
}

int jg_nr_adjust_angle(jg_nr* h, int64_t bus, double angle) {
    if (!h || bus < 1 || bus > h->n) return fail(1, "jg_nr_adjust_angle: bad argument (bus: 1-based index)");
    if (int rc = set_device(h)) return rc;
    if (!h->d_shift) NR_HIP(h->alloc(&h->d_shift, (size_t)h->ld));
    jg::adjust_angle_launch(h->d_shift, h->d_va, h->n, h->ld, h->batch, (int)bus - 1, angle, h->stream);
    NR_HIP(hipGetLastError());
    NR_HIP(hipStreamSynchronize(h->stream));
    h->jac_valid = false;
    h->start_is_base = false;
    return 0;
}

int jg_nr_time_kernel(jg_nr* h, int kernel, int reps, double* mean_ms) {
    if (!h || reps < 1 || !mean_ms || kernel < 0 || kernel > 5) return fail(1, "jg_nr_time_kernel: bad argument");
    if (kernel == 4 && (!h->base || !h->d_cw)) return fail(1, "jg_nr_time_kernel: kernel 4 (first iteration on the shared base factor) needs an attached base");
    if (h->fast && kernel < 2) return fail(1, "jg_nr_time_kernel: assembly / factorisation timing would overwrite the constant factor of a fast Newton-Raphson handle");
    if (int rc = set_device(h)) return rc;
    BranchArgs ba{};
    if (kernel == 3) {                                           // power!/current! branch kernel, all seven outputs
        if (!h->d_bparam) return fail(1, "jg_nr_time_kernel: call jg_nr_set_branches first");
        const size_t one = (size_t)h->nb * h->ld * 2;
        if (int rc = post_staging(h, one * 7 * sizeof(double))) return rc;
        ba = BranchArgs{h->d_bfrom, h->d_bto, h->d_bstatus, h->d_bparam, h->d_vm, h->d_va, h->d_outage, h->d_post, h->d_post + one,
                        h->d_post + 2 * one, h->d_post + 3 * one, h->d_post + 4 * one, h->d_post + 5 * one, h->d_post + 6 * one,
                        h->nb, h->ld, h->batch};
    }
    hipEvent_t e0, e1;
    NR_HIP(hipEventCreate(&e0));
    NR_HIP(hipEventCreate(&e1));
    jg::StateUpdate none{};
    NR_HIP(hipStreamSynchronize(h->stream));
    {
        NR_HIP(hipEventRecord(e0, h->stream));
        for (int r = 0; r < reps; ++r) {
            if (kernel == 0) launch_assemble(h, jg::GroupSel{}, true, nullptr, 0, nullptr, true);     // as the iteration runs it
            else if (kernel == 1) { if (int rc = h->eng.factor(h->stream, nullptr, h->d_F, jg::GroupSel{}, h->eng.plan->S.prefactor != 0)) return fail(rc, h->eng.error); }
            else if (kernel == 3) hipLaunchKernelGGL(k_branch_quantities, dim3((h->nb + 15) / 16, h->ld / 64), dim3(64, 16), 0, h->stream, ba);
            else if (kernel == 4) {                              // the linear step of a compensated first iteration: correction + sweep pair on the shared factor (no state update)
                const jg::CompBase& cb = h->base->cb;
                jg::CompFixArgs fa{h->d_ppos, h->d_pdg, h->d_pdb, h->mp, cb.rowptr, cb.colm, cb.posrow, cb.rowtype, cb.v0, cb.th0, cb.y0, cb.Zc,
                                   h->d_F, h->eng.status, nullptr, h->ld, h->batch};
                if (h->mp > 0) jg::launch_comp_fix(fa, h->stream);
                if (int rc = cb.solve(cb.split, h->stream, h->d_F, h->d_cw, inc_out(h), h->ld, h->batch, none, jg::GroupSel{}, comp_dead_ok(h))) return fail(rc, "shared-factor sweep failed");
            }
            else if (kernel == 5) launch_assemble(h, jg::GroupSel{}, false);      // the mismatch-only pass of a compensated start
            else { if (int rc = h->eng.backsolve(h->stream, inc_out(h), none, jg::GroupSel{})) return fail(rc, h->eng.error); }   // (the sweep as the handle's iterations run it)
        }
        NR_HIP(hipEventRecord(e1, h->stream));
    }
    NR_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    NR_HIP(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (kernel <= 1) h->jac_valid = false;                       // the factor storage no longer holds the plain Jacobian (kernel 0 runs the
                                                                 // prefactoring assembly: leaf diagonal blocks leave as 2x2 LU factors)
    *mean_ms = (double)ms / reps;
    return 0;
}

}  // extern "C"
