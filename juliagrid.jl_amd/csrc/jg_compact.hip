// jg_compact.hip -- the scenario compaction, the lane moves and the straggler hand-off of the Newton-Raphson handle (jg_compact.hpp).
#include "jg_compact.hpp"

#include <algorithm>

#include "jg_engine.hpp"

namespace jg {

namespace {

// inclusive scan over the 1024 threads of the workgroup: shuffles inside a wave, the 16 wave totals through LDS (two barriers; the
// Hillis-Steele loop it replaces had twenty and made the verdict of a single instance 12 us long)
__device__ __forceinline__ int block_scan_1024(int v, int* wsum, int t, int& total) {
    const int lane = t & 63, w = t >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int q = wsum[k]; off += k < w ? q : 0; total += q; }
    __syncthreads();
    return x + off;
}

// run_setup on the device: parameters of the run, every real scenario active with zero iterations, lanes in home order, all lane groups in use
__global__ void k_run_setup(double* params, double tol, double max_iter, double defer_at, int* iters, int* lu_status, int* active, int* lid, int* cflags, int* group, int* glist,
                            int ld, int lanes, int keep_iters) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < ld) {
        if (!keep_iters) { iters[b] = 0; lu_status[b] = 0; active[b] = b < lanes ? 1 : 0; }
        lid[b] = b;
    }
    if (b < ld / 64) { group[b] = 1; glist[b] = b; }
    if (b == 0) {
        params[0] = tol; params[1] = max_iter; params[2] = defer_at;
        cflags[0] = 0; cflags[1] = lanes; cflags[2] = ld / 64; cflags[3] = ld / 64; cflags[4] = 0; cflags[5] = 0; cflags[6] = 0; cflags[7] = 0;
    }
}

__global__ __launch_bounds__(1024) void k_compact(CompactArgs a) {
    __shared__ int wsum[16];
    const int t = threadIdx.x;
    const int ld = a.ld, ngroups = ld / 64;
    const int per = (ld + 1023) / 1024;
    const int b0 = t * per, b1 = min(b0 + per, ld);
    int cnt = 0;
    for (int b = b0; b < b1; ++b) cnt += a.active[b] != 0;
    int n_active;
    (void)block_scan_1024(cnt, wsum, t, n_active);
    const int groups_new = (n_active + 63) / 64;
    const int groups_cur = a.flags[2];
    const int defer_at = a.params ? (int)a.params[2] : 0;
    const bool hold = !a.restore && defer_at > 0 && n_active > 0 && n_active <= defer_at;
    bool moved = false;
    if (a.restore) {                                              // lanes that never left home need no pass over the rows
        int away = 0;
        for (int b = b0; b < b1; ++b) away += a.lid[b] != b;
        int any;
        (void)block_scan_1024(away, wsum, t, any);
        moved = any > 0;
    }
    const bool permute = a.restore ? moved : (!hold && n_active > 0 && groups_new < groups_cur);
    if (a.host_res && n_active == 0 && t < 64) { a.host_res[t] = a.iters[t]; a.host_res[64 + t] = a.status[t]; __threadfence_system(); }   // ... ahead of the word the host polls
    __syncthreads();
    if (t == 0) { a.flags[0] = permute ? 1 : 0; a.flags[1] = n_active; a.flags[4] = hold ? 1 : 0; if (permute) a.flags[2] = a.restore ? ngroups : groups_new; if (a.host_count) *a.host_count = n_active; }
    if (a.restore && !permute) {
        for (int g = t; g < ngroups; g += 1024) { a.group[g] = 1; a.glist[g] = g; }
        if (t == 0) { a.flags[2] = ngroups; a.flags[3] = ngroups; }
        return;
    }
    if (hold) {                                                   // the hand-off's list of the lanes that leave, in lane order
        int tot;
        const int incl = block_scan_1024(cnt, wsum, t, tot);
        int r = incl - cnt;
        for (int b = b0; b < b1; ++b) if (a.active[b] != 0) a.dest[r++] = b;
    }
    if (!permute) {                                               // groups = those that still hold an active lane
        for (int g = t; g < ngroups; g += 1024) {
            int any = 0;
            for (int l = 0; l < 64; ++l) any |= a.active[g * 64 + l];
            a.group[g] = any;
        }
        __syncthreads();
        if (t == 0) {
            int m = 0;
            for (int g = 0; g < ngroups; ++g) if (a.group[g]) a.glist[m++] = g;
            a.flags[3] = m;
        }
        return;
    }
    if (a.restore) {
        for (int b = b0; b < b1; ++b) a.dest[b] = a.lid[b];      // send every lane home
    } else {
        // Minimal moves: an active lane inside the leading groups_new groups stays where it is; the k-th active lane behind them
        // swaps with the k-th inactive lane inside them.  (A stable partition shifted almost every lane: 1 GB of lane rows per
        // compaction of 512 scenarios of a 10 000-bus grid, and again for the way home; 37 stragglers of 512 now move 64 lanes.)
        const int L = groups_new * 64;
        int holes = 0, outs = 0;
        for (int b = b0; b < b1; ++b) { const bool act = a.active[b] != 0; holes += (b < L && !act); outs += (b >= L && act); a.dest[b] = b; }
        int both;
        const int incl = block_scan_1024(holes | outs << 16, wsum, t, both);   // both counts in one scan: ld < 65 536
        int hr = (incl & 0xffff) - holes, orank = (incl >> 16) - outs;         // holes / outside actives in front of this thread's chunk
        int* hole_at = a.tmp;                                     // [k] position of the k-th hole, [ld / 2 + k] of the k-th outside active lane
        int* out_at = a.tmp + ld / 2;
        const int n_out = both >> 16;                             // <= min(L, ld - L) <= ld / 2; the leading groups hold at least as many holes
        for (int b = b0; b < b1; ++b) {
            const bool act = a.active[b] != 0;
            if (b < L && !act) { if (hr < n_out) hole_at[hr] = b; ++hr; }
            if (b >= L && act) out_at[orank++] = b;
        }
        __syncthreads();
        for (int k = t; k < n_out; k += 1024) { const int hpos = hole_at[k], opos = out_at[k]; a.dest[opos] = hpos; a.dest[hpos] = opos; }
    }
    __syncthreads();
    int* arrays[5] = {a.active, a.iters, a.status, a.lu_status, a.lid};
    for (int k = 0; k < 5 + a.mp; ++k) {
        int* x = k < 5 ? arrays[k] : a.ppos + (size_t)(k - 5) * ld;
        for (int b = b0; b < b1; ++b) a.tmp[a.dest[b]] = x[b];
        __syncthreads();
        for (int b = b0; b < b1; ++b) x[b] = a.tmp[b];
        __syncthreads();
    }
    for (int g = t; g < ngroups; g += 1024) { a.group[g] = a.restore ? 1 : (g < groups_new); a.glist[g] = g; }
    if (t == 0) a.flags[3] = a.restore ? ngroups : groups_new;
}

// The per-scenario arrays of a compaction in TWO launches (scatter into the staging area, copy back; no-ops unless flags[0]) instead of two per array:
// the launches are predicated on flags[0] and mostly return at once, so what they cost is their number.
struct LaneSet { double* x[8]; int rows[8]; int elem[8]; long long off[8]; };
__global__ void k_lanes_move(LaneSet s, double* tmp, const int* dest, const int* flags, int ld, int back) {
    if (!flags[0]) return;
    const int b = blockIdx.y * 256 + threadIdx.x;
    if (b >= ld) return;
    const int a = blockIdx.z;
    const int rows = s.rows[a], E = s.elem[a];
    double* x = s.x[a];
    double* t = tmp + s.off[a];
    const int d = dest[b];
    if (d == b) return;                            // this lane stays (a permutation maps the lanes that move onto themselves)
    if (E == 2) {                                  // interleaved 2-vectors: one 16-byte access per lane
        double2* x2 = (double2*)x;
        double2* t2 = (double2*)t;
        for (int r = blockIdx.x; r < rows; r += gridDim.x) {
            if (back) x2[(size_t)r * ld + b] = t2[(size_t)r * ld + b];
            else t2[(size_t)r * ld + d] = x2[(size_t)r * ld + b];
        }
        return;
    }
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        if (back) x[(size_t)r * ld + b] = t[(size_t)r * ld + b];
        else t[(size_t)r * ld + d] = x[(size_t)r * ld + b];
    }
}

// The same move IN PLACE, one launch (round 5): dest is a permutation of the lanes (k_compact: swaps of a hole with a straggler; restore: every lane to its home), so a
// workgroup that holds ALL lanes of a row reads what moves, waits for the values, meets at a barrier and writes them to their new lanes -- no staging area, half
// the traffic and half the launches of the two-pass move (which remains for handles of more than LANES_INPLACE lanes).
constexpr int LANES_INPLACE = 4096;
__global__ __launch_bounds__(1024) void k_lanes_permute(LaneSet s, const int* dest, const int* flags, int ld) {
    if (!flags[0]) return;
    constexpr int NL = LANES_INPLACE / 1024;
    const int a = blockIdx.z;
    const int rows = s.rows[a], E = s.elem[a];
    int b[NL], d[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) { b[k] = (int)threadIdx.x + k * 1024; d[k] = b[k] < ld ? dest[b[k]] : b[k]; }
    if (E == 2) {
        double2* x = (double2*)s.x[a];
        for (int r = blockIdx.x; r < rows; r += gridDim.x) {
            double2 v[NL];
#pragma unroll
            for (int k = 0; k < NL; ++k) if (d[k] != b[k]) v[k] = x[(size_t)r * ld + b[k]];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the values are HERE before any lane of the row is overwritten
            __syncthreads();
#pragma unroll
            for (int k = 0; k < NL; ++k) if (d[k] != b[k]) x[(size_t)r * ld + d[k]] = v[k];
        }
        return;
    }
    double* x = s.x[a];
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        double v[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) if (d[k] != b[k]) v[k] = x[(size_t)r * ld + b[k]];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NL; ++k) if (d[k] != b[k]) x[(size_t)r * ld + d[k]] = v[k];
    }
}

// ---- straggler hand-off (jg_nr_move_lanes): the scenarios of a paused batch that are still active -- all inside its first
// lane group -- continue in another handle of the same grid (a pool that collects the stragglers of several batches).
// k_move_plan (one wave): pool lane of every active position, the per-lane integers, the home lane of each moved scenario; the
// source lanes become inactive with status 4 (deferred).  k_move_rows: the per-lane rows (V, theta, P, Q, patch values).
struct MovePlanArgs {
    int* s_active; int* s_iters; int* s_status; const int* s_lid; const int* s_ppos; int s_ld;
    int* d_active; int* d_iters; int* d_status; int* d_lu; int* d_ppos; int d_ld;
    int* map; int* home; int* count; int mp; int lane0; int cap;
    const int* s_flags; const int* s_list; int* srcl;          // the source's compaction flags / list of the lanes that leave (k_compact: hold); [64] source lane of candidate p
};
__global__ __launch_bounds__(64) void k_move_plan(MovePlanArgs a) {
    const int p0 = threadIdx.x;
    // where the p-th candidate sits: packed into the first lane group by a compaction, or -- the batch stopped for this hand-off (k_compact: hold) -- wherever
    // it was, listed in the source's dest[]
    const bool listed = a.s_flags[4] != 0;
    const int p = listed ? (p0 < a.s_flags[1] ? a.s_list[p0] : -1) : p0;
    a.srcl[p0] = p;
    const bool act = p >= 0 && a.s_active[p] != 0;
    const unsigned long long m = __ballot(act);
    const int r = __popcll(m & ((1ull << p0) - 1ull));
    const int total = __popcll(m);
    const bool fits = a.lane0 + total <= a.cap;
    if (p0 == 0) a.count[0] = fits ? total : -1;
    a.map[p0] = -1;
    if (!act || !fits) return;
    const int d = a.lane0 + r;
    a.map[p0] = d;
    a.home[r] = a.s_lid[p];
    a.d_active[d] = 1; a.d_iters[d] = a.s_iters[p]; a.d_status[d] = 1; a.d_lu[d] = 0;
    for (int k = 0; k < a.mp; ++k) a.d_ppos[(size_t)k * a.d_ld + d] = a.s_ppos[(size_t)k * a.s_ld + p];
    a.s_active[p] = 0; a.s_status[p] = 4;
}
struct MoveRowsArgs { const double* src[6]; double* dst[6]; int rows[6]; int s_ld; int d_ld; const int* map; const int* srcl; };
__global__ __launch_bounds__(256) void k_move_rows(MoveRowsArgs a) {
    const int p0 = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const int d = a.map[p0];
    if (d < 0) return;
    const int p = a.srcl[p0];
    const int arr = blockIdx.y;
    const double* s = a.src[arr];
    double* t = a.dst[arr];
    for (int r = blockIdx.x * 4 + sub; r < a.rows[arr]; r += gridDim.x * 4) t[(size_t)r * a.d_ld + d] = s[(size_t)r * a.s_ld + p];
}

}  // namespace

void Compaction::run_setup(hipStream_t st, double tol, double max_iter, double defer_at, int lanes, bool keep_iters) const {
    hipLaunchKernelGGL(k_run_setup, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, st, params, tol, max_iter, defer_at,
                       iters /* acPowerFlow.jl:1401 */, lu_status, active, lid, cflags, group, glist, ld, lanes, keep_iters ? 1 : 0);
}

void Compaction::launch_compact(hipStream_t st, int restore, bool report_, const std::vector<LaneRows>& rows) const {
    hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, st, args(restore, report_));
    if (ld == 64) return;                          // one lane group: nothing to pack, lanes never leave their home order
    LaneSet ls{};
    int na = 0, max_rows = 0;
    long long off = 0;
    for (const LaneRows& r : rows) {
        ls.x[na] = r.x; ls.rows[na] = r.rows; ls.elem[na] = r.elem; ls.off[na] = off;
        off += (long long)r.rows * r.elem * ld; max_rows = std::max(max_rows, r.rows); ++na;
    }
    static const bool inplace_env = knob("LANES_INPLACE", 1) != 0;
    if (ld <= LANES_INPLACE && inplace_env) {      // one launch, in place (k_lanes_permute); JG_LANES_INPLACE=0: the two-pass move
        hipLaunchKernelGGL(k_lanes_permute, dim3((unsigned)std::min(max_rows, 2048), 1, (unsigned)na), dim3((unsigned)std::min(1024, ld)), 0, st, ls, dest, cflags, ld);
        return;
    }
    const dim3 block(256), gy((unsigned)((ld + 255) / 256));
    if (fits((size_t)(off / ld))) {                // always, except for grids of a handful of buses
        const dim3 grid((unsigned)std::min(max_rows, 1024), gy.x, (unsigned)na);
        hipLaunchKernelGGL(k_lanes_move, grid, block, 0, st, ls, stage, dest, cflags, ld, 0);
        hipLaunchKernelGGL(k_lanes_move, grid, block, 0, st, ls, stage, dest, cflags, ld, 1);
        return;
    }
    // All arrays together exceed the staging area: the same pair of launches once per array.  ONE array always fits -- the handle holds none longer than
    // the increment, 2 n doubles per lane, and the factor of n buses holds at least its n diagonal blocks, 4 n (jg_nr_create checks fits(2 n)).
    for (const LaneRows& r : rows) {
        const LaneSet one{{r.x}, {r.rows}, {r.elem}, {0}};
        const dim3 grid((unsigned)std::min(r.rows, 1024), gy.x, 1);
        hipLaunchKernelGGL(k_lanes_move, grid, block, 0, st, one, stage, dest, cflags, ld, 0);
        hipLaunchKernelGGL(k_lanes_move, grid, block, 0, st, one, stage, dest, cflags, ld, 1);
    }
}

void Compaction::launch_move_plan(hipStream_t st, const Compaction& dst, int* move, int lane0, int cap) const {
    MovePlanArgs pa{active, iters, status, lid, ppos, ld, dst.active, dst.iters, dst.status, dst.lu_status, dst.ppos, dst.ld,
                    move, move + MOVE_HOME, move + MOVE_COUNT, mp, lane0, cap, cflags, dest, move + MOVE_SRCL};
    hipLaunchKernelGGL(k_move_plan, dim3(1), dim3(64), 0, st, pa);
}

void Compaction::launch_move_rows(hipStream_t st, const Compaction& dst, const int* move, const std::vector<LanePair>& rows) const {
    MoveRowsArgs ra{{}, {}, {}, ld, dst.ld, move, move + MOVE_SRCL};
    int na = 0, max_rows = 0;
    for (const LanePair& r : rows) { ra.src[na] = r.src; ra.dst[na] = r.dst; ra.rows[na] = r.rows; max_rows = std::max(max_rows, r.rows); ++na; }
    hipLaunchKernelGGL(k_move_rows, dim3((unsigned)std::min((max_rows + 3) / 4, 1024), (unsigned)na), dim3(256), 0, st, ra);
}

}  // namespace jg
