// jg_dc_records.hpp -- the host side of a screen call on the kept sensitivities (jg_dc_phi.hpp) and the records of its row block: ONE kernel and ONE host
// function for the pair, series and transfer screens (.hip units only).
//
// The count pass k_dc_rows<P, false> gives a wave a block row: it walks the row 64 columns at a time, counts each list's hits with a ballot and reduces
// the row (max or min).  The host prefix-sums the rows' counts and uploads the offsets; the scatter pass k_dc_rows<P, true> walks the same way and writes
// a hit at the row's offset + the hits of earlier chunks + its ballot rank.  So a list is sorted by (row, column) without atomics, one that overflows keeps
// the first entries (`at < cap`) and the totals are exact whatever the capacity.  A NaN compares false: no hit, and the row's reduction does not see it.
// A screen supplies the policy P: its argument block and the few __device__ members that say what differs.  Every store is a vector store.
#pragma once
#include "jg_dc_phi.hpp"

namespace jg {

// One record list of a state's row block: [cap] entries, grown and never shrunk; per block row the hits of the count pass and the row's first entry
struct DcRecords {
    size_t entry;                                            // bytes of an entry
    void* rec = nullptr; long long cap = 0;
    int* r_count = nullptr; long long* r_off = nullptr;      // [blk_rows]
    DcRecords limited(long long call_cap) const { DcRecords r = *this; r.cap = call_cap; return r; }     // as a call's kernels see it: the caller's capacity
};

// The row block of a call, grown and never shrunk (the caller asks only when `rows` exceed blk_rows): the rows of the record lists and the arrays listed
// (dc_blk: pointer, elements; 0 elements: not wanted) are released, `need` bytes are held against the free device memory (code 5 with the sizes, blk_rows
// 0), then allocated and zeroed.
template <typename T> struct DcBlk { T** p; size_t count; };
template <typename T> DcBlk<T> dc_blk(T*& p, size_t count) { return {&p, count}; }
template <typename... T>
int dc_block_grow(DcHandle* h, DcMem& own, const char* who, int rows, int& blk_rows, size_t need, std::initializer_list<DcRecords*> lists, DcBlk<T>... a) {
    for (DcRecords* l : lists) { dev_release(h, own, l->r_count); dev_release(h, own, l->r_off); }
    (dev_release(h, own, *a.p), ...);
    blk_rows = 0;
    size_t free_b = 0, total_b = 0;
    DC_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        h->error = std::string(who) + ": a block of " + std::to_string(rows) + " rows needs " + dc_bytes_text(need) + ", " + dc_bytes_text(free_b) + " are free: screen fewer rows per call";
        return 5;
    }
    int rc = 0;
    ((rc = rc || !a.count ? rc : dev_alloc(h, own, a.p, a.count, (const T*)nullptr, true)), ...);
    for (DcRecords* l : lists) {
        rc = rc ? rc : dev_alloc(h, own, &l->r_count, (size_t)rows, (const int*)nullptr, true);
        rc = rc ? rc : dev_alloc(h, own, &l->r_off, (size_t)rows, (const long long*)nullptr, true);
    }
    if (!rc) blk_rows = rows;
    return rc;
}
// a record list on the device, grown to `want` entries
inline int dc_list_grow(DcHandle* h, DcMem& own, DcRecords& r, long long want) {
    if (want <= r.cap) return 0;
    r.cap = 0;
    DC_TRY(dev_alloc(h, own, (char**)&r.rec, (size_t)want * r.entry, (const char*)nullptr, true));
    r.cap = want;
    return 0;
}
// the block's dense result of one quantity on the host: the device's [rb][ld] of V as [rb][T] of D, dst[i][j] = map(i, j, src[i][j])
template <typename V, typename D, typename Map>
int dc_dense(DcHandle* h, D* dst, const V* src, int rb, int ld, int T, Map&& map) {
    std::vector<V> t((size_t)rb * ld);
    DC_HIP(sync_copy(t.data(), src, t.size() * sizeof(V), hipMemcpyDeviceToHost, h->stream));
    for (int i = 0; i < rb; ++i)
        for (int j = 0; j < T; ++j) dst[(size_t)i * T + j] = (D)map(i, j, t[(size_t)i * ld + j]);
    return 0;
}
// the candidates of [k0, k1) that `bridge` marks, as 1-based branch labels into `out` (nullable); returns their number
inline long long dc_bridge_list(const DcPhi& p, const std::vector<char>& bridge, int k0, int k1, int64_t* out) {
    long long n = 0;
    for (int k = k0; k < k1; ++k)
        if (bridge[k]) { if (out) out[n] = p.h_cand[k] + 1; ++n; }
    return n;
}

// ---- the rows kernel ----------------------------------------------------------------------------------------------------------------------------
// A policy P is a screen's argument block with
//   LISTS, list[LISTS]         1 or 2 record lists, as the call limits them (a loop of constant trip count: one list costs one ballot and one offset)
//   clabel, k0, k1, r_red      the candidates' labels, the block's rows [k0, k1), where the rows' reductions go
//   first(k), cols()           the first column of row k's walk (a multiple of 64) and the end of every row's
//   valid(k, j), value(i, j)   whether column j counts in row k, and the dense value of block row i there (read only where valid)
//   hit(q, v, j)               the predicate of list q
//   write(q, at, klab, i, k, j, v)               writes entry `at` of list q; it may decline, the slot stays taken
//   identity(), better(v, m), combine(x, y)      the row's reduction: a lane takes v where better(v, m), the lanes meet by combine
template <class P, bool SCATTER>
__global__ __launch_bounds__(256) void k_dc_rows(P a) {
    const int wave = uniform(threadIdx.y), lane = threadIdx.x;
    const int i = blockIdx.x * 4 + wave;
    const int k = a.k0 + i;
    if (k >= a.k1) return;
    int n[P::LISTS];
    long long base[P::LISTS];
    for (int q = 0; q < P::LISTS; ++q) { n[q] = 0; base[q] = SCATTER ? a.list[q].r_off[i] : 0; }
    double red = P::identity();
    const int klab = ((CInt)a.clabel)[k];
    for (int j0 = a.first(k); j0 < a.cols(); j0 += 64) {
        const int j = j0 + lane;
        const bool valid = a.valid(k, j);
        const double v = valid ? a.value(i, j) : 0.0;
#pragma unroll
        for (int q = 0; q < P::LISTS; ++q) {
            const bool hit = valid && a.hit(q, v, j);
            const unsigned long long m = __ballot(hit);
            if (SCATTER) {
                const long long at = base[q] + __popcll(m & ((1ull << lane) - 1ull));
                if (hit && at < a.list[q].cap) a.write(q, at, klab, i, k, j, v);
                base[q] += __popcll(m);
            } else n[q] += __popcll(m);
        }
        if (!SCATTER && valid && P::better(v, red)) red = v;     // (a NaN compares false)
    }
    if (!SCATTER) {
        for (int s = 32; s; s >>= 1) red = P::combine(red, __shfl_xor(red, s, 64));
        for (int q = 0; q < P::LISTS && lane == 0; ++q) a.list[q].r_count[i] = n[q];
        if (lane == 0) a.r_red[i] = red;
    }
}
template <bool SCATTER, class P>
void dc_launch_rows(DcHandle* h, const P& a) {
    hipLaunchKernelGGL((k_dc_rows<P, SCATTER>), dim3((a.k1 - a.k0 + 3) / 4), dim3(64, 4), 0, h->stream, a);
}

// ---- the records of a block, behind the launches of the screen kernel and the count pass ------------------------------------------------------------
// One list of a call: `cap` entries at the most go to `dst`; out: the hits of the block and how many of them were delivered
struct DcListCall {
    const DcRecords* r; long long cap; void* dst;
    long long total = 0, kept = 0;
    std::vector<int> count; std::vector<long long> off;     // per block row, on the host
};
// Downloads the lists' per-row counts, then lets `rest` enqueue the screen's other small downloads, whose closing sync_copy ends the batch; prefix-sums
// the counts; and only if some list has a record to deliver: uploads the offsets, has `scatter` launch the scatter pass, downloads min(total, cap)
// entries per list and waits (the offsets go out of scope behind it).
template <typename Rest, typename Scatter>
int dc_block_records(DcHandle* h, int rb, std::initializer_list<DcListCall*> lists, Rest&& rest, Scatter&& scatter) {
    DC_HIP(hipGetLastError());
    for (DcListCall* l : lists) {
        l->count.resize(rb); l->off.resize(rb);
        DC_HIP(hipMemcpyAsync(l->count.data(), l->r->r_count, rb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    DC_TRY(rest());
    bool any = false;
    for (DcListCall* l : lists) {
        for (int i = 0; i < rb; ++i) { l->off[i] = l->total; l->total += l->count[i]; }      // the first record of row i
        l->kept = std::min(l->total, l->cap);
        any = any || l->kept;
    }
    if (!any) return 0;
    for (DcListCall* l : lists) DC_HIP(hipMemcpyAsync(l->r->r_off, l->off.data(), rb * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    scatter();
    DC_HIP(hipGetLastError());
    for (DcListCall* l : lists)
        if (l->kept) DC_HIP(hipMemcpyAsync(l->dst, l->r->rec, (size_t)l->kept * l->r->entry, hipMemcpyDeviceToHost, h->stream));
    DC_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

}  // namespace jg
