// jg_dc_phi.hpp -- the kept outage sensitivities Phi of a DcHandle (jg_dc.hpp), with ONE owner, shared by the three screens on them: the N-2 pair screen
// (jg_dc_pair.hpp, which has the algebra of Phi), the N-1 screen over a series of profiles (jg_dc_series.hpp) and the transfer-capability screen
// (jg_dc_transfer.hpp).  Each screen's state owns a DcPhi beside its own call-time buffers; nothing here knows a screen.  The host side of a screen call and
// the records of its row block: jg_dc_records.hpp.
//
// What is kept: Phi on the rows R = monitored u candidates (ascending branch index), columns = candidates, [rows][ldk] doubles with ldk = candidates
// rounded up to 64 -- the sweep pair of jg_dc_sweep.hip runs once per candidate (a lane batch at a time), never per case.
//
// Device memory of a state is registered with the state as it is allocated (DcMem, beside the handle's allocs) and released as one: no release function
// names a field.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "jg_dc.hpp"
#include "jg_dc_abi.hpp"

namespace jg {

constexpr int DC_PAIR_WAVES = 4;             // waves of a workgroup of the screen kernels: they share ONE chunk of 64 lanes, so its Phi rows meet in the vector L1
constexpr int DC_PAIR_LANES = 512;           // candidates / right-hand sides per sweep pair of a build (a lane batch)
constexpr double DC_PAIR_BUDGET = 0.8;       // default budget of a build: this fraction of the free device memory

typedef std::vector<void*> DcMem;            // the device memory a state owns

struct DcPhi {
    int nk = 0, ldk = 0, rows = 0;
    std::vector<int> h_cand;                 // [nk] candidate branches (0-based, strictly ascending)
    double* Phi = nullptr;                   // [rows][ldk]
    int* row_branch = nullptr;               // [rows] branch of a row (0-based, ascending)
    int* row_pos = nullptr;                  // [rows] position of the row's branch in the candidate list, -1: not a candidate
    int* row_mon = nullptr;                  // [rows] 1: monitored
    double* row_f0 = nullptr;                // [rows] base-case flow
    double* row_rinv = nullptr;              // [rows] 1 / rating of a monitored, rated row, else 0 (every screen call sets it from the handle's rating)
    int* cand_row = nullptr;                 // [ldk] row of a candidate
    int* cand_label = nullptr;               // [ldk] 1-based branch label of a candidate
    double* cand_diag = nullptr;             // [ldk] Phi[k,k]
    double* cand_f0 = nullptr;               // [ldk]
    // shed mode of a build (jg_dc_series.hpp; the pair screen: jg_dc_pair.hpp): a bridge candidate's column holds Z[:,k] = y_l a_l' B^-1 e_m instead of Phi[:,k]
    bool shed = false;
    std::vector<int> h_side, h_lo, h_hi;     // [nk] dc_island_table of the candidates: side 0: not a bridge; lo .. hi the preorder interval of what leaves
    int* cand_isl = nullptr;                 // [ldk][4] side, lo, hi, 0 ((0, 1, 0, 0): not a bridge, the interval is empty)
    int* row_pre = nullptr;                  // [rows] preorder number of the from end of the row's branch
    double build_ms[3] = {0, 0, 0};          // the last build: total, sweep pairs, Phi kernel (HIP events)
    DcMem mem;                               // the device memory of the fields above: what release frees
};

// ---- device memory of a state -----------------------------------------------------------------------------------------------------------
template <typename T>
void dev_release(DcHandle* h, DcMem& own, T*& p) {       // one pointer, out of both lists: the grow paths
    own.erase(std::remove(own.begin(), own.end(), (void*)p), own.end());
    dev_release(h, p);
}
template <typename T>
int dev_alloc(DcHandle* h, DcMem& own, T** p, size_t count, const T* src = nullptr, bool zero = false) {
    dev_release(h, own, *p);                 // (what *p still held goes first, so `own` never keeps a block nothing points to)
    const int rc = dev_alloc(h, p, count, src, zero);
    if (*p) own.push_back(*p);               // (also when only the upload failed: the state's release frees it)
    return rc;
}
// a screen's state `s` (its own memory and its DcPhi's), behind the work of the handle's stream
template <typename S>
void dc_state_release(DcHandle* h, S*& s) {
    if (!s) return;
    hipStreamSynchronize(h->stream);
    for (DcMem* m : {&s->phi.mem, &s->mem})
        for (void* q : *m) dev_release(h, q);
    delete s;
    s = nullptr;
}
// a build that failed with `rc`: the half-built state goes, the text of the failure stays
template <typename S>
int dc_build_failed(DcHandle* h, S*& s, int rc) {
    const std::string msg = h->error;
    dc_state_release(h, s);
    h->error = msg;
    return rc;
}

// ---- the build ----------------------------------------------------------------------------------------------------------------------------
//   dc_phi_lists        the candidate / monitored lists of a build call (1-based in, 0-based out) with the checks of jg_dc_pair_build; 1 and h->error
//   dc_phi_build        Phi and its tables into the empty `p`.  `extra` bytes the caller keeps beside Phi count in the memory question (code 5, nothing
//                       allocated, `extra_text` names them in the message); info [8] as jg_dc_pair_build.  `shed`: the candidates the handle's island
//                       table (dc_handle_island_table, the graph) calls bridges get the sweep pair on e_m and the tables above
//   dc_phi_rinv         row_rinv from the handle's rating (a launch on the handle's stream)
//   dc_phi_row_flows    F [rows of p][ldt] from `T` right-hand sides rhs [T][n] (the slack's entry is taken as 0): uploads DC_PAIR_LANES of them at a
//                       time, runs the sweep pair and turns the angles into row flows y_m (a_m' theta - shiftAngle_m); shift false: y_m a_m' theta,
//                       the sensitivity of the flow to the right-hand side.  Scratch of its own (dc_phi_flows_scratch bytes), released on return;
//                       ms [2] gets the milliseconds of the sweep pairs and of the flow kernel added (HIP events).  Not 0: the text is in h->error
//   dc_phi_bridges      bridge [nk] 1: |1 - Phi[k,k]| < DC_SINGULAR (and not a bridge the shed mode solves)
//   dc_phi_shed_gather  out [bridges in [k0, k1)][T] on the host = s_k F[row of k][t], from the device (k_shed_gather: one thread per value)
//   dc_phi_row_labels   a build with row flows [rows][ldt] beside Phi (F0, G) opens: the rows, monitored u candidates, as 1-based labels ascending; info [8]
//                       the row flows' bytes, [9..11] 0.  It ends with dc_phi_flows_ms: build_ms [3] and info [9..11] from ms [2] of dc_phi_row_flows
//   dc_hip              a HIP call's result as a step of such a build: 0, or 2 and "`what`: ..." in h->error
int dc_phi_lists(DcHandle* h, const std::string& who, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, std::vector<int>& cand,
                 std::vector<int>& mon);
int dc_phi_build(DcHandle* h, DcPhi* p, const char* who, const std::vector<int>& cand, const std::vector<int>& mon, int64_t budget, size_t extra,
                 const std::string& extra_text, double* info, bool shed = false);
void dc_phi_rinv(DcHandle* h, DcPhi* p);
std::string dc_bytes_text(size_t b);
size_t dc_phi_flows_scratch(const DcHandle* h, int ldt);
int dc_phi_row_flows(DcHandle* h, const DcPhi* p, int T, const double* rhs, bool shift, double* F, int ldt, double* ms);
int dc_phi_bridges(DcHandle* h, const DcPhi* p, std::vector<char>& bridge);
int dc_phi_shed_gather(DcHandle* h, const DcPhi* p, int k0, int k1, const double* F, int ldt, int T, double* out);
std::vector<int> dc_phi_row_labels(const DcHandle* h, const std::vector<int>& cand, const std::vector<int>& mon, int ldt, double* info);
inline void dc_phi_flows_ms(const double* ms, double* build_ms, double* info) {
    build_ms[0] = info[9] = ms[0] + ms[1]; build_ms[1] = info[10] = ms[0]; build_ms[2] = info[11] = ms[1];
}
inline int dc_hip(DcHandle* h, hipError_t e, const char* what) {
    if (e != hipSuccess) h->error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipSuccess ? 0 : 2;
}

// ---- exports the three screens share: `screen` is "pair" / "series" / "transfer", `p` null before the screen's build ---------------------------
// jg_dc_<screen>_set_island_mode.  `flag` (DcHandle::pair_shed / series_shed / transfer_shed) is the mode of the NEXT build, which takes it and sets it back to 0
int dc_phi_set_island_mode(DcHandle* d, const std::string& screen, int mode, int& flag);
// jg_dc_<screen>_get_shed_table: the bridge candidates (shed mode) among the positions [k0, k1): their number, and per bridge the label, the buses that
// leave, m (1-based) and the side; null outputs are skipped
int dc_phi_get_shed_table(DcHandle* d, const std::string& screen, const DcPhi* p, int64_t k0, int64_t k1, int64_t* count, int64_t* labels, int64_t* buses,
                          int64_t* m, int64_t* side);
// jg_dc_<screen>_time_kernel for the rows [k0, k1) of a block of `blk_rows` the screen has held: `make`, called once behind the checks, builds the argument
// blocks and returns what enqueues kernel 0 (the screen kernel) or 1 (the summaries) from them
// dc_phi_time_kernel_rows: the same for a screen whose block rows are not the candidates (the group screen's groups): `count` of them
template <typename Make>
int dc_phi_time_kernel_rows(DcHandle* d, const std::string& screen, const DcPhi* p, int count, int blk_rows, int kernel, int64_t k0, int64_t k1, int reps, double* ms,
                            Make&& make) {
    const std::string me = "jg_dc_" + screen + "_time_kernel: ", of = "jg_dc_" + screen;
    if (!p) return api_fail(4, me + of + "_build first");
    if (!ms || reps < 1 || kernel < 0 || kernel > 1 || k0 < 0 || k1 <= k0 || k1 > count) return api_fail(1, me + "bad argument");
    if (k1 - k0 > blk_rows) return api_fail(4, me + of + "_screen with a block of at least these rows first");
    const auto enqueue = make();
    const int rc = time_events(d->stream, reps, ms, d->error, [&]() -> int { enqueue(kernel); return 0; });
    return rc ? api_fail(rc, d->error) : 0;
}
template <typename Make>
int dc_phi_time_kernel(DcHandle* d, const std::string& screen, const DcPhi* p, int blk_rows, int kernel, int64_t k0, int64_t k1, int reps, double* ms, Make&& make) {
    return dc_phi_time_kernel_rows(d, screen, p, p ? p->nk : 0, blk_rows, kernel, k0, k1, reps, ms, make);
}

}  // namespace jg
