// jg_dc_sweep.hpp -- internal: the scalar factorisation of ONE matrix on a static pivot order and the level-scheduled sweeps on that shared factor,
// lanes = scenarios / realisations.  The kernels and their launchers are compiled once, in jg_dc_sweep.hip; this header declares the factor they work on
// (DcFactor), what a handle allocates through (DcDevice) and the argument blocks and constants the includers' own kernels share.  Used by jg_dc.hip (the
// DC nodal matrix), jg_dcse.hip (the gain matrix of DC state estimation) and jg_dc_phi.hip (the sweeps of the pair, series and transfer screens' builds on the DC
// handle's factor; the screens' own kernels in jg_dc_pair.hip, jg_dc_series.hip and jg_dc_transfer.hip share the typedefs and constants).
//
// What runs: the elimination order, fill pattern, update terms and dependency levels come from jg_symbolic (no top tasks); the factorisation is a launch
// per dependency level with a thread per entry; the sweeps give a wavefront one row x 64 lanes, read the premultiplied factor values and the column
// indices through the scalar cache (they are the same for every lane) and move 8 bytes per (row, lane) through the vector pipe.  Every store is a
// vector store.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "jg_engine.hpp"
#include "jg_symbolic.hpp"

namespace jg {

typedef const double __attribute__((address_space(4)))* CDbl;      // wave-uniform values: scalar loads
typedef const int __attribute__((address_space(4)))* CInt;
typedef int I4 __attribute__((ext_vector_type(4)));
typedef double D4 __attribute__((ext_vector_type(4)));
typedef const I4 __attribute__((address_space(4)))* CI4;
typedef const D4 __attribute__((address_space(4)))* CD4;

constexpr int DC_T = 4;            // terms per step of a sweep row: the rows' lists are padded to it (pad = factor value 0 x the zero row n of the scratch)
constexpr int DC_CHAIN_WAVES = 16; // a level of at most this many rows is "narrow": runs of narrow levels are ONE launch (workgroup barriers between levels)
constexpr int DC_FLOW_BRANCHES = 32;    // branches per wave of the flow kernel
// policy bits 8-15 = 255: no pivot goes to a top task (jg_symbolic.hpp), every pivot is a level item.  The JG_TOP_LEVEL test knob can override that
// byte; the top tasks it would add are further replay tables -- the generic lists read here (t_ptr / t_a / t_d / t_b, e_level, l_* / u_*, bwd_level)
// are complete before build_top runs and neither it nor build_tables changes them, so the factor is the same with the knob set.
constexpr long long DC_POLICY_NO_TOP = (long long)255 << 8;

struct DcSweepTables {             // one triangle of the factor, rows grouped by dependency level
    int* rows = nullptr;           // [n] pivots, level-major
    int* lev = nullptr;            // [levels + 1] offsets into rows
    int* ptr = nullptr;            // [n + 1] offsets of the padded term lists (multiples of DC_T)
    int* col = nullptr;            // [terms] pivot of the operand row (n = the zero row)
    double* val = nullptr;         // [terms] premultiplied factor value, in list order (k_dc_compact)
    int* ent = nullptr;            // [terms] factor entry of a term and the pivot whose diagonal divides it: kept only by a handle that refactorises
    int* dpiv = nullptr;
    std::vector<int> h_lev;
    long long terms = 0;
    struct Launch { int l0, l1, chain; };     // levels [l0, l1): a chain launch, or one wide level
    std::vector<Launch> launches;
};

// the factor A = Lh D^-1 U of one matrix in its own order (buses / states); a handle that never refactorises releases the factorisation tables, A, X and bad
// after its create call
struct DcFactor {
    int n = 0, n_entries = 0, n_fact_levels = 0;
    int* perm = nullptr;                                    // [n] pivot -> row of the matrix
    int* f_ent = nullptr; std::vector<int> f_lev;           // entries by factorisation level
    int* t_ptr = nullptr; int* t_a = nullptr; int* t_d = nullptr; int* t_b = nullptr;
    int* e_src = nullptr; int* diag = nullptr;
    double* A = nullptr;                                    // [nnz] row-CSR values: the caller's
    double* X = nullptr;                                    // [n_entries + 1] factor
    double* dinv = nullptr;                                 // [n]
    int* bad = nullptr;                                     // zero / non-finite pivot flag
    DcSweepTables fwd, bwd;
};

// what a handle allocates and reports through: DcHandle and DcseHandle derive from it
struct DcDevice {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;
    std::vector<void*> allocs;                              // everything the handle owns on the device
};

struct DcSweepArgs {
    const int* rows; const int* lev; const int* ptr; const int* col; const double* val;
    const int* perm; const double* dinv;
    const double* rhs;                  // MODE 0: [n][ld], bus order
    const int* of; const int* ot;       // MODE 1: the lanes' outage buses (-1: none / the slack): the right-hand side e_from - e_to is formed here
    double* W;                          // [n + 1][ld], pivot order; row n stays zero
    double* out;                        // MODE 2: [n][ld], bus order
    const int* groups;                  // nullable: the lane groups this launch works on
    int ld, l0, l1;
};
struct DcFlowArgs {
    const double* TH; const int* bf; const int* bt; const double* by; const double* bs; const double* rating;    // rating nullable
    const int* obr;
    const int* obr2;                    // nullable: the lanes' second outaged branch (-1: none)
    double* flows;                      // nullable [nbr][ld]
    double* part;                       // [chunks][4][ld]: worst loading, its branch, largest |from|, its branch
    int nbr, ld;
    const int* preorder; const I4* isl; // ISL: DFS preorder number per bus; per lane (S end, lo, hi, side) of a bridge outage solved on the slack's island
};

#define DC_HIP(expr)                                                                      \
    do {                                                                                  \
        hipError_t err__ = (expr);                                                        \
        if (err__ != hipSuccess) {                                                        \
            h->error = std::string(#expr) + ": " + hipGetErrorString(err__);              \
            return 2;                                                                     \
        }                                                                                 \
    } while (0)
#define DC_TRY(expr) do { const int rc__ = (expr); if (rc__) return rc__; } while (0)

template <typename T>
int dev_alloc(DcDevice* h, T** p, size_t count, const T* src = nullptr, bool zero = false) {
    void* q = nullptr;
    DC_HIP(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
    h->allocs.push_back(q);
    *p = (T*)q;
    if (src && count) DC_HIP(sync_copy(q, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
    else if (zero && count) DC_HIP(sync_fill(q, 0, count * sizeof(T), h->stream));
    return 0;
}
// frees what only a create call needed (factorisation tables, the unfactorised values)
template <typename T>
void dev_release(DcDevice* h, T*& p) {
    if (!p) return;
    h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), (void*)p), h->allocs.end());
    hipFree((void*)p);
    p = nullptr;
}

// device tables of the factorisation (entries by dependency level, update terms) for the analysis S of an n x n pattern; the values F.A [nnz] are the caller's
int factor_tables(DcDevice* h, DcFactor& F, int n, const BlockSymbolic& S);
// numeric factorisation of F.A into F.X, F.dinv: a launch per dependency level; F.bad collects zero / non-finite pivots
void factor_numeric(const DcFactor& F, hipStream_t stream);
// dependency levels of the forward sweep's rows
std::vector<int> forward_levels(int n, const BlockSymbolic& S);
// term lists of one triangle (F.fwd or F.bwd), rows grouped by level, lists padded to DC_T; `keep`: the entry maps stay for a later numeric refactorisation
int build_sweep(DcDevice* h, const DcFactor& F, DcSweepTables& T, const std::vector<int>& level, const std::vector<int>& lptr, const std::vector<int>& lent,
                const std::vector<int>& lcol, bool upper, bool keep = false);
// the sweeps' values of one triangle from the factor F.X, F.dinv
void compact_sweep(const DcFactor& F, const DcSweepTables& T, hipStream_t stream);
// x = M^-1 r on the shared factor for `groups` lane groups (glist nullable: groups 0 .. groups - 1): mode_f 0 (r = rhs, [n][ld] in the matrix's own
// order) or 1 (r = e_from - e_to of the lanes in of / ot); W is the [n + 1][ld] scratch in pivot order, out [n][ld] in the matrix's own order
void sweep_pair(const DcFactor& F, hipStream_t stream, int mode_f, const double* rhs, const int* of, const int* ot, double* W, double* out, int ld, int groups,
                const int* glist);
// branch flows and the partial screen records of every lane, DC_FLOW_BRANCHES branches per wave: grid = (chunks of branches / 4, lane groups).  isl: a
// lane whose outage sheds the buses with preorder numbers lo .. hi (their angles are NaN) carries 0 on every branch with an end among them
void launch_dc_flows(const DcFlowArgs& a, bool isl, dim3 grid, hipStream_t stream);

}  // namespace jg
