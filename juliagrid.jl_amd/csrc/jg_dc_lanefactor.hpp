// jg_dc_lanefactor.hpp -- internal: a LANE-VALUED scalar factorisation with lane-valued sweeps on the shared symbolic tables of jg_dc_sweep.hpp.
//
// The shared factor (DcFactor) holds ONE set of values for every lane; the per-lane block-LU engine (jg_engine) holds per-lane values of the AC Jacobian's
// 2x2 blocks.  This is the piece between them: the pattern, elimination order, update terms and dependency levels of one scalar matrix are analysed
// once (factor_tables / forward_levels / build_sweep(..., keep = true) of jg_dc_sweep.hpp, unchanged), the VALUES are held per lane, lane-fastest:
//     A    [nnz][ld]             the matrix, row-CSR entries
//     X    [n_entries + 1][ld]   the factor; entry n_entries is a zero row that stays zero (the operand of the sweep lists' padding)
//     dinv [n][ld]               1 / pivot
//     bad  [ld]                  1 where a lane met a zero or non-finite pivot (dc_bad_pivot below)
// ld is the batch padded to 64.  Entry and term indices are wave-uniform and go through the scalar cache (CInt of jg_dc_sweep.hpp); the values move
// through the vector pipe, 512 contiguous bytes per wavefront and operand.  Every store is a vector store from plain C++.
//
// The sweeps read the factor value of a term as X[ent][lane] * dinv[dpiv][lane]: two vector loads and a multiplication per term.  A premultiplied
// copy in list order (what compact_sweep keeps for the shared factor) would save one load per term and cost (fwd.terms + bwd.terms) x ld x 8 bytes --
// the padded lists hold every off-diagonal factor entry once, so that is about as much again as X itself -- and one more pass over the factor per
// factorisation.  An interior-point iteration factorises once and sweeps twice, so the copy would be read twice per write: it is not kept.
//
// Used by jg_dclav.hip (the gain H' Q H of the LAV iteration, Q per lane and iteration).
#pragma once
#include "jg_dc_sweep.hpp"

namespace jg {

// The pivot rule of the scalar DC factors: a pivot that is zero or not finite marks the matrix as singular.  k_dc_dinv of jg_dc_sweep.hip (the shared
// factor of jg_dc / jg_dcse) tests the same expression; that file is compiled as it stands, so the rule is restated here for the lane-valued factor.
__host__ __device__ inline bool dc_bad_pivot(double d) { return d == 0.0 || !(d - d == 0.0); }

#ifdef __HIPCC__
// the lane of a thread of a (64, waves) workgroup whose blockIdx.y walks lane groups: the group list is wave-uniform (nullable: group = blockIdx.y)
__device__ __forceinline__ size_t lane_of(const int* groups) {
    const int grp = groups ? ((CInt)groups)[blockIdx.y] : (int)blockIdx.y;
    return (size_t)grp * 64 + threadIdx.x;
}
#endif

struct DcLaneFactor {
    DcFactor sym;                       // the tables only (perm, f_ent, t_*, e_src, diag, fwd / bwd lists with ent / dpiv); its A, X, dinv, bad are not used
    int ld = 0, nnz = 0;
    double* A = nullptr; double* X = nullptr; double* dinv = nullptr; int* bad = nullptr;
};

// bytes of A, X, dinv and bad per lane
inline size_t lane_factor_bytes_per_lane(int nnz, int n_entries, int n) { return ((size_t)nnz + (size_t)n_entries + 1 + (size_t)n) * sizeof(double) + sizeof(int); }

// the tables of the analysis S of an n x n pattern with nnz entries and the lane values for ld lanes (zeroed)
int lane_factor_create(DcDevice* h, DcLaneFactor& F, int n, int nnz, const BlockSymbolic& S, int ld);
// numeric factorisation of F.A into F.X, F.dinv for `groups` lane groups (glist nullable: groups 0 .. groups - 1): a launch per dependency level, a
// thread per (entry, lane); F.bad of these lanes is cleared first and set where a pivot is bad
void lane_factor_numeric(const DcLaneFactor& F, hipStream_t stream, int groups, const int* glist);
// x = A^-1 r per lane: rhs and out [n][ld] in the matrix's own order, W the [n + 1][ld] scratch in pivot order whose row n is zero
void lane_sweep_pair(const DcLaneFactor& F, hipStream_t stream, const double* rhs, double* W, double* out, int groups, const int* glist);

}  // namespace jg
