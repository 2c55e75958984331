// jg_dc_group_lu.hpp -- the k x k solve of an outage set, stated ONCE for the kernels that need it: k_group_solve (jg_dc_group.hip, a lane = a group) and
// k_cascade (jg_dc_cascade.hip, where every wave repeats its lane's solve at every stage).  jg_dc_group.hpp has the algebra.
//
// The matrix lives in registers: every index below is a constant once the loops are unrolled, a row exchange is a select per entry (no array is indexed
// by a runtime value, which would send the matrix to scratch).  A slot behind the set's last member is an identity row and column with right-hand side 0:
// its pivot is 1 and its coefficient 0, so a set may grow from 1 to K members under one instance.  Partial pivoting: row j takes the entry of largest
// magnitude of column j among the rows i >= j (ties: the upper row stays).  A pivot below DC_SINGULAR in magnitude (a NaN too): the set is singular.
#pragma once
#include <hip/hip_runtime.h>

#include "jg_dc.hpp"

namespace jg {

// q [K]: the members as candidate positions, -1 behind the last.  x [K]: the coefficients c (0 on a slot without a member, 0 everywhere when singular).
// Returns true when the system is singular.
template <int K>
__device__ __forceinline__ bool dc_group_lu(const double* __restrict__ Phi, size_t ldk, const int* __restrict__ crow, const double* __restrict__ cf0,
                                            const int (&q)[K], double (&c)[K]) {
    int p[K];
    bool on[K];
    double A[K][K], b[K], x[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        on[i] = q[i] >= 0;
        p[i] = on[i] ? q[i] : 0;
        b[i] = on[i] ? cf0[p[i]] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double* prow = Phi + (size_t)crow[p[i]] * ldk;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double v = prow[p[j]];                         // Phi[s_i, s_j]: K gathers inside one row
            A[i][j] = (i == j ? 1.0 : 0.0) - ((on[i] && on[j]) ? v : 0.0);
        }
    }
    bool sing = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
            const bool sw = fabs(A[i][j]) > fabs(A[j][j]);
#pragma unroll
            for (int k = j; k < K; ++k) {
                const double u = A[j][k], w = A[i][k];
                A[j][k] = sw ? w : u; A[i][k] = sw ? u : w;
            }
            const double u = b[j], w = b[i];
            b[j] = sw ? w : u; b[i] = sw ? u : w;
        }
        const bool bad = !(fabs(A[j][j]) >= DC_SINGULAR);       // (a NaN is singular too)
        sing = sing || bad;
        if (bad) A[j][j] = 1.0;                                  // the lane goes on with finite numbers; its result is not delivered
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
            const double l = A[i][j] / A[j][j];
#pragma unroll
            for (int k = j + 1; k < K; ++k) A[i][k] = fma(-l, A[j][k], A[i][k]);
            b[i] = fma(-l, b[j], b[i]);
        }
    }
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        double s = b[j];
#pragma unroll
        for (int k = j + 1; k < K; ++k) s = fma(-A[j][k], x[k], s);
        x[j] = s / A[j][j];
    }
#pragma unroll
    for (int i = 0; i < K; ++i) c[i] = (sing || !on[i]) ? 0.0 : x[i];
    return sing;
}

}  // namespace jg
