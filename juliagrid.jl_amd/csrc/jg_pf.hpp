// jg_pf.hpp -- the polar power-flow equations, stated ONCE for the kernels that need them (jg_nr.hip: k_assemble, k_assemble1, k_refine_residual,
// k_branch_quantities, k_screen_partial; jg_comp.hip: k_comp_fix).  Arithmetic on values the caller holds in registers: no stores, no sincos, and no loads but
// those of patched<MP>.  The refinement residual is f - J d against the J the assembly wrote, the shared-factor first step J_s - J_0 of that same J: they agree
// to the bit because they call the same functions.  tools/pf_check.cpp checks every formula on the host (tests/test_pf_equations_cpu.py).
// Reference (relative to its src/): backend/equations.jl:63-144, powerFlow/acPowerFlow.jl:645-685, postprocessing/acAnalysis.jl:891-931.
#pragma once
#include "jg_engine.hpp"

namespace jg { namespace pf {
#define JG_PF __host__ __device__ __forceinline__
// Ybus entry (i, j) = g + j b at theta_i - theta_j (sine s, cosine c): ac = G cos + B sin, ad = G sin - B cos   equations.jl:63-103
// WHICH product is fused is written out: left to contraction the compiler fused g * c in one caller, b * s in another, and the callers disagreed in the last bit
struct Terms { double ac, ad; };
JG_PF Terms entry_terms(double g, double b, double s, double c) { return Terms{__builtin_fma(g, c, b * s), __builtin_fma(g, s, -(b * c))}; }
// Off-diagonal block (i, j).  mk: bit0 dP/dth, bit1 dP/dV, bit2 dQ/dth, bit3 dQ/dV exist (rows: P unless slack, Q for PQ; columns: theta unless slack, V for PQ)
JG_PF Blk offdiag(int mk, double vi, double vj, double ac, double ad) {
    return Blk{(mk & 1) ? vi * vj * ad : 0.0,            // dP_i/dtheta_j   equations.jl:109-111
               (mk & 2) ? vi * ac : 0.0,                 // dP_i/dV_j       equations.jl:117-119
               (mk & 4) ? -(vi * vj) * ac : 0.0,         // dQ_i/dtheta_j   equations.jl:134-136
               (mk & 8) ? vi * ad : 0.0};                // dQ_i/dV_j       equations.jl:142-144
}
// Row i closed over its sums s1 = sum_j V_j ac_ij, s2 = sum_j V_j ad_ij (j = i included): the diagonal block and the mismatch
struct Row { Blk d; double fp, fq; };
JG_PF Row row_closure(double vi, double s1, double s2, double gii, double bii, double pinj, double qinj) {
    return Row{Blk{-vi * s2 - bii * (vi * vi),           // dP_i/dtheta_i   equations.jl:105-107, acPowerFlow.jl:872
                   s1 + gii * vi,                        // dP_i/dV_i       equations.jl:113-115
                   vi * s1 - gii * (vi * vi),            // dQ_i/dtheta_i   equations.jl:130-132
                   s2 - bii * vi},                       // dQ_i/dV_i       equations.jl:138-140
               vi * s1 - pinj, vi * s2 - qinj};          // acPowerFlow.jl:676, 679
}
// Padding by bus type (1 PQ, 2 PV, 3 slack): a row that is no equation gets `one` on the diagonal and a zero mismatch.  one = 1: identity rows (the assembling
// kernels); one = 0: what such a row adds to a DIFFERENCE of two Jacobians (k_comp_fix).  (Through a Row& the stores are merged and the Row ends in scratch.)
JG_PF Row pad(int ti, double one, const Row& r) {
    double d00 = r.d.v00, d01 = r.d.v01, d10 = r.d.v10, d11 = r.d.v11, fp = r.fp, fq = r.fq;
    if (ti == 3) { d00 = one; d01 = 0.0; d10 = 0.0; d11 = one; fp = 0.0; fq = 0.0; }
    else if (ti == 2) { d01 = 0.0; d10 = 0.0; d11 = one; fq = 0.0; }
    return Row{Blk{d00, d01, d10, d11}, fp, fq};
}
// NaN-propagating maximum of x and the running maximum m: a NaN mismatch must not look converged
JG_PF double nanmax(double x, double m) { return (x > m || x != x) ? x : m; }
// Both ends of a branch from y = param[0..7] = {yff, yft, ytf, ytt} (re, im), |V| and sin / cos of the angle at the two buses: the rectangular voltages, the
// currents Iij = Vi yff + Vj yft, Iji = Vi ytf + Vj ytt (acAnalysis.jl:921-927) and the powers Sij = Vi conj(Iij), Sji = Vj conj(Iji) (:898-904)
struct TwoPort { double y[8]; };
struct BranchEnds { double vir, vii, vjr, vji, ifr, ifi, itr, iti, pf, qf, pt, qt; };
JG_PF BranchEnds branch_ends(TwoPort t, double Vi, double Vj, double si, double ci, double sj, double cj) {
    const double* p = t.y;
    BranchEnds e;
    e.vir = Vi * ci; e.vii = Vi * si; e.vjr = Vj * cj; e.vji = Vj * sj;
    e.ifr = e.vir * p[0] - e.vii * p[1] + e.vjr * p[2] - e.vji * p[3]; e.ifi = e.vir * p[1] + e.vii * p[0] + e.vjr * p[3] + e.vji * p[2];
    e.itr = e.vir * p[4] - e.vii * p[5] + e.vjr * p[6] - e.vji * p[7]; e.iti = e.vir * p[5] + e.vii * p[4] + e.vjr * p[7] + e.vji * p[6];
    e.pf = e.vir * e.ifr + e.vii * e.ifi; e.qf = e.vii * e.ifr - e.vir * e.ifi;
    e.pt = e.vjr * e.itr + e.vji * e.iti; e.qt = e.vji * e.itr - e.vjr * e.iti;
    return e;
}
// Ybus entry p of scenario b with its edits applied: g += pdg[m], bb += pdb[m] where ppos[m] == p (ppos: the caller's registers; pdg, pdb [MP][ld])
template <int MP>
JG_PF void patched(int p, const int* ppos, const double* pdg, const double* pdb, size_t ld, size_t b, double& g, double& bb) {
#pragma unroll
    for (int m = 0; m < MP; ++m)
        if (ppos[m] == p) { g += pdg[(size_t)m * ld + b]; bb += pdb[(size_t)m * ld + b]; }
}
#undef JG_PF
} }  // namespace jg::pf
