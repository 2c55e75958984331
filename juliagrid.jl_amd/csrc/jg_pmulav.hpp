// jg_pmulav.hpp -- batched PMU least-absolute-value state estimation: the interior-point iteration of jg_dclav.hpp on the linear phasor model, per lane.
//
// Reference counterpart: pmuLavStateEstimation / solve! (src/stateEstimation/pmuStateEstimation.jl:223-338, 474-512), where the model goes to a JuMP
// solver.  States: 2 n, re(1 .. n) then im(1 .. n).  Rows: two per PMU in device order, row 2 i the real and row 2 i + 1 the imaginary part of PMU i (0-based);
// a bus PMU has 1 on re_b resp. im_b, a branch PMU the pi-model's current coefficients on the four states of its two buses (the coefficient matrix of the
// WLS model, jg_gn's rows 22 .. 27).  Readings arrive polar and become z_re = magnitude cos(angle), z_im = magnitude sin(angle) on the device.  A PMU
// whose magnitude or angle channel is out of service leaves with both rows.  No state is fixed: phasors observe the angle reference themselves.
//     minimise  sum_i (u_i + v_i)   subject to   h_i x + u_i - v_i = z_i,  u, v >= 0          (= min |z - H x|_1, unweighted as in the reference)
// The iteration, its start, its three stopping tests, its frozen lanes and its group list are jg_dclav.hpp's, reached through lav_create (no added
// diagonal entry in the gain, no zeroed column, no offset).  An optional constant scale per row (jg_pmulav_set_scale, 1 / sigma of the stored readings'
// rectangular variances) multiplies z on the device; H is scaled by the caller.  It is ONE scale for every lane.
// Status: 0 solved, 5 iteration limit, 1 a state that no in-service row touches (an exact zero pivot of the unit-weight start: every lane, NaN), 3 a bad
// pivot in a later iteration of that lane.  A rank deficiency that leaves small non-zero pivots is NOT status 1: it ends as 3 or 5.
//
// Kernels of this file (lane-fastest [rows][ld], (64, 4) workgroups, blockIdx.y over lane groups, indices and coefficients wave-uniform):
//     k_pmu_rect     (PMU, lane)     polar reading -> the two rows of Z, one sincos
//     k_pmu_polar    (bus, lane)     (re, im) -> (magnitude, angle), hypot / atan2
//     k_pmu_branch   (branch, lane)  from / to current phasors and powers, series current and loss, charging power (pf::branch_ends of jg_pf.hpp on the
//                                    rectangular voltages); k_pmu_bus (bus, lane) sums a bus's branch ends in list order and adds the shunt
//     k_pmu_suspect  (PMU, lane)     rho = |unscaled residual phasor|, flag rho > threshold, per chunk the count and the largest rho with its device;
//                                    k_pmu_suspect_finish finishes both per lane over the chunks in ascending order (ties: the lowest device)
// All are bound by memory: each moves its operands once and does a handful of flops and at most one sincos / hypot / atan2 pair per element.
#pragma once
#include "jg_dclav.hpp"

namespace jg {

constexpr int PMULAV_DEVS = 32;                 // PMUs per wavefront in the suspect pass
constexpr int PMULAV_PLANES = 14;               // per (branch, lane): from I (mag, ang), to I, series I, from S (p, q), to S, series S, charging S

struct PmulavHandle : DclavHandle {             // n = 2 buses, m = 2 pmus
    int nbus = 0, npmu = 0, n_schunks = 0;
    std::vector<double> h_scale;                // [m]
    double* SC = nullptr;                       // [m] what a row's reading is multiplied by
    double* MAG = nullptr; double* ANG = nullptr;               // [npmu][ld] the polar readings
    double* VM = nullptr; double* VA = nullptr;                 // [nbus][ld]
    double* RHO = nullptr; int* FLAG = nullptr;                 // [npmu][ld]
    double* spart = nullptr;                    // [chunks][3][ld]: flagged devices, largest rho, its device
    int* CNT = nullptr; int* WORST = nullptr;   // [ld]
    // branches (jg_pmulav_set_branches)
    int* br_from = nullptr; int* br_to = nullptr; int* br_on = nullptr; double* br_par = nullptr;      // [nbr], [nbr][16] as jg_nr_set_branches
    int* e_ptr = nullptr; int* e_idx = nullptr;                 // per bus its branch ends, 2 branch + end, ascending
    double* sh_g = nullptr; double* sh_b = nullptr;             // [nbus]
    double* OUT = nullptr;                      // [PMULAV_PLANES][nbr][ld]
    double* INJ = nullptr;                      // [2][nbus][ld]
    double threshold = 0.0;                     // of the last suspect pass
    bool have_polar = false, have_flows = false;    // VM / VA resp. OUT / INJ hold the results of the last solve
};

}  // namespace jg
