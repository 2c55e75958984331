// jg_gs.hpp -- Gauss-Seidel AC power flow, one scenario per lane.
//
// Reference counterpart: gaussSeidel / mismatch! / solve! / powerFlow! (src/powerFlow/acPowerFlow.jl:563-619, 732-764, 985-1041, 1389-1433).  A sweep is
// strictly sequential over the buses of ONE scenario (every update reads the voltages the updates before it wrote), and scenarios never meet: a lane
// runs the reference's update sequence unchanged on its own column of the [n][ld] voltages (ld = batch rounded up to 64), a wavefront is 64 scenarios.
// The Ybus pattern and values are the same for every lane and reach the wave through the scalar cache; a lane's branch outage is 4 value positions and
// 4 complex deltas it holds in registers and adds where the walk meets one of the positions.  No barriers, no LDS, no atomics; every store is a vector
// store.
//
// Row i of Ybus is walked as the reference walks it: j in colptr[i] .. colptr[i + 1] - 1, the value nodalMatrixTranspose.nzval[j] = Y[i, rowval[j]].
#pragma once
#include <hip/hip_runtime.h>

#include "jg_dc_sweep.hpp"

namespace jg {

struct GsHandle : DcDevice {
    int n = 0, nnz = 0, batch = 0, ld = 0, npq = 0, npv = 0;
    int* rp = nullptr; int* ci = nullptr;                   // [n + 1], [nnz]: colptr and rowval of nodalMatrix, 0-based
    double* yr = nullptr; double* yi = nullptr;             // [nnz] nodalMatrixTranspose.nzval, re / im
    int* pq = nullptr; int* pv = nullptr;                   // [npq], [npv] buses in bus order, 0-based
    double* vg = nullptr;                                   // [npv] magnitude set-point of the first in-service generator of pv[k]
    std::vector<int> h_pv;
    double* vr = nullptr; double* vi = nullptr;             // [n][ld] method.voltage
    double* P = nullptr; double* Q = nullptr;               // [n][ld] supply - demand
    int* ppos = nullptr; double* pdr = nullptr; double* pdi = nullptr;   // [4][ld] a lane's outage: positions in yr / yi (-1: none) and what is added there
    int* iteration = nullptr; int* status = nullptr;        // [ld]
    double* stopP = nullptr; double* stopQ = nullptr;       // [ld] the maxima of the last mismatch
};

}  // namespace jg
