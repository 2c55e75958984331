// jg_qlim.hpp -- reactive-power limits per scenario of a batched Newton-Raphson handle (reactiveLimit!, acPowerFlow.jl:1081-1155) and adjustAngle!
// per lane (acPowerFlow.jl:1196-1206).  The tables are uploaded once (jg_nr_set_generators); the kernels work on the handle's [row][ld] lane arrays.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

namespace jg {

struct QlimTables {
    int n = 0, ng = 0, nbg = 0, ld = 0;                 // buses, generators, buses with an in-service generator, lanes of the scratch below
    double base_mva = 100.0;                            // base power in MVA (the 10 eps test of the proportional Q split, acAnalysis.jl:84-166)
    // lane-independent tables (host-built)
    int* gb_bus = nullptr;                              // [nbg] bus (0-based) of generator bus g
    int* gb_ptr = nullptr;                              // [nbg + 1] its in-service generators in g_list, label order
    int* g_list = nullptr;                              // [sum] generator indices
    int* g_bus = nullptr;                               // [ng] bus of generator k (0-based)
    int* g_gbi = nullptr;                               // [ng] generator bus of k (-1: out of service)
    int* b_gbi = nullptr;                               // [n] generator bus of bus i (-1: none)
    double* g_pg = nullptr; double* g_qmin = nullptr; double* g_qmax = nullptr;   // [ng] gen.output.active, capability limits
    double* gb_qmins = nullptr; double* gb_qmaxs = nullptr;                      // [nbg] sums of the FINITE limits of the bus's generators
    double* b_vg = nullptr; double* b_vm = nullptr; double* b_va = nullptr;      // [n] initial point: set-point of the first in-service generator (bus.voltage where none), bus.voltage
    double* b_pd = nullptr; double* b_qd = nullptr;                              // [n] demand
    // per-lane scratch (sized for ld lanes)
    int* conv = nullptr;                                // [nbg][ld] the generator at which the bus turns PQ (INT_MAX: it does not)
    int* slack_conv = nullptr;                          // [ld] ... that of the lane's slack bus
    signed char* VO = nullptr;                          // [ng][ld] the violate vector of reactiveLimit!
    double* SP = nullptr; double* SQ = nullptr;         // [nbg][ld] bus.supply of the generator buses
    int* cnt = nullptr; int* dead = nullptr;            // [ld] violations, no slack left
    unsigned long long* lt_bak = nullptr;               // [ceil(n / 32)][ld] the lane types before the walk (restored where no slack is left)
    bool ready() const { return gb_bus != nullptr; }
    void destroy();
};

// Builds and uploads the tables (status: int8 1 = in service); 0 or an error code with msg set
int qlim_setup(QlimTables& t, int n, int ld, int ng, const int64_t* bus, const int8_t* status, const double* pg, const double* qmin, const double* qmax,
               const double* vg, const double* bus_vm, const double* bus_va, const double* pd, const double* qd, double base_mva, hipStream_t s, std::string& msg);

// reactiveLimit! for lanes [0, batch) except those with skip_dev[b] != 0.
//   pq: [n][ld][2] the calculated injections P_i, Q_i of every lane (the mismatch pass's pq_out); lt: the lane types (changed in place);
//   p, q: the lane injections [n][ld] (written for the generator buses of lanes that keep a slack); vm, va: reset to the initial point of the
//   lanes with a violation when restart is set.  Outputs in t.VO, t.cnt, t.dead.
void qlim_launch(QlimTables& t, const double* pq, unsigned long long* lt, double* p, double* q, double* vm, double* va, const int* skip_dev,
                 int batch, int ld, bool restart, hipStream_t s);

// adjustAngle!: va[., b] += angle - va[bus, b] for b < batch (shift: [ld] scratch)
void adjust_angle_launch(double* shift, double* va, int n, int ld, int batch, int bus, double angle, hipStream_t s);

}  // namespace jg
