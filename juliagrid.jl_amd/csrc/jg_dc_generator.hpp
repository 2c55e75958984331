// jg_dc_generator.hpp -- the DC generator-outage screen: the loss of a generating unit alone (G-1) and with a branch candidate out of service beside it
// (generator x branch), on the ONE factor of a DcHandle (jg_dc.hpp) and the outage sensitivities a DcPhi keeps (jg_dc_phi.hpp).
//
// Reference counterpart: the user loop
//     for g in generators: updateGenerator!(system, analysis; label = g, status = 0); solve!; power!                        (row 0: G-1)
//       for k in branches: updateBranch!(...; label = k, status = 0); solve!; power!; updateBranch!(...; status = 1)        (row k)
//     updateGenerator!(...; label = g, status = 1)
// The loss of unit g moves the right-hand side alone: rhs_g = rhs + A[:,g], where column g of the sparse A [distinct generator buses x G] is the net
// change of the bus injections -- -Pg at g's bus, and what the units that pick the loss up add at theirs (nothing: the slack takes it, the reference's
// semantics).  The slack's own row is not in A: its entry of a right-hand side is dropped.  With Psi[m,b] = y_m a_m' B^-1 e_b, the flow on row m per unit
// of injection at bus b (no shift angle: the form Phi has), and the base flows f0:
//     F0[m,g]  = f0[m] + sum_b Psi[m,b] A[b,g]                 the flows of the G-1 case g: ONE sweep pair per distinct generator bus, never per generator
//     f_m(k,g) = F0[m,g] + Phi[m,k] F0[k,g] / (1 - Phi[k,k])   the series screen's arithmetic (jg_dc_series.hpp) with F0's columns for the profiles
// so the (k, g) screen IS k_series_screen, launched on this state's arrays through dc_series_launch_screen, shed mode included: a bridge candidate is
// solved on the slack's island for every column, and a unit that sits behind the bridge leaves with it -- its column is then the shed case without
// the outage, because what the buses behind the bridge inject never enters what is left.
//
// What is kept: Phi [rows][ldk] (a DcPhi of the screen's own), Psi [rows][ldb] (ldb = distinct generator buses rounded up to 64), A in CSC, and
// F0 [rows][ldg] (ldg = G rounded up to 64, 0 behind G).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "jg_dc_records.hpp"

namespace jg {

constexpr int DC_GEN_FLOW_ROWS = 8;          // rows of F0 a wave of k_gen_flows keeps in registers: an entry of A is loaded once for all of them

struct DcGeneratorState {
    DcPhi phi;                               // Phi and the row / candidate tables of the shared build
    int G = 0, ldg = 0;                      // generator outages (columns), rounded up to 64
    int nb = 0, ldb = 0;                     // distinct generator buses that get a sweep pair (the slack is none of them), rounded up to 64
    long long nnz = 0;
    double* Psi = nullptr;                   // [rows][ldb]
    int* a_ptr = nullptr; int* a_row = nullptr; double* a_val = nullptr;            // A in CSC: [ldg + 1] (flat behind G), [nnz] rows < nb, [nnz]
    double* F0 = nullptr;                    // [rows][ldg]
    int* walk_label = nullptr;               // [ldk + 1] labels of the walk's rows: 0 (row 0, the G-1 cases), then the candidates'
    std::vector<char> h_bridge;              // [nk] 1: |1 - Phi[k,k]| < DC_SINGULAR
    // the row block of a screen call (grown on demand); blk_rows counts the rows of the WALK: the candidates' and row 0
    int blk_rows = 0;
    double* b_load = nullptr; int* b_branch = nullptr; int* b_count = nullptr;      // [blk_rows][ldg]
    double* r_max = nullptr;                 // [blk_rows]
    double* c_max = nullptr; int* c_viol = nullptr;                                 // [ldg] over the block's candidates, per generator
    double* base = nullptr;                  // [ldg][3] the G-1 cases: worst loading, its branch, the count
    DcRecords viol{5 * sizeof(double)};      // the violators [5]
    double build_ms[4] = {0, 0, 0, 0};       // the last build: Psi total, its sweep pairs, its flow kernel; k_gen_flows (HIP events)
    DcMem mem;                               // the device memory of the fields above (not the DcPhi's): what release frees
};

void dc_generator_free(DcHandle* h);         // releases what the generator screen holds (jg_dc_destroy, jg_dc_generator_release)

}  // namespace jg
