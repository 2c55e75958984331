/*
 * jgrid.h -- C ABI of libjgrid_hip.so: MI355X-native Newton-Raphson AC power flow and Gauss-Newton
 * WLS state estimation inner loops, drop-in behind JuliaGrid's newtonRaphson()/mismatch!()/solve!()
 * and gaussNewton()/increment!()/solve!() (reference paths relative to /root/reference).
 *
 * Conventions
 *  - Every array argument is a HOST pointer owned by the caller and copied during the call; no
 *    pointer outlives the call.  Device memory lives behind the opaque handle.
 *  - Index arrays are the reference's own containers: 1-based int64, CSC (Julia SparseMatrixCSC).
 *  - `batch` independent scenarios of one grid are solved at once.  Per-scenario arrays are
 *    scenario-major on the host ([batch][n], C order); the library keeps them batch-minor in HBM.
 *  - Return codes: 0 ok, 1 bad argument, 2 HIP runtime error, 3 zero / non-finite pivot,
 *    4 stale model.  jg_last_error() gives the text of the last failure on this thread.
 *  - A handle is bound to one device and one HIP stream; handles are independent, a single handle
 *    is not thread-safe.  No global mutable state.
 */
#ifndef JGRID_H
#define JGRID_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jg_nr jg_nr;
typedef struct jg_nr_base jg_nr_base;
typedef struct jg_gn jg_gn;

const char* jg_last_error(void);
/* Number of visible HIP devices (<0 on runtime failure). */
int jg_device_count(void);
/* Engines that factorise the same block pattern under the same plan policy on the same device share ONE symbolic analysis and ONE
 * device copy of its replay tables through a process-wide cache (csrc/jg_engine.hpp: SharedPlan; the reference redoes its symbolic
 * factorisation in every newtonRaphson() / gaussNewton() call).  jg_plan_cache_clear drops the cache's own references -- live handles keep
 * their plans -- so that the next jg_*_create pays a full analysis again (benchmarks measure that cost with it).  JG_PLAN_CACHE=0 in the
 * environment switches the cache off. */
void jg_plan_cache_clear(void);

/* ---------------------------------------------------------------------------------------------
 * Newton-Raphson AC power flow
 * ------------------------------------------------------------------------------------------- */

/*
 * newtonRaphson(system)  -- src/powerFlow/acPowerFlow.jl:39-87 after initializeACPowerFlow (:1312-1331).
 * Builds the index maps pq/pvpq and the Jacobian CSC pattern exactly as newtonJacobian (:89-175),
 * runs the symbolic analysis that replaces the first `lu(J)` (src/backend/utility.jl:470-476),
 * and uploads the grid.
 *   n               number of buses
 *   colptr,rowval   Ybus pattern, system.model.ac.nodalMatrix (src/definition/system.jl:213-221)
 *   y_reim          nodalMatrix.nzval as (re,im) pairs, 2*nnz doubles
 *   yt_reim         nodalMatrixTranspose.nzval, same pattern (src/powerSystem/model.jl:75)
 *   type            bus.layout.type AFTER bus-type normalisation (1 PQ, 2 PV, 3 slack)
 *   slack           bus.layout.slack (1-based)
 *   batch           number of scenarios resident on this device (>= 1)
 *   max_patch       Ybus entries a scenario may override (4 per branch outage), >= 0
 *   device          HIP device ordinal
 */
int jg_nr_create(jg_nr** h, int64_t n, const int64_t* colptr, const int64_t* rowval,
                 const double* y_reim, const double* yt_reim, const int8_t* type, int64_t slack,
                 int64_t batch, int64_t max_patch, int device);
void jg_nr_destroy(jg_nr* h);

/* sizes: dims[0]=dimJ, dims[1]=nnz(J), dims[2]=nnz blocks of L+D+U, dims[3]=LU update terms,
 * dims[4]=launches per factorization (forward elimination fused in), dims[5]=launches per backward sweep */
int jg_nr_dims(jg_nr* h, int64_t* dims);

/* bus.supply - bus.demand per scenario (acPowerFlow.jl:676-680). [batch][n] each;
 * batch_stride 0 broadcasts one [n] vector to all scenarios. */
int jg_nr_set_injection(jg_nr* h, const double* p_inj, const double* q_inj, int64_t batch_stride);
/* analysis.voltage.{magnitude,angle} (setInitialPoint!, acPowerFlow.jl:1226-1249, 1281-1295). */
int jg_nr_set_voltage(jg_nr* h, const double* vm, const double* va, int64_t batch_stride);
int jg_nr_get_voltage(jg_nr* h, double* vm, double* va);
/* Device-resident start point: snapshot the current voltages inside HBM / restore them (the
 * setInitialPoint! of a benchmark or Monte-Carlo loop without a PCIe round trip). */
int jg_nr_snapshot_voltage(jg_nr* h);
int jg_nr_restore_voltage(jg_nr* h);
/* Same as jg_nr_get_voltage but into DEVICE buffers of the caller (e.g. for an RCCL gather):
 * vm_dev/va_dev are device pointers, [batch][n] doubles, written on the handle's stream and
 * synchronised before return. */
int jg_nr_get_voltage_device(jg_nr* h, double* vm_dev, double* va_dev);
/* The whole result of a batch as ONE device buffer, [batch][2 n + 2] doubles per scenario: V[n] | theta[n] | iterations |
 * status (the analysis.voltage / method.iteration a caller of powerFlow! reads, src/powerFlow/acPowerFlow.jl:1389-1433) --
 * the record a sharded screen gathers with a single collective. */
int jg_nr_pack_results_device(jg_nr* h, double* dst_dev);

/*
 * Per-scenario Ybus edit on top of the shared base matrix -- what acNodalUpdate!
 * (src/powerSystem/model.jl:81-110) does for updateBranch!(...; status = 0)
 * (src/powerSystem/branch.jl:344-350): k entries, ptr[] = 1-based pointers into nodalMatrix.nzval
 * (entry (row,col)); dy_reim = values ADDED to Y[row,col].  Pattern never changes (stored zeros).
 * Replaces any previous patch of that scenario; k = 0 clears it.
 */
int jg_nr_patch_ybus(jg_nr* h, int64_t scenario, int64_t k, const int64_t* ptr, const double* dy_reim);

/* The same for `count` consecutive scenarios starting at `scenario0` in one call (a contingency screen re-targets a
 * whole batch between solves): ptr [count][k], dy_reim [count][k][2]; ptr 0 = unused slot of that scenario. */
int jg_nr_patch_ybus_batch(jg_nr* h, int64_t scenario0, int64_t count, int64_t k, const int64_t* ptr, const double* dy_reim);

/* Re-upload the SHARED Ybus values after an in-place edit of the system (updateBranch!(analysis; ...),
 * src/powerSystem/branch.jl:453-459 -> acNodalUpdate!, model.jl:81-110).  Same pattern as at create. */
int jg_nr_set_ybus(jg_nr* h, const double* y_reim, const double* yt_reim);

/* mismatch!(analysis) -- acPowerFlow.jl:645-685. max_p/max_q: [batch] infinity norms. */
int jg_nr_mismatch(jg_nr* h, double* max_p, double* max_q);
/* solve!(analysis) -- acPowerFlow.jl:793-911: Jacobian fill, refactorization, solve, state update,
 * iteration += 1, for every scenario. */
int jg_nr_solve(jg_nr* h);
/* Guard of the static-pivot factorisation, opt-in.  mode 1: every Newton step (jg_nr_solve and the steps of jg_nr_run) is followed
 * by ONE step of iterative refinement, rho = f - J d, d += J^-1 rho, before the state moves -- what the reference gets from
 * UMFPACK's solve behind ldiv! (src/backend/utility.jl:576-586; UMFPACK refines by default, KLU does not).  J d is formed from
 * Ybus and the state (the factor has overwritten J); costs one more pass over the rows, a forward-only and a backward sweep
 * (~ +45 % per iteration).  Independent of the mode a pivot block that cancels to rounding level marks its scenario (status 3).
 * mode 0 (default): no refinement -- Newton's iteration corrects a rounding-level error of one step in the next.
 * Refinement writes the increment: mode 1 switches jg_nr_set_keep_increment back to 1 on a handle that had it at 0, and fails on such a handle while
 * it is paused (jg_nr_run_defer). */
int jg_nr_set_refine(jg_nr* h, int mode);
/* Performance hint, no counterpart in the reference (one analysis at a time).  mode 1: this handle is one of SEVERAL batches in flight on
 * its GPU (a pipeline of contingency batches): the multifrontal top of the factorisation always runs its 4-wave kernel variant, which
 * leaves room on a CU for the workgroups of the other batches (+2-3 % throughput with three 512-scenario batches in flight, -0.6 % for a
 * handle that runs alone).  Results are bitwise the same either way (tests/test_top_variants_gpu.py).  mode 0 (default): by the size of
 * each launch. */
int jg_nr_set_shared(jg_nr* h, int mode);
/* Performance switch, no counterpart in the reference.  mode 1 (default): every Newton step leaves method.increment in bus order for
 * jg_nr_get_increment, and a scenario's last increment travels with its lane.  mode 0: the batched sweeps (the refactorising iteration and the
 * first step on a shared base factor) write the increment in pivot order and into the state only -- 16 bytes x buses x lanes less per sweep and
 * per lane compaction; jg_nr_get_increment then fails (it never returns an older run's values).  V, theta, iteration counts and status are
 * bitwise the same either way (tests/test_sweep_diet_gpu.py).  Switching back to 1 holds from the next run; until that run jg_nr_get_increment
 * still fails.  jg_nr_set_refine(h, 1) switches the handle back to 1 (refinement writes the increment), and mode 0 is refused while refinement
 * is on or the handle is paused.  A single-instance handle accepts the switch but its sweep stores as before.  A pipeline of contingency batches
 * sets 0 on its batch and pool handles: it reads V, theta and branch records, never the increment. */
int jg_nr_set_keep_increment(jg_nr* h, int mode);
/* powerFlow!(analysis; iteration, tolerance) -- acPowerFlow.jl:1389-1433, per scenario, with the
 * reference's loop accounting.  iters/status: [batch]; status 0 converged, 1 iteration limit,
 * 3 numeric failure, 4 deferred to a pool (jg_nr_run_defer), 5 no slack bus left after jg_nr_reactive_limit (the reference's
 * errorSlackDefinition, src/powerFlow/acPowerFlow.jl:1151-1153; the scenario keeps its state and types, the others are unaffected). */
int jg_nr_run(jg_nr* h, int64_t max_iter, double tol, int32_t* iters, int32_t* status);
/* Straggler hand-off between batches of the same grid (no counterpart in the reference, which has no batch: its loop runs one
 * scenario at a time, acPowerFlow.jl:1389-1433).  A batch advances in lockstep until its slowest scenario is done; the last
 * iterations of 512 N-1 scenarios run on a few dozen of them at the latency of a full pass.  A pipeline of batches therefore
 * stops a batch once at most defer_at (<= 64) scenarios are active, moves those into a POOL handle that collects the stragglers of
 * several batches, and finishes them together:
 *   jg_nr_run_defer   jg_nr_run that returns as soon as <= defer_at scenarios are active (n_left of them; 0: the batch is done);
 *                     the handle is PAUSED: lanes packed, results not yet in home order.  Handles of one lane group never pause.
 *   jg_nr_move_lanes  the active scenarios of the paused handle src (state, injections, Ybus patch, iteration count) continue in
 *                     lanes dst_lane0.. of dst; home[i] = the scenario (lane of src) that went to lane dst_lane0 + i, count of them;
 *                     in src they end with status 4 (deferred).  Same grid, same device, dst must not be running.
 *   jg_nr_finish      ends a paused run: lanes home, iters / status [batch] (deferred scenarios: status 4).
 *   jg_nr_resume      runs the scenarios in lanes [0, lanes) of a pool to the end, each with the iteration count it arrived with
 *                     (per-scenario results are bitwise those of an undisturbed batch: lanes never interact, and jg_nr_move_lanes refuses
 *                     a pool that runs another factorisation plan than the batch -- the plan depends on the CLASS of batch a handle was
 *                     created for, decided by the scenario count PADDED to a multiple of 64 lanes: 64 lanes with at most 32 scenarios,
 *                     64 lanes (33-64 scenarios), 128 or 192 lanes (65-192), 256 lanes and more (193 scenarios and more: a batch of
 *                     200 is in the class of 512, not of 192); iters / status [lanes].
 *   jg_nr_pack_rows_device  V | theta | iterations | status of lanes lane0 .. lane0 + count - 1 into rows rows[i] of a result
 *                     record [.][2 n + 2] in device memory (the record jg_nr_pack_results_device writes for the batch they left). */
int jg_nr_run_defer(jg_nr* h, int64_t max_iter, double tol, int64_t defer_at, int32_t* n_left);
int jg_nr_move_lanes(jg_nr* dst, int64_t dst_lane0, jg_nr* src, int32_t* home, int32_t* count);
int jg_nr_finish(jg_nr* h, int32_t* iters, int32_t* status);
int jg_nr_resume(jg_nr* h, int64_t lanes, int64_t max_iter, double tol, int32_t* iters, int32_t* status);
int jg_nr_pack_rows_device(jg_nr* h, double* dst_dev, int64_t lane0, int64_t count, const int32_t* rows);

/*
 * The FIRST iteration of a batch whose scenarios all start from one state, on ONE shared factor (compensation method) -- what replaces, for the
 * user loop of an N-1 screen (src/powerSystem/branch.jl:453-459: updateBranch!(analysis; label, status = 0), setInitialPoint!, powerFlow!), the first
 * lu! + ldiv! of every scenario (src/powerFlow/acPowerFlow.jl:890-897; src/backend/utility.jl:478-484, 576-586).  At the common start the Jacobian of
 * scenario s is J_0 + E M_s F' with M_s the change of the <= 4 blocks of the two buses its Ybus edits touch, so its Newton step is
 *     x_s = J_0^-1 (f_s - E c_s),   c_s = M_s (I + S_s M_s)^-1 F' J_0^-1 f_s,   S_s = the 4 x 4 of J_0^-1 at those buses
 * -- one factorisation per BASE CASE instead of one per scenario; the batch pays a mismatch pass, a correction of <= 4 numbers per scenario and one
 * sweep pair whose factor values are shared (scalar loads).  Iterations >= 2 refactorise as before.  Results agree with the refactorising path to
 * rounding (the step is the same Newton step); a scenario whose 4 x 4 system is singular -- the outage islands a part of the grid -- ends with
 * status 3, like a cancelled pivot of the batched factorisation.
 *   jg_nr_base_create   `single`: a handle with batch = 1 whose CURRENT nodal matrix, injections and voltages are the base case and the common
 *                       start (e.g. its converged power flow).  Factorises its Jacobian once, forms J_0^-1 f_0, the blocks of J_0^-1 on the Ybus
 *                       pattern and the dense inverse of the top of the elimination tree (top_cap: at most this many pivots there; 0 = default
 *                       512, < 0 = none: every level a launch).  The base keeps copies: `single` may be reused or destroyed afterwards.
 *                       rc 3: the base Jacobian is singular.
 *   jg_nr_base_destroy  releases the caller's reference (the memory goes when the last attached handle lets go).
 *   jg_nr_attach_base   the scenarios of h may start from this base (same grid, bus types and device; NULL detaches).  jg_nr_set_ybus detaches.
 *   jg_nr_start_from_base   V, theta of EVERY scenario of h = the base's start (device-side broadcast; replaces jg_nr_restore_voltage in the loop).
 *   jg_nr_run / jg_nr_run_defer then take the shared-factor iteration BY THEMSELVES when (a) the state is untouched since jg_nr_start_from_base,
 *                       (b) every scenario's Ybus edits (jg_nr_patch_ybus*) lie in the rows / columns of at most two buses joined by an edited
 *                       entry -- a branch outage or parameter change, a shunt change --, (c) scenarios with edits keep the base's injections
 *                       (checked on the device once per jg_nr_set_injection; scenarios WITHOUT edits may have any injections: Monte-Carlo
 *                       variations solve J_0 x = f_s directly), (d) no refinement (jg_nr_set_refine); otherwise they refactorise as always.
 *   jg_nr_set_first_iteration   mode 0: always refactorise (the A/B switch of bench.py's value_full_refactor); 1 (default): as above.
 *   jg_nr_first_iteration_counts   how many runs of h started the one way / the other (NULL: not wanted).
 *   jg_nr_base_info     info[8] = pivots in the dense top, forward level above which a pivot belongs to it, forward / backward level launches of a
 *                       sweep pair, the same two without a top (the set-up solver), creation time in microseconds, attached handles.
 *   jg_nr_base_get      test access: which = 0 J_0^-1 on the Ybus pattern [nnz][4] (row-CSR position (i, j) of the stored pattern: block
 *                       (theta_i, V_i) x (P_j, Q_j), row-major), 1 J_0^-1 f_0 [n][2], 2 f_0 [n][2], 3 the dense inverse of the top's Schur
 *                       complement in the fragment order of the kernel that applies it (csrc/jg_comp.hip: k_ctop), 4 the compact factor [entries][4].
 */
int jg_nr_base_create(jg_nr_base** out, jg_nr* single, int64_t top_cap);
void jg_nr_base_destroy(jg_nr_base* b);
int jg_nr_base_info(jg_nr_base* b, int64_t* info);
int jg_nr_base_get(jg_nr_base* b, int which, double* out, int64_t cap);
int jg_nr_attach_base(jg_nr* h, jg_nr_base* b);
int jg_nr_start_from_base(jg_nr* h);
int jg_nr_set_first_iteration(jg_nr* h, int mode);
int jg_nr_first_iteration_counts(jg_nr* h, int64_t* compensated, int64_t* refactorised);

/* analysis.method.{mismatch,increment,jacobian.nzval} in the reference's own ordering
 * (rows/cols pvpq then pq; CSC of newtonJacobian).  [batch][dimJ] / [batch][nnzJ]. */
int jg_nr_get_mismatch(jg_nr* h, double* mism);
int jg_nr_get_increment(jg_nr* h, double* incr);
int jg_nr_get_jacobian(jg_nr* h, double* nzval);
/* analysis.method.{pq,pvpq,pcount} and jacobian.{colptr,rowval} (1-based, bit-exact). */
int jg_nr_get_maps(jg_nr* h, int64_t* pq, int64_t* pvpq, int64_t* pcount, int64_t* jcolptr, int64_t* jrowval);
/* analysis.method.iteration per scenario. */
int jg_nr_get_iteration(jg_nr* h, int32_t* iters);

/*
 * Bus types per scenario of a batched handle (batch >= 2, not fast Newton-Raphson, no iterative refinement).  The symbolic analysis, the factor
 * pattern and the plan depend on the Ybus pattern alone; a type that differs per scenario is a change of VALUES in the same plan: the assembly reads
 * the types of its lane (2 bits per bus in the lane layout, moved with the lanes by the compaction) and pads PV / slack rows and columns with identity
 * as for the create-time types, and every variable is updated (a masked one has an increment of exactly 0).  While any scenario has types of its own,
 * jg_nr_get_jacobian / _mismatch / _increment / _maps (reference layout: depends on the types), jg_nr_set_refine(h, 1), jg_nr_move_lanes and
 * jg_nr_fast_setup return 1; the next run after a change refactorises (no first iteration on an attached base's factor).
 *   jg_nr_set_bus_type  scenarios scenario0 .. scenario0 + count - 1 take type [count][n] (1 PQ, 2 PV, 3 slack; exactly one slack per scenario);
 *                       type == NULL: the create-time types again.  Replaces, per scenario, what reactiveLimit! does to system.bus.layout.type
 *                       and the newtonRaphson(system) built on it (src/powerFlow/acPowerFlow.jl:39-87, 1081-1155).  Refused (1): a fast handle,
 *                       a handle of batch 1, a scenario without exactly one slack.
 *   jg_nr_get_bus_type  type [batch][n] (nullable) and the 1-based slack bus of every scenario, slack [batch] (nullable).
 */
int jg_nr_set_bus_type(jg_nr* h, int64_t scenario0, int64_t count, const int8_t* type);
int jg_nr_get_bus_type(jg_nr* h, int8_t* type, int64_t* slack);

/*
 * reactiveLimit!(analysis) (src/powerFlow/acPowerFlow.jl:1081-1155) for EVERY scenario of a batched handle, on the device (csrc/jg_qlim.hip).
 *   jg_nr_set_generators  one-time set-up: the generator table in label order -- bus [ng] 1-based, status [ng] (1 in service), pg (gen.output.active),
 *                         qmin, qmax (gen.capability, may be infinite), vg (gen.voltage.magnitude) -- and the buses' bus_vm, bus_va (bus.voltage),
 *                         pd, qd (bus.demand) [n], base_mva = system.base.power in MVA.  The per-bus generator lists and their finite Q-limit sums
 *                         are built here; the initial point is that of initializeACPowerFlow / setInitialPoint! (acPowerFlow.jl:1226-1249, 1312-1358).
 *   jg_nr_reactive_limit  per scenario (not those left without a slack before): the generator outputs of generatorPower
 *                         (src/postprocessing/acAnalysis.jl:538-633) at the scenario's state, bus.supply with the slack's P from that state, the
 *                         violating PV / slack buses turned PQ with Q pinned at the limit, the slack handed over to the first bus that is PV at that
 *                         point of the reference's loop; the new types and the P / Q injections of the generator buses are written to the lanes.
 *                         flags & 1: the scenarios with a violation restart from the initial point under their NEW types (the newtonRaphson(system)
 *                         the reference's user builds next); the others keep their state (the next jg_nr_run confirms them in 0 iterations).
 *                         violate [batch][ng] (nullable): -1 / 0 / +1 per generator, the reference's return value; count [batch] (nullable): violations.
 *                         A scenario left without a slack keeps its types and state and reports status 5 from the next run on.
 *   jg_nr_adjust_angle    adjustAngle!(analysis; slack = bus) (acPowerFlow.jl:1196-1206) per scenario: theta += angle - theta[bus] (bus 1-based,
 *                         angle = system.bus.voltage.angle of that bus), on the device state.
 */
int jg_nr_set_generators(jg_nr* h, int64_t ng, const int64_t* bus, const int8_t* status, const double* pg, const double* qmin, const double* qmax,
                         const double* vg, const double* bus_vm, const double* bus_va, const double* pd, const double* qd, double base_mva);
int jg_nr_reactive_limit(jg_nr* h, int flags, int8_t* violate, int32_t* count);
int jg_nr_adjust_angle(jg_nr* h, int64_t bus, double angle);

/*
 * Fast Newton-Raphson (fastNewtonRaphsonBX / XB) on the same handle -- acPowerFlow.jl:215-537 (model), 687-730
 * (mismatch!), 913-983 (solve!), 1389-1433 (powerFlow!).  The two constant matrices are factorised ONCE on the device
 * (as one block matrix diag(B', B'') per bus pair) and every iteration is two forward/backward sweeps.
 * jg_nr_fast_setup: bp, bq [nnz of Ybus] = B'[pvpq r, pvpq c] and B''[pq r, pq c] of the stored Ybus entry (r, c) at
 *   that CSC pointer (fastNewtonJacobian!, :407-447), identity on the diagonal / zero elsewhere for rows and
 *   columns that are not in the reduced matrices (slack; PV buses in B'').  Shared by all scenarios of the batch.
 * jg_nr_fast_mismatch / _solve / _run mirror jg_nr_mismatch / _solve / _run; jg_nr_get_mismatch returns
 *   [active.mismatch | reactive.mismatch], jg_nr_fast_get_increment [active.increment | reactive.increment].
 */
int jg_nr_fast_setup(jg_nr* h, const double* bp, const double* bq);
/* Fast Newton-Raphson under BATCHED outages -- _updateBranch!(::AcPowerFlow{<:FastNewtonRaphson}), src/powerSystem/branch.jl:477 with
 * fastNewtonJacobian! / Pijtheta*, QijV* (acPowerFlow.jl:416-537): the reference edits the entries of B' and B'' a branch touches and refactorises.
 * Here scenario scenario0 + s keeps the shared matrices of jg_nr_fast_setup plus up to k <= 4 edits: ptr [count][k] 1-based pointers into the stored
 * Ybus pattern (0 = unused slot), dbp / dbq [count][k] what is ADDED to B' / B'' at that entry (0 where the entry is not in the reduced matrix).
 * Replaces the edits of those scenarios, keeps the others', then rebuilds and factorises the whole batch ONCE; the iterations are solves only.
 * The Ybus side of the same outage (the mismatches) is jg_nr_patch_ybus_batch.  A scenario whose edited matrix is singular comes back from
 * jg_nr_fast_run with status 3; jg_nr_fast_setup drops all edits. */
int jg_nr_fast_patch_batch(jg_nr* h, int64_t scenario0, int64_t count, int64_t k, const int64_t* ptr, const double* dbp, const double* dbq);
int jg_nr_fast_mismatch(jg_nr* h, double* max_p, double* max_q);
int jg_nr_fast_solve(jg_nr* h);
int jg_nr_fast_run(jg_nr* h, int64_t max_iter, double tol, int32_t* iters, int32_t* status);
int jg_nr_fast_get_increment(jg_nr* h, double* incr);

/*
 * power!(analysis) / current!(analysis) for every scenario of the batch at its CURRENT state --
 * src/postprocessing/acAnalysis.jl:30-169 (power!), 672-704 (current!), formula helpers :838-925.
 * jg_nr_set_branches (once): the branch table the post-processing needs,
 *   from,to [nb] 1-based; status [nb]; param [nb][16] = re,im of nodalFromFrom, nodalFromTo, nodalToFrom, nodalToTo,
 *   admittance (model.jl:54-67), re,im of t_ij = (1/turnsRatio) cis(-shiftAngle) (:846-851), branch conductance,
 *   susceptance, 1/turnsRatio, 0.
 * jg_nr_set_outage_labels: label[batch] = 1-based branch that is out of service in that scenario (0 none): its
 *   quantities are zero there, like an out-of-service branch of the reference (:71-81, :693-701).
 * jg_nr_branch_quantities: any output may be NULL; each [batch][nb][2]:
 *   from_pq, to_pq = PijQij, PjiQji (:898-904); series_pq = PlQl (:906-908); charging_pq = PcQc (:910-919);
 *   from_i, to_i, series_i = (magnitude, angle) of Iij, Iji, Is (:921-931).
 * jg_nr_bus_injection: inj_pq [batch][n][2] = PiQi (:891-896); the injection current, shunt, supply and generator
 *   powers follow from it on the host (juliagrid.jl_amd/powerflow.py:power_, O(n) each).
 */
int jg_nr_set_branches(jg_nr* h, int64_t nb, const int64_t* from, const int64_t* to, const int8_t* status, const double* param);
int jg_nr_set_outage_labels(jg_nr* h, const int64_t* label);
int jg_nr_branch_quantities(jg_nr* h, double* from_pq, double* to_pq, double* series_pq, double* charging_pq,
                            double* from_i, double* to_i, double* series_i);
int jg_nr_bus_injection(jg_nr* h, double* inj_pq);

/*
 * Contingency screen summary on the device (the next widening of the path) -- what a user of the reference reads off power!(analysis)
 * after every powerFlow! of the outage loop (src/powerSystem/branch.jl:453-459 + postprocessing/acAnalysis.jl:30-169), reduced per scenario so that
 * a sharded screen gathers 10 doubles per scenario instead of its 2 n + 2 state record.  For every scenario at its CURRENT state:
 *   rec[b][0] worst loading  max_k max(|S_ij|, |S_ji|) / rating[k]  over the in-service branches with rating[k] > 0 (0 if none), rec[b][1] its branch (1-based, 0: none)
 *   rec[b][2] largest apparent power at a branch end max(|S_ij|, |S_ji|) (pu; PijQij / PjiQji, :898-904), rec[b][3] its branch
 *   rec[b][4] lowest voltage magnitude, rec[b][5] its bus (1-based); rec[b][6] highest, rec[b][7] its bus
 *   rec[b][8] method.iteration, rec[b][9] status (0 converged, 1 iteration limit, 3 numeric failure) of the last jg_nr_run
 * Ties go to the lowest index.  The branch that is out of service in a scenario (jg_nr_set_outage_labels) does not count there.
 * A scenario that ended with status 3 (numeric failure: its state is NaN) delivers NaN in rec[b][0], [2], [4], [6] and index 0 in [1], [3], [5], [7]:
 * rank by rec[b][9] first -- a diverged contingency must never read as the safest one.
 * jg_nr_set_branches with another branch count drops an installed rating (it belongs to the table it was given for): call jg_nr_set_screen again.
 * jg_nr_set_screen: rating [nb] in pu of apparent power (branch.flow.maxFromBus / maxToBus of type 2, src/powerSystem/branch.jl:29-37), 0 = no limit, NULL = none;
 *   needs jg_nr_set_branches.  jg_nr_screen: rec [batch][10] to the host; jg_nr_screen_device: into a device buffer (the operand of jg_comm_allgather_device).
 * jg_nr_screen_rows_device: the summaries of lanes lane0 .. lane0 + count - 1 into rows rows[0 .. count) of a [.][10] device record (a pool handle returns the
 *   stragglers it finished to the record of the batch they came from, like jg_nr_pack_rows_device does for the state record).
 */
int jg_nr_set_screen(jg_nr* h, const double* rating);
int jg_nr_screen(jg_nr* h, double* rec);
int jg_nr_screen_device(jg_nr* h, double* rec_dev);
int jg_nr_screen_rows_device(jg_nr* h, double* rec_dev, int64_t lane0, int64_t count, const int32_t* rows);

/* Measurement hooks (HIP events on the handle's own stream).
 * kernel: 0 fused mismatch+Jacobian assembly, 1 LU refactorization + fused forward elimination (all
 * launches), 2 backward sweep (no state update), 3 power!/current! branch kernel (all outputs), 4 the linear step of a first
 * iteration on the shared base factor (per-scenario correction + sweep pair; needs jg_nr_attach_base), 5 the mismatch-only pass of such
 * a start.  Returns the mean milliseconds of `reps` back-to-back executions. */
int jg_nr_time_kernel(jg_nr* h, int kernel, int reps, double* mean_ms);

/* ---------------------------------------------------------------------------------------------
 * Gauss-Newton WLS state estimation
 * ------------------------------------------------------------------------------------------- */

/*
 * gaussNewton(monitoring) -- src/stateEstimation/acStateEstimation.jl:43-75 over acWLS (:77-259).
 * The caller passes what acWLS derives from the Measurement container row by row (rows ordered
 * voltmeters, ammeters, wattmeters, varmeters, PMUs x2):
 *   code[m]     measurement type code 1..21 (Appendix B of SURVEY.md) BEFORE status masking; codes 22..27 are the
 *               LINEAR rows of pmuStateEstimation (src/stateEstimation/pmuStateEstimation.jl:72-177): state = (Re V, Im V)
 *               per bus (kept in the angle / magnitude arrays), 22/23 bus phasor Re/Im, 24/25 from-end current Re/Im,
 *               26/27 to-end current Re/Im; pass slack = 0 for that model (no reference bus; every variable is estimated),
 *   status[m]   0/1; se.type = status * code (:139, :1139, :1161, :1190-1193, :1222),
 *   index[m]    1-based bus or branch index (se.index),
 *   corr_row[]  1-based FIRST row of every rectangular PMU with a 2x2 precision block (:220-221).
 * The library rebuilds the H pattern exactly as oneIndices!/twoIndices!/fourIndices!/nthIndices!
 * (:1130-1238) + sparse() (:238) do, the block pattern of the gain matrix H'WH, the gather lists
 * and the symbolic analysis replacing the first lu(gain) (src/backend/utility.jl:470-476).
 *   colptr,rowval,y_reim,yt_reim,slack   as for jg_nr_create (system.model.ac)
 *   from,to [nb]                          branch.layout.{from,to}
 *   branch_param [nb][6]                  re(ac.admittance), im(ac.admittance), branch.parameter.conductance,
 *                                         susceptance, turnsRatio, shiftAngle  (equations.jl:147-436)
 */
int jg_gn_create(jg_gn** h, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* y_reim,
                 const double* yt_reim, int64_t nb, const int64_t* from, const int64_t* to, const double* branch_param,
                 int64_t slack, int64_t m, const int8_t* code, const int8_t* status, const int64_t* index,
                 int64_t n_corr, const int64_t* corr_row, int64_t batch, int device);
void jg_gn_destroy(jg_gn* h);
/* dims[0]=m, [1]=nnz(H), [2]=gain blocks, [3]=L+D+U blocks, [4]=LU terms, [5]=factor launches,
 * [6]=backward launches, [7]=H slots (1x2 blocks) */
int jg_gn_dims(jg_gn* h, int64_t* dims);
/* The WlsMethod tag of gaussNewton(monitoring, T) (src/definition/analysis.jl:36-99; increment! methods
 * acStateEstimation.jl:878-971).  method 0 = the Normal tags (LU, KLU, QR, LDLt, LL: gain matrix H'WH, factorised by the
 * block engine).  method 1 = the Orthogonal and PetersWilkinson tags: the least-squares increment of
 * sqrt(W) H d = sqrt(W) r without forming Q -- the triangular factor of the reference's qr(sqrt(W) H) is the Cholesky factor of
 * the gain the engine already holds, and one correction pass through H itself (rho = r - H d; d += G^-1 H'W rho: corrected
 * semi-normal equations) replaces the multiplication by Q'.  Needs a diagonal precision matrix (the reference's
 * sqrtPrecision!, dcStateEstimation.jl:488-492, has the same restriction); returns 1 if the set has correlated PMUs. */
int jg_gn_set_method(jg_gn* h, int method);
/* se.mean [batch][m] and se.precision: diagonal [batch][m] + W[r,r+1] of every correlated pair
 * [batch][n_corr] (acStateEstimation.jl:135-236; equations.jl:576-677).  stride 0 broadcasts. */
int jg_gn_set_measurement(jg_gn* h, const double* mean, const double* wdiag, const double* woff,
                          int64_t batch_stride_m, int64_t batch_stride_corr);
/* Monte-Carlo realisations drawn ON the device.  The reference draws one inside add<Meter>!(...; noise = true) -- mean + variance^(1/2) * randn,
 * src/measurement/utility.jl:70-73 -- and acWLS applies its value rules to the noisy readings (acStateEstimation.jl:135-236; squared currents,
 * rectangular PMUs: equations.jl:576-666).  jg_gn_set_readings (once): the RAW readings per device in acWLS's row order -- row [ndev] 1-based first row,
 * kind [ndev]: 0 one row, value z; 1 one row, squared current (mean z^2, variance 4 z^2 sigma^2); 2 polar PMU (rows magnitude, angle); 3 polar PMU with
 * squared current magnitude; 4 / 5 rectangular PMU without / with its 2x2 precision block (5 exactly on the corr_row rows of jg_gn_create);
 * z1, v1, s1 magnitude (or the single quantity): mean, variance, status; z2, v2, s2 the PMU angle (ignored for kinds 0, 1).
 * jg_gn_draw_noise: lane b becomes realisation first_realisation + b of `seed`: z + scale * sigma * N(0,1) per raw reading from a counter-based generator
 * (csrc/jg_gn.hip: k_gn_noise -- the same realisation gets the same numbers on any rank, batch and lane.  Exactly, for device d (0-based, in row order) and realisation r, in
 * uint64 arithmetic:  c = (seed + 0x9E3779B97F4A7C15 * (2 d)) ^ (r * 0xD1B54A32D192ED03);  u1 = mix64(c), u2 = mix64(c + 0x9E3779B97F4A7C15) with mix64 the splitmix64 finaliser;
 * uniform (0, 1] = ((u >> 11) + 1) 2^-53;  the two normals of the device = sqrt(-2 ln u1) (cos, sin)(2 pi u2) -- the numpy restatement is tests/test_montecarlo_gpu.py:_normals), then the value
 * rules: se.mean and se.precision of every scenario are rewritten in place, nothing crosses PCIe.  scale 0 restores the noise-free set.  Returns 1 when a
 * variance comes out zero or not finite (the reference's errorVariance).  jg_gn_get_measurement: se.mean / diag(se.precision) [batch][m], pair terms [batch][n_corr]. */
int jg_gn_set_readings(jg_gn* h, int64_t ndev, const int64_t* row, const int8_t* kind, const double* z1, const double* v1, const int8_t* s1,
                       const double* z2, const double* v2, const int8_t* s2);
int jg_gn_draw_noise(jg_gn* h, uint64_t seed, double scale, int64_t first_realisation);
int jg_gn_get_measurement(jg_gn* h, double* mean, double* wdiag, double* woff);
int jg_gn_set_voltage(jg_gn* h, const double* vm, const double* va, int64_t batch_stride);
int jg_gn_get_voltage(jg_gn* h, double* vm, double* va);
/* Keep / restore the current state inside HBM (restart of a Monte-Carlo batch from the same start point without a
 * host round trip; the counterpart of jg_nr_snapshot_voltage / jg_nr_restore_voltage). */
int jg_gn_snapshot_voltage(jg_gn* h);
int jg_gn_restore_voltage(jg_gn* h);
/* increment!(analysis) -- acStateEstimation.jl:878-904: residual + Jacobian, gain, factor, solve.
 * max_inc [batch] = maximum(abs, increment). */
int jg_gn_increment(jg_gn* h, double* max_inc);
/* solve!(analysis) -- acStateEstimation.jl:1035-1047 */
int jg_gn_solve(jg_gn* h);
/* stateEstimation!(analysis; iteration, tolerance) -- acStateEstimation.jl:1286-1329, per scenario.
 * status 0 converged, 1 iteration limit, 3 singular gain. */
int jg_gn_run(jg_gn* h, int64_t max_iter, double tol, int32_t* iters, int32_t* status);
/* se.type and jacobian.{colptr,rowval} (m x 2n CSC, 1-based, bit-exact) */
int jg_gn_get_maps(jg_gn* h, int8_t* type, int64_t* hcolptr, int64_t* hrowval);
/* se.jacobian.nzval [batch][nnzH], se.residual [batch][m], se.increment [batch][2n] (theta then V) */
int jg_gn_get_jacobian(jg_gn* h, double* nzval);
int jg_gn_get_residual(jg_gn* h, double* residual);
int jg_gn_get_increment(jg_gn* h, double* increment);
int jg_gn_get_iteration(jg_gn* h, int32_t* iters);
/* se.objective = r' W r at the residual the handle holds (the last increment! / evaluate: after stateEstimation! the residual of every scenario at its
 * final state) -- src/backend/equations.jl:689-698 incl. the cross terms of correlated PMU pairs --, reduced on the device in a fixed order; [batch]. */
int jg_gn_get_objective(jg_gn* h, double* objective);
/*
 * Sharded Monte-Carlo state estimation (SURVEY.md 8e for the Gauss-Newton side): noisy realisations of one measurement set are independent scenarios
 * (the reference draws them in add<Meter>!(...; noise = true), src/measurement/utility.jl:70-73, and estimates them one after the other,
 * acStateEstimation.jl:1286-1329); a rank estimates a contiguous block of them and ONE collective hands every rank the whole result.
 *   jg_gn_pack_results_device  the handle's record after jg_gn_run into device memory of the caller: [batch][2 n + 3] =
 *                              magnitude[n] | angle[n] | method.iteration | status | se.objective  per realisation (the state arrays as jg_gn_get_voltage
 *                              returns them; bitwise the getters' values).  Returns after the stream has drained.
 *   jg_gn_allgather_results    packs into block `rank` of dst_dev [world x batch][2 n + 3] and gathers in place (ncclAllGather of RCCL on the handle's
 *                              stream); every rank calls it with the same batch.
 */
int jg_gn_pack_results_device(jg_gn* h, double* dst_dev);
/* residualTest!(analysis) -- src/stateEstimation/badData.jl:119-311, the numeric part, per scenario: residual, Jacobian,
 * gain and its factor at the CURRENT state, selected inverse of the gain on its factor pattern (replaces
 * takahashiCholeskyLower / selectedInverse, :536-637), c = rowProjection (:289-311), normalised residuals
 * |r_i| / sqrt(|1 / W_ii - c_i|) (0 where r_i == 0 or the row carries no weight in that scenario).
 * max_nres [batch], index [batch] = 1-based row of the largest one (first on ties, 0 if all are zero). */
int jg_gn_residual_test(jg_gn* h, double* max_nres, int32_t* index);
/* update<Meter>!(analysis; label, status) -- src/measurement/powermeter.jl:640-677 and siblings: new in-service mask,
 * se.type = status * code; the Jacobian pattern (and every table derived from it) stays.  code (optional, NULL = keep):
 * new type codes; only 2 <-> 4 and 3 <-> 5 may change (updateAmmeter!(...; square), ammeter.jl:367-420). */
int jg_gn_set_status(jg_gn* h, const int8_t* status, const int8_t* code);
/* residual and Jacobian at the CURRENT state, nothing else (se.residual for chiTest after the last solve!) */
int jg_gn_evaluate(jg_gn* h);
/* all normalised residuals of the last jg_gn_residual_test [batch][m] */
int jg_gn_get_normalized_residual(jg_gn* h, double* nres);
/* kernel: 0 measurement rows (H + residual), 1 gain + rhs gather, 2 factor (+ fused forward), 3 backward,
 * 4 selected inverse (needs a factor: call after an increment) */
int jg_gn_time_kernel(jg_gn* h, int kernel, int reps, double* mean_ms);

/* ---------------------------------------------------------------------------------------------
 * Sharded contingency screen: the final gather.  Scenarios are independent, a rank (one process per GPU) solves a
 * contiguous block of them, and ONE collective -- ncclAllGather of RCCL over xGMI -- hands every rank the result record of the whole
 * screen in scenario order.  The reference has no counterpart: its user-level loop runs the scenarios one after the other in one
 * process (src/powerSystem/branch.jl:453-459: updateBranch!(...; status = 0), powerFlow!, updateBranch!(...; status = 1)).
 *   jg_comm_unique_id  rank 0 draws the 128-byte id of a communicator; the HOST ships it to the other ranks (MPI, a file, a socket)
 *   jg_comm_create     collective over the `world` ranks: rank's communicator on HIP device `device`
 *   jg_nr_allgather_results  packs the handle's record ([batch][2 n + 2]: V | theta | iterations | status, jg_nr_pack_results_device)
 *                      into block `rank` of dst_dev [world x batch][2 n + 2] (device memory of the caller) and gathers in place on
 *                      the handle's stream; every rank must call it with the same batch.  Returns after the stream has drained.
 *   jg_comm_allgather_device  the same collective for a record that is already packed (a ContingencyPipeline fills its records
 *                      itself): count doubles per rank, recv_dev [world][count]; send_dev may be recv_dev + rank * count.  The gather runs on the
 *                      communicator's own stream: whatever produced send_dev must have been synchronised before the call; it returns when done.
 * librccl is bound at run time on the first call (csrc/jg_comm.cpp); return code 2 with jg_last_error() when it is missing.
 * ------------------------------------------------------------------------------------------- */
#define JG_COMM_ID_BYTES 128
typedef struct jg_comm jg_comm;
int jg_comm_unique_id(uint8_t* id);
int jg_comm_create(jg_comm** c, int64_t rank, int64_t world, const uint8_t* id, int device);
void jg_comm_destroy(jg_comm* c);
int jg_comm_rank(const jg_comm* c);
int jg_comm_world(const jg_comm* c);
int jg_comm_allgather_device(jg_comm* c, const double* send_dev, double* recv_dev, int64_t count);
int jg_nr_allgather_results(jg_nr* h, jg_comm* c, double* dst_dev);
int jg_gn_allgather_results(jg_gn* h, jg_comm* c, double* dst_dev);

/* ---------------------------------------------------------------------------------------------
 * DC power flow and the batched DC N-1 screen (csrc/jg_dc.hip)
 * ------------------------------------------------------------------------------------------- */

/*
 * The DC handle is an int64 TOKEN (0 = none), not a pointer to an opaque struct: it crosses every binding as a plain integer.
 *
 * dcPowerFlow(system)  -- src/powerFlow/dcPowerFlow.jl:42-61 with the factorisation of the first solve! (:63-101): the slack row and column leave
 * system.model.dc.nodalMatrix (dcModel!, src/powerSystem/model.jl:161-209), the slack diagonal becomes 1, and the matrix is factorised ONCE on the
 * device (scalar LU on the elimination order and dependency levels of the bus graph, no pivoting); every later solve reuses that factor.
 *   n               number of buses
 *   colptr,rowval   pattern of dc.nodalMatrix (1-based CSC, rows sorted: SparseMatrixCSC), structurally symmetric with a full diagonal
 *   nzval           its values, stored zeros of out-of-service branches included
 *   slack           bus.layout.slack (1-based);  slack_angle = bus.voltage.angle[slack], added to every angle (dcPowerFlow.jl:94-99)
 *   batch           scenarios resident on the device (>= 1; kept batch-minor with a leading dimension of batch rounded up to 64)
 * Return code 3: zero / non-finite pivot.
 * jg_dc_dims: {n, batch, ld, branches, factor entries, factorisation levels, forward levels, backward levels, launches of a sweep pair, padded sweep terms}.
 */
int jg_dc_create(int64_t* h, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, int64_t slack,
                 double slack_angle, int64_t batch, int device);
void jg_dc_destroy(int64_t h);
int jg_dc_dims(int64_t h, int64_t* dims10);
/*
 * The right-hand side of solve! (dcPowerFlow.jl:82-92): b = supply.active - demand.active - shunt.conductance - shiftPower, [n] (the slack's
 * entry is ignored).  jg_dc_set_rhs is the base case of every lane and drops earlier per-scenario injections.
 * jg_dc_set_injections: lanes lane0 .. lane0 + count - 1 get right-hand sides of their own, rhs [count][n] (the user loop updateBus!(analysis; active) /
 * updateGenerator!(analysis; active) -> solve!, src/powerSystem/bus.jl:300-311, generator.jl:382-395, over Monte-Carlo draws).  Only the 64-lane groups
 * that hold such a lane pay a second sweep pair.
 */
int jg_dc_set_rhs(int64_t h, const double* rhs);
int jg_dc_set_injections(int64_t h, int64_t lane0, int64_t count, const double* rhs);
/*
 * The branch table, once per handle: from / to (1-based bus indices, branch.layout.from / to), dc.admittance (0 for a branch out of service in the base,
 * model.jl:176-183), parameter.shiftAngle.  Needed by outages, flows and the screen.  jg_dc_set_rating: the [branches] ratings the screen divides |from| by
 * (per unit of active power; <= 0: the branch is not rated; NULL: none is).
 */
int jg_dc_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, const double* shift_angle);
int jg_dc_set_rating(int64_t h, const double* rating);
/*
 * updateBranch!(analysis; label, status = 0) per scenario (src/powerSystem/branch.jl:453-459 with dcNodalUpdate! / dcShiftUpdate! / dcAdmittanceUpdate!,
 * model.jl:212-262): lane lane0 + s loses branch branch[s] (1-based, 0 = no outage).  The matrix is NOT rebuilt: the lane's solution is the base
 * solution plus a rank-1 correction on the shared factor (csrc/jg_dc.hpp).
 */
int jg_dc_set_outages(int64_t h, int64_t lane0, int64_t count, const int64_t* branch);
/*
 * solve!(analysis) for every lane (dcPowerFlow.jl:63-101): the base solution if the right-hand side changed, one sweep pair for the lanes' outages,
 * the rank-1 combine.  status per scenario: 0 solved, 3 the outaged branch is a bridge (the outage islands the grid; its angles are NaN);
 * 4 only in island mode 1 (below): solved on the slack's island, the rest shed).
 *   jg_dc_get_angle     theta [batch][n] = analysis.voltage.angle, status [batch] (either may be NULL)
 *   jg_dc_angle_device  info[0] = device address of the angles, batch-minor [n][info[1]], info[2] = device address of the int32 status [info[1]]
 *   jg_dc_get_flows     power!(analysis) branch part (src/postprocessing/dcAnalysis.jl:41-48): from [batch][branches], to = -from; the outaged branch of a lane carries 0
 *   jg_dc_screen        rec [batch][5]: worst |from| / rating and its branch (1-based, 0 = none rated), largest |from| and its branch, status; ties go to
 *                       the lowest branch index.  jg_dc_screen_device: the same record into device memory of the caller (an operand of jg_comm_allgather_device)
 *   jg_dc_pack_results_device   angle | status, [batch][n + 1] doubles, into device memory of the caller (likewise)
 *   jg_dc_time_kernel   milliseconds (HIP events on the handle's stream) of `reps` runs of: 0 the whole chain of a batch (sweeps, combine, flows + summary),
 *                       1 the sweep pair, 2 the combine, 3 flows + summary; ms [reps]
 */
int jg_dc_solve(int64_t h);
int jg_dc_get_angle(int64_t h, double* theta, int32_t* status);
int jg_dc_angle_device(int64_t h, int64_t* info3);
int jg_dc_get_flows(int64_t h, double* from);
int jg_dc_screen(int64_t h, double* rec);
int jg_dc_screen_device(int64_t h, double* rec_dev);
int jg_dc_pack_results_device(int64_t h, double* dst_dev);
int jg_dc_time_kernel(int64_t h, int kernel, int reps, double* ms);
/*
 * Two outages per lane: updateBranch!(analysis; label = a, status = 0), updateBranch!(analysis; label = b, status = 0), solve!.  Lane lane0 + s loses
 * branch_a[s] and branch_b[s] (1-based; branch_b[s] = 0: a single outage, both 0: none; the two must differ).  jg_dc_solve then runs a second sweep pair
 * for the 64-lane groups that hold a second outage, and only for those, and combines through the 2 x 2 system of csrc/jg_dc_pair.hpp (injections of
 * the lane's own included).  Flows and the screen put 0 on both branches; a pair that islands a part of the grid gets status 3 and NaN angles, also
 * when neither branch alone is a bridge.  A handle on which no second outage was ever set allocates nothing for this and takes the one-outage path.
 * jg_dc_set_outages over such lanes clears their second outage.
 */
int jg_dc_set_outage_pairs(int64_t h, int64_t lane0, int64_t count, const int64_t* branch_a, const int64_t* branch_b);
/*
 * Bridge outages solved on the slack's island (an extension of the batch interface: the reference's solve! meets a singular matrix there).
 *   jg_dc_set_island_mode   mode 0 (default): a lane whose outage is a bridge gets status 3 and NaN angles.  mode 1: lanes set AFTERWARDS by
 *                       jg_dc_set_outages (or by jg_dc_set_outage_pairs with one branch) whose branch is a bridge are solved on the side of the bridge
 *                       that holds the slack: status 4, the angles of the buses that leave are NaN, flows are 0 on the outaged branch and on every
 *                       branch with an end among those buses, and the screen record covers the branches that stay.  The same sweep pair as any lane
 *                       (right-hand side e_m, m the bridge's end on the slack's side) and a combine without a denominator (csrc/jg_dc.hpp).  Lanes with
 *                       TWO outages keep status 3 for whatever islands (jg_dc_pair_screen has a mode of its own).  Every other lane is bitwise what it is in mode 0.
 *                       Needs jg_dc_set_branches.
 *   jg_dc_get_islands   rec [batch][4] after jg_dc_solve: buses shed, the lane's right-hand side summed over them, m (1-based), g = the flow that left m
 *                       over the bridge before the outage; zeros on lanes that shed nothing.
 *   jg_dc_island_table  host only (no device is touched): the table behind it for a branch list (from / to 1-based, admittance 0 = out of service).
 *                       preorder [n]: DFS number of every bus from the slack (-1: not reached); per branch lo, hi: the buses that leave with it are those
 *                       with lo <= preorder <= hi (lo > hi: not a bridge), side: +1 / -1 the from / to end stays on the slack's side (0: not a bridge).
 */
int jg_dc_set_island_mode(int64_t h, int mode);
int jg_dc_get_islands(int64_t h, double* rec);
int jg_dc_island_table(int64_t n, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, int64_t slack,
                       int32_t* preorder, int32_t* lo, int32_t* hi, int32_t* side);
/*
 * The DC N-2 screen over ALL pairs k < l of a candidate list, from the one factor and the kept outage sensitivities (csrc/jg_dc_pair.hpp): the user loop
 * updateBranch!(k), updateBranch!(l), solve!, power! over all pairs.  Needs jg_dc_set_branches and jg_dc_set_rhs; the lanes of the handle are not touched.
 *   jg_dc_pair_build    candidates [nk] (1-based branches, in service, strictly ascending, nk >= 2); monitored [nm] (1-based; NULL: every branch in
 *                       service).  One sweep pair per candidate (512 at a time) fills Phi[m,k] = y_m a_m' B^-1 a_k on the rows monitored u candidates,
 *                       [rows][nk rounded up to 64] doubles.  budget_bytes: what Phi and the build's scratch may take (<= 0: 0.8 of the free device
 *                       memory, asked from hipMemGetInfo); return code 5 and a message that names the sizes when they do not fit -- nothing is
 *                       allocated then and the handle stays as it was.  info [8]: rows, leading dimension, bytes of Phi, free bytes, budget, and
 *                       the milliseconds (HIP events) of the build: total, sweep pairs, Phi kernel.  A second build replaces the first.
 *   jg_dc_pair_screen   the pairs (k, l > k) of the candidate POSITIONS k in [k0, k1) (0-based; the row block bounds the memory of a call, 16 bytes per
 *                       pair, and is the unit a caller shards by) against the ratings of jg_dc_set_rating (not rated or not monitored: loading 0).
 *                       records [capacity][5]: the pairs whose worst loading exceeds threshold, sorted by (k, l): branch k, branch l (1-based), worst
 *                       branch, worst |from| / rating, number of monitored branches above threshold; ties of the worst branch go to the lowest index.
 *                       islanding [island_capacity][2]: the pairs whose 2 x 2 system is singular (|det| < 1e-9: status 3), sorted likewise.
 *                       totals [6]: pairs screened, violating, islanding, records written, islanding pairs written, flags (1: the record list
 *                       overflowed, 2: the islanding list did) -- the counts are exact also then, and the entries kept are the FIRST by (k, l).
 *                       worst [nk] (nullable, in/out): max-merged with the worst loading over the pairs of each candidate, as k or as l.
 *                       dense_* (each nullable) [k1 - k0][nk]: worst loading (NaN: islanding), its branch, the count, the determinant; 0 where l <= k.
 *   jg_dc_pair_time_kernel   milliseconds of `reps` runs on rows [k0, k1) (a block jg_dc_pair_screen has held): 0 the screen kernel, 1 the row / column
 *                       summaries behind it
 *   jg_dc_pair_release  frees what the screen holds on the device
 * Pairs with a bridge screened on the slack's island (csrc/jg_dc_pair.hpp, "shed mode"):
 *   jg_dc_pair_set_island_mode     the island mode of the NEXT jg_dc_pair_build, which takes it and sets it back to 0.  0: a pair with a bridge is
 *                       singular (status 3, as above).  1: a candidate the graph calls a bridge (the table of jg_dc_island_table on the handle's branches)
 *                       is shed as jg_dc_set_island_mode 1 sheds a lane's: in a pair that holds one or two bridges the buses behind them leave, a
 *                       branch with an end among them carries 0, the other branch (if it stays) is solved on what is left, and the pair enters the
 *                       records, the counts and worst like any other.  `islanding` keeps the joint cuts of two non-bridges and the pairs with a
 *                       non-bridge whose |1 - Phi[l,l]| < 1e-9.  A pair of two non-bridges is bitwise what it is after a build in mode 0.  dense_det of
 *                       a pair with a bridge: the denominator of the branch that is solved, 1 where there is none.
 *   jg_dc_pair_get_shed_table      as jg_dc_series_get_shed_table.
 *   jg_dc_pair_get_shed            flow [count]: what left m over the bridge in the base case, per bridge of [k0, k1) in the order of the table.
 */
int jg_dc_pair_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t budget_bytes, double* info8);
int jg_dc_pair_screen(int64_t h, int64_t k0, int64_t k1, double threshold, int64_t capacity, double* records, int64_t island_capacity,
                      int64_t* islanding, int64_t* totals6, double* worst, double* dense_load, int32_t* dense_branch, int32_t* dense_count,
                      double* dense_det);
int jg_dc_pair_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms);
int jg_dc_pair_release(int64_t h);
int jg_dc_pair_set_island_mode(int64_t h, int mode);
int jg_dc_pair_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* branches, int64_t* buses, int64_t* m, int64_t* side);
int jg_dc_pair_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow);
/*
 * The DC common-mode screen over named outage GROUPS of 1 to 8 branches, each group one case (csrc/jg_dc_group.hpp): the user loop updateBranch!(s, status = 0)
 * for every member s, solve!, power! per group.  With Phi of jg_dc_pair_build on the candidates = the sorted union of all members, a group S costs a
 * |S| x |S| solve (I - Phi_SS) c = f0_S and one pass f_m(S) = f0_m + sum_s Phi[m,s] c_s over the rows, 0 on the members -- no sweep per case.  Needs
 * jg_dc_set_branches and jg_dc_set_rhs; neither the lanes of the handle nor what the other screens keep are touched.
 *   jg_dc_group_build   the groups as a CSR: offsets [ngroups + 1] (offsets [0] = 0), members (1-based branches, in service, no branch twice within a
 *                       group, 1 to 8 per group; return code 1 names the offending group, 0-based).  monitored, budget_bytes and info [8] as jg_dc_pair_build.
 *                       A second build replaces the first.
 *   jg_dc_group_screen  the groups [g0, g1) (0-based; the block bounds the memory of a call) against the ratings of jg_dc_set_rating.  Per group of the
 *                       block (each nullable): status (0, or 3: a pivot of the LU with partial pivoting of I - Phi_SS is below 1e-9 in magnitude -- the
 *                       group holds a bridge or its members form a joint cut), worst (the largest |from| / rating over the monitored branches that
 *                       stay; NaN for status 3), worst_branch (1-based, ties to the lowest index; 0: none), count (monitored branches above threshold).
 *                       records [capacity][4]: the violating branches, sorted by (group, branch): group (0-based), branch (1-based), flow, loading.
 *                       islanding [island_capacity]: the status-3 groups (0-based), ascending.  totals [6]: groups screened, violating branches,
 *                       islanding groups, records written, islanding groups written, flags (1: the record list overflowed, 2: the islanding list did)
 *                       -- the counts are exact also then, and the entries kept are the FIRST.  dense_flow (nullable) [g1 - g0][monitored ascending]:
 *                       the flows, 0 on the members, NaN for status 3.  ms (nullable): the milliseconds of the call's solves and screen kernel (HIP events).
 *   jg_dc_group_get_dims         dims [6]: groups, their leading dimension, candidates, rows of Phi, monitored branches, members of the largest group
 *   jg_dc_group_get_candidates   labels [candidates]: the union of the members, 1-based ascending
 *   jg_dc_group_get_base         flow [monitored]: the base-case flows of the monitored branches, ascending
 *   jg_dc_group_time_kernel      milliseconds of `reps` runs on the groups [g0, g1) (a block jg_dc_group_screen has held): 0 the screen kernel, 1 the solves
 *   jg_dc_group_release          frees what the screen holds on the device
 */
int jg_dc_group_build(int64_t h, int64_t ngroups, const int64_t* offsets, const int64_t* members, int64_t nm, const int64_t* monitored, int64_t budget_bytes,
                      double* info8);
int jg_dc_group_screen(int64_t h, int64_t g0, int64_t g1, double threshold, int64_t capacity, double* records, int64_t island_capacity, int64_t* islanding,
                       int64_t* totals6, int32_t* status, double* worst, int32_t* worst_branch, int32_t* count, double* dense_flow, double* ms);
int jg_dc_group_get_dims(int64_t h, int64_t* dims6);
int jg_dc_group_get_candidates(int64_t h, int64_t* labels);
int jg_dc_group_get_base(int64_t h, double* flow);
int jg_dc_group_time_kernel(int64_t h, int kernel, int64_t g0, int64_t g1, int reps, double* ms);
int jg_dc_group_release(int64_t h);
/*
 * The DC probabilistic N-1 screen under Gaussian injection uncertainty (csrc/jg_dc_chance.hpp): with branch k out of service, how likely is branch m to
 * exceed its rating?  Injections are p0 + L' xi, xi ~ N(0, I_r); the flows are linear in them, so with Phi of jg_dc_pair_build, the base flows f0 and the
 * factor sensitivities S[m,j] = y_m a_m' B^-1 L_j (ONE sweep pair per factor) the post-contingency flow of m is Gaussian with
 *     g = Phi[m,k] / (1 - Phi[k,k]),   mu = f0[m] + g f0[k],   sigma = sqrt(sum_j (S[m,j] + g S[k,j])^2),
 *     P = 1/2 erfc((rating - mu) / (sigma sqrt 2)) + 1/2 erfc((rating + mu) / (sigma sqrt 2))          (sigma == 0: 1 if |mu| > rating, else 0)
 * and no sample is drawn.  Needs jg_dc_set_branches and jg_dc_set_rhs; neither the lanes of the handle nor what the other screens keep are touched.
 *   jg_dc_chance_build   factors [r][n], 1 <= r <= 32 (return code 1 otherwise): net active injection per unit of xi_j, the slack's entry is taken as 0.
 *                        candidates [nk] (nk >= 1), monitored [nm] and budget_bytes as jg_dc_series_build takes them.  injection_rhs (nullable) [n]: the
 *                        right-hand side of p0 as jg_dc_set_rhs takes it; null: the handle's base case.  info [12]: [0..7] as jg_dc_pair_build, [8] the
 *                        bytes of S, [9..11] the milliseconds of S: total, sweep pairs, flow kernel.  A second build replaces the first.
 *   jg_dc_chance_screen  the candidates [k0, k1) (positions; the block bounds the memory of a call) against the ratings of jg_dc_set_rating; an unrated or
 *                        unmonitored branch has P = 0 and enters nothing.  0 < probability <= 1.  Per candidate of the block (each nullable): worst (the
 *                        largest P over the monitored branches; NaN for status 3), worst_branch (1-based, ties to the lowest index; 0: none), count
 *                        (branches with P >= probability), status (0, or 3: |1 - Phi[k,k]| < 1e-9, a bridge; no shedding).  records [capacity][5]: the
 *                        (k, m) with P >= probability, sorted by (k, m): label k, label m, mu, sigma, P.  totals [5]: candidates screened, records,
 *                        bridges, records written, 1 when the list overflowed -- the counts are exact also then, and the entries kept are the FIRST.
 *                        dense_mu / dense_sigma / dense_p (nullable) [k1 - k0][monitored ascending]: 0 at m = k, NaN for status 3.
 *   jg_dc_chance_get_dims         dims [6]: candidates, their leading dimension, rows of Phi, monitored branches, factors, leading dimension of S
 *   jg_dc_chance_get_base         mean / std_dev / probability (each nullable) [monitored]: the base case, no outage (needs jg_dc_set_rating)
 *   jg_dc_chance_time_kernel      milliseconds of `reps` runs on the candidates [k0, k1) (a block jg_dc_chance_screen has held): 0 the screen kernel,
 *                                 1 the base-case kernel
 *   jg_dc_chance_release          frees what the screen holds on the device
 */
int jg_dc_chance_build(int64_t h, int64_t r, const double* factors, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored,
                       const double* injection_rhs, int64_t budget_bytes, double* info12);
int jg_dc_chance_screen(int64_t h, int64_t k0, int64_t k1, double probability, int64_t capacity, double* records, int64_t* totals5, double* worst,
                        int32_t* worst_branch, int32_t* count, int32_t* status, double* dense_mu, double* dense_sigma, double* dense_p);
int jg_dc_chance_get_dims(int64_t h, int64_t* dims6);
int jg_dc_chance_get_base(int64_t h, double* mean, double* std_dev, double* probability);
int jg_dc_chance_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms);
int jg_dc_chance_release(int64_t h);
/*
 * The DC cascading-outage screen (csrc/jg_dc_cascade.hpp): the user loop updateBranch!(s, status = 0) for an initiating outage, solve!, power!, then
 * updateBranch! for every overloaded branch, solve!, power! again, until nothing is overloaded -- per initiating event.  Here an event is an outage set S
 * that grows on the device: the algebra of jg_dc_group_build per stage, (I - Phi_SS) c = f0_S by LU with partial pivoting, f_m = f0_m + sum_s Phi[m,s] c_s,
 * and ONE kernel launch runs a block of cascades to their ends.  Needs jg_dc_set_branches and jg_dc_set_rhs; neither the lanes of the handle nor what the
 * other screens keep are touched.
 *   jg_dc_cascade_build  the initiating events as a CSR, as jg_dc_group_build takes its groups (return code 1 names the event).  monitored [nm] (null:
 *                        every branch in service): the branches that can trip and that are reported.  The candidates are the sorted union of all members
 *                        and of the monitored branches in service -- whatever can trip needs its column -- so Phi is not blocked over candidates:
 *                        return code 5 and the bytes needed and available when it does not fit budget_bytes (0: 80 % of the free memory), before any
 *                        sweep.  info [8] as jg_dc_pair_build.  A second build replaces the first.
 *   jg_dc_cascade_run    the cascades [c0, c1) (0-based; the block bounds the memory of a call) against the ratings of jg_dc_set_rating.  A monitored,
 *                        rated branch trips when |flow| / rating > trip (strict; trip >= 0).  rule 0: every overloaded branch leaves at once, ascending
 *                        by branch within a stage; rule 1: only the most loaded one (ties to the lowest branch).  most (2 to 8): branches out of service
 *                        in one cascade, initiating ones included (an event with more members: return code 1).  Per cascade (each nullable): status
 *                        (0: stable, 3: the set islands a part of the grid, 5: truncated -- the next stage would exceed `most`, the set stays), stages
 *                        (stages of trips applied), size (branches out at the end), tripped / stage / loading [c1 - c0][most] (labels in the order they
 *                        left, 0 unused; the stage each left at, 0 initiating, -1 unused; the loading that tripped it, NaN for initiating and unused
 *                        slots), worst / worst_branch (the final state; NaN and 0 for status 3), pending (status 5: the overloaded branches).
 *                        dense_flow (nullable) [c1 - c0][monitored ascending]: the final flows, 0 on what is out, NaN for status 3.  ms (nullable): the
 *                        milliseconds of the kernel (HIP events).
 *   jg_dc_cascade_get_dims         dims [6]: events, their leading dimension, candidates, rows of Phi, monitored branches, members of the largest event
 *   jg_dc_cascade_get_candidates   labels [candidates], 1-based ascending
 *   jg_dc_cascade_get_base         flow [monitored]: the base-case flows of the monitored branches, ascending
 *   jg_dc_cascade_time_kernel      milliseconds of `reps` runs on the cascades [c0, c1) (a block jg_dc_cascade_run has held) with the trip and most of
 *                                  the last run: kernel 0 rule 0, kernel 1 rule 1
 *   jg_dc_cascade_release          frees what the screen holds on the device
 */
int jg_dc_cascade_build(int64_t h, int64_t nevents, const int64_t* offsets, const int64_t* members, int64_t nm, const int64_t* monitored, int64_t budget_bytes,
                        double* info8);
int jg_dc_cascade_run(int64_t h, int64_t c0, int64_t c1, double trip, int rule, int most, int32_t* status, int32_t* stages, int32_t* size, int64_t* tripped,
                      int32_t* stage, double* loading, double* worst, int32_t* worst_branch, int32_t* pending, double* dense_flow, double* ms);
int jg_dc_cascade_get_dims(int64_t h, int64_t* dims6);
int jg_dc_cascade_get_candidates(int64_t h, int64_t* labels);
int jg_dc_cascade_get_base(int64_t h, double* flow);
int jg_dc_cascade_time_kernel(int64_t h, int kernel, int64_t c0, int64_t c1, int reps, double* ms);
int jg_dc_cascade_release(int64_t h);
/*
 * The DC N-1 screen over a SERIES of injection profiles (csrc/jg_dc_series.hpp): the user loop updateBus!(...; active) / updateGenerator!(...; active) per
 * profile t around updateBranch!(k, status = 0), solve!, power!, updateBranch!(k, status = 1) per branch k.  No sweep per case: with Phi of
 * jg_dc_pair_build and the profiles' base flows F0[m,t], f_m(k,t) = F0[m,t] + Phi[m,k] F0[k,t] / (1 - Phi[k,k]).  Needs jg_dc_set_branches and
 * jg_dc_set_rhs; neither the lanes of the handle nor what jg_dc_pair_build keeps are touched.
 *   jg_dc_series_build  candidates [nk] and monitored [nm] as jg_dc_pair_build takes them, but nk >= 1; rhs [profiles][n]: the right-hand sides as
 *                       jg_dc_set_injections takes them (net injection - shunt conductance - shiftPower).  Phi by the build of jg_dc_pair_build, then
 *                       one sweep pair per profile (512 at a time, scratch of the build's own) fills F0 [rows][profiles rounded up to 64] doubles.
 *                       budget_bytes as jg_dc_pair_build, for Phi + F0 + the scratch of both: return code 5 with the sizes in the message and nothing
 *                       allocated when they do not fit (a caller with more profiles than fit splits them: the result of a profile does not depend on
 *                       the others).  info [12]: the eight of jg_dc_pair_build, bytes of F0, and the milliseconds of its build: total, sweep pairs,
 *                       F0 kernel.  A second build replaces the first.
 *   jg_dc_series_screen the cases (k, t) of the candidate POSITIONS k in [k0, k1) (0-based; the row block bounds the memory of a call, 16 bytes per
 *                       case) x all profiles against the ratings of jg_dc_set_rating (not rated or not monitored: loading 0).
 *                       records [capacity][5]: the cases whose worst loading exceeds threshold, sorted by (k, t): branch k (1-based), profile t
 *                       (0-based), worst branch, worst |from| / rating, number of monitored branches above threshold; ties of the worst branch go to
 *                       the lowest index.  islanding [k1 - k0] (nullable): the candidates of the block that are bridges (|1 - Phi[k,k]| < 1e-9:
 *                       status 3 and a NaN loading in every profile; never in the records), 1-based.
 *                       totals [5]: cases screened, violating, bridge candidates, records written, 1 when the record list overflowed -- the counts
 *                       are exact also then, and the records kept are the FIRST by (k, t).
 *                       worst [nk] (nullable): positions k0 .. k1 - 1 get the worst loading over the profiles (0 on a bridge).  worst_profile
 *                       [profiles] (nullable, in/out): max-merged with the worst loading over the block's candidates (bridges aside);
 *                       violating_profile [profiles] (nullable, in/out): the block's candidates whose outage violates are added.
 *                       base [profiles][3] (nullable): the profiles' base case -- worst loading, its branch, branches above threshold.
 *                       dense_* (each nullable) [k1 - k0][profiles]: worst loading (NaN: bridge), its branch, the count.
 *   jg_dc_series_time_kernel   milliseconds of `reps` runs on rows [k0, k1) (a block jg_dc_series_screen has held): 0 the screen kernel, 1 the row /
 *                       column summaries behind it
 *   jg_dc_series_release  frees what the screen holds on the device
 * Bridge candidates screened on the slack's island (csrc/jg_dc_series.hpp, "shed mode"):
 *   jg_dc_series_set_island_mode   the island mode of the NEXT jg_dc_series_build, which takes it and sets it back to 0.  0: a bridge candidate is
 *                       skipped (status 3, as above).  1: a candidate the graph calls a bridge (the table of jg_dc_island_table on the handle's branches)
 *                       is solved as jg_dc_set_island_mode 1 solves a lane: the buses behind it leave, a branch with an end among them carries 0, the
 *                       worst loading, its branch and the count cover the branches that stay, and the case enters the records, worst, worst_profile
 *                       and violating_profile like any other; it is not in `islanding`, which keeps the non-bridges with |1 - Phi[k,k]| < 1e-9.
 *   jg_dc_series_get_shed_table    the bridge candidates among the POSITIONS [k0, k1) of a build in mode 1 (none after a build in mode 0): *count, and
 *                       per bridge (each [k1 - k0], nullable) the branch (1-based), the buses that leave, the bridge's end m on the slack's side
 *                       (1-based bus), side +1 / -1: m is the from / to end.
 *   jg_dc_series_get_shed          flow [count][profiles]: what left m over the bridge before the outage, per bridge of [k0, k1) in the order of the
 *                       table and per profile, gathered on the device.  The right-hand side summed over what leaves is its negative.
 */
int jg_dc_series_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t profiles, const double* rhs,
                       int64_t budget_bytes, double* info12);
int jg_dc_series_screen(int64_t h, int64_t k0, int64_t k1, double threshold, int64_t capacity, double* records, int64_t* islanding, int64_t* totals5,
                        double* worst, double* worst_profile, int64_t* violating_profile, double* base, double* dense_load, int32_t* dense_branch,
                        int32_t* dense_count);
int jg_dc_series_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms);
int jg_dc_series_release(int64_t h);
int jg_dc_series_set_island_mode(int64_t h, int mode);
int jg_dc_series_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* branches, int64_t* buses, int64_t* m, int64_t* side);
int jg_dc_series_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow);
/*
 * The DC transfer-capability screen over transfers x N-1 outages (csrc/jg_dc_transfer.hpp): the user loop that raises the injections along a direction
 * with updateBus! / updateGenerator! around updateBranch!(k, status = 0), solve!, power! per branch until a monitored branch reaches its rating.  No
 * sweep per case: with Phi of jg_dc_pair_build, the base flows F0[m] and the flow sensitivities G[m,t] of the directions, the post-outage flow at
 * P0 + lambda d_t is f + lambda g with f = F0[m] + Phi[m,k] F0[k] / (1 - Phi[k,k]), g = G[m,t] + Phi[m,k] G[k,t] / (1 - Phi[k,k]), and the capability
 * TC(k,t) is the least (sign(g) rating_m - f) / g over the monitored, rated branches m != k with |g| > cutoff (negative: that branch is beyond the rating
 * at zero transfer; +inf: no such branch).  Needs jg_dc_set_branches and jg_dc_set_rhs; neither the lanes of the handle nor what jg_dc_pair_build and
 * jg_dc_series_build keep are touched.
 *   jg_dc_transfer_build  candidates [nk] and monitored [nm] as jg_dc_series_build takes them (nk >= 1); directions [transfers][n]: net active injection
 *                       per unit of transfer (no shunt, no shiftPower term; the slack's entry is ignored: the slack takes what a direction does not
 *                       balance).  base_rhs [n] (nullable): the right-hand side of a base profile as jg_dc_set_rhs takes it; NULL: the handle's own.
 *                       Phi by the build of jg_dc_pair_build, then one sweep pair per direction (512 at a time, scratch of the build's own) fills
 *                       G [rows][transfers rounded up to 64] doubles.  budget_bytes as jg_dc_pair_build, for Phi + G + the scratch of both: return code 5
 *                       with the sizes in the message and nothing allocated when they do not fit.  info [12]: the eight of jg_dc_pair_build, bytes of
 *                       G, and the milliseconds of its build: total, sweep pairs, G kernel.  A second build replaces the first.
 *   jg_dc_transfer_screen the cases (k, t) of the candidate POSITIONS k in [k0, k1) (0-based; the row block bounds the memory of a call, 12 bytes per
 *                       case) x all transfers against the ratings of jg_dc_set_rating; cutoff > 0 in per unit of flow per per unit of transfer.
 *                       amount [transfers] (nullable: no records): records [capacity][5] are the cases with TC(k,t) < amount[t], sorted by (k, t):
 *                       branch k (1-based), transfer t (0-based), limiting branch, TC, g of the limiting branch; ties of the limiting branch go to the
 *                       lowest index.  islanding [k1 - k0] (nullable): the candidates of the block that are bridges (|1 - Phi[k,k]| < 1e-9: status 3
 *                       and a NaN capability for every transfer; never in a record or a minimum), 1-based.
 *                       totals [5]: cases screened, cases below their amount, bridge candidates, records written, 1 when the record list overflowed --
 *                       the counts are exact also then, and the records kept are the FIRST by (k, t).
 *                       worst [nk] (nullable): positions k0 .. k1 - 1 get the least TC over the transfers (NaN on a bridge).  capability,
 *                       limiting_outage, limiting_branch [transfers] (nullable together, in/out): min-merged with the least TC over the block's
 *                       candidates (bridges aside), the candidate (1-based branch) and the branch that give it; ties go to the lowest candidate, so
 *                       the result of a caller that starts from +inf does not depend on the blocks.  base [transfers][3] (nullable): the base case of
 *                       every transfer, no outage -- TC, limiting branch (0: none), monitored branches above their rating at zero transfer.
 *                       dense_* (each nullable) [k1 - k0][transfers]: TC (NaN: bridge), the limiting branch (0: none).
 *   jg_dc_transfer_time_kernel   milliseconds of `reps` runs on rows [k0, k1) (a block jg_dc_transfer_screen has held): 0 the screen kernel, 1 the row /
 *                       column summaries behind it
 *   jg_dc_transfer_release  frees what the screen holds on the device
 * Bridge candidates screened on the slack's island, as for the series screen:
 *   jg_dc_transfer_set_island_mode the island mode of the NEXT jg_dc_transfer_build (0 / 1 as jg_dc_series_set_island_mode).  In mode 1 a branch that
 *                       leaves with a bridge candidate limits nothing; the case has a real TC and limiting branch (+inf and 0 when nothing eligible
 *                       stays) and enters the records and the minima like any other.
 *   jg_dc_transfer_get_shed_table  as jg_dc_series_get_shed_table.
 *   jg_dc_transfer_get_shed        flow [count]: what left m over the bridge at zero transfer; transfer [count][transfers]: per unit of each transfer
 *                       (not 0: the direction has a source or sink behind the bridge and is partly shed with it).
 */
int jg_dc_transfer_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t transfers,
                         const double* directions, const double* base_rhs, int64_t budget_bytes, double* info12);
int jg_dc_transfer_screen(int64_t h, int64_t k0, int64_t k1, double cutoff, const double* amount, int64_t capacity, double* records, int64_t* islanding,
                          int64_t* totals5, double* worst, double* capability, int64_t* limiting_outage, int64_t* limiting_branch, double* base,
                          double* dense_capability, int32_t* dense_branch);
int jg_dc_transfer_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms);
int jg_dc_transfer_release(int64_t h);
int jg_dc_transfer_set_island_mode(int64_t h, int mode);
int jg_dc_transfer_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* branches, int64_t* buses, int64_t* m, int64_t* side);
int jg_dc_transfer_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow, double* transfer);
/*
 * The DC generator-outage screen: G-1 and generator x branch cases (csrc/jg_dc_generator.hpp).  The user loop
 *     updateGenerator!(system, analysis; label = g, status = 0); solve!; power!                                (src/powerSystem/generator.jl:262-360, :433-446;
 *                                                                                                              src/powerFlow/dcPowerFlow.jl:63-134: row 0, G-1)
 *       updateBranch!(system, analysis; label = k, status = 0); solve!; power!; updateBranch!(...; status = 1)  (src/powerSystem/branch.jl: row k, per branch k)
 *     updateGenerator!(...; label = g, status = 1)
 * per generator g.  The loss of a unit moves the right-hand side alone, so a G-1 case needs no sweep of its own: with Psi[m,b], the flow on row m per unit
 * of injection at the generator bus b (ONE sweep pair per distinct generator bus), and A [generator buses x generators], the net change of the bus
 * injections per outage, F0[m,g] = f0[m] + sum_b Psi[m,b] A[b,g]; the case (k, g) is then f_m(k,g) = F0[m,g] + Phi[m,k] F0[k,g] / (1 - Phi[k,k]), the
 * arithmetic of jg_dc_series_screen with F0's columns for the profiles.  The reference refuses the loss of the slack bus's last unit
 * (generator.jl:441-445) and so does the caller of this screen; nothing here picks a new slack.  Needs jg_dc_set_branches and jg_dc_set_rhs; neither the
 * lanes of the handle nor what the other screens' builds keep are touched.
 *   jg_dc_generator_build  candidates [nk] and monitored [nm] as jg_dc_series_build takes them (nk >= 1).  buses [nbus]: the distinct generator buses
 *                       (1-based, strictly ascending; the slack's entry of a right-hand side is dropped, so the slack bus gets a zero column and is best
 *                       left out).  A in CSC: colptr [generators + 1] from 0, rowidx [colptr[generators]] 0-based POSITIONS in `buses`, values: column g
 *                       holds -Pg at g's bus (updateGenerator!(...; status = 0) takes Pg out of bus.supply.active) and what the units that pick the loss
 *                       up add at theirs; an empty column is the base case.  Phi by the build of jg_dc_pair_build, Psi [rows][nbus rounded up to 64] by
 *                       one sweep pair per generator bus (512 at a time, scratch of the build's own), then F0 [rows][generators rounded up to 64] by one
 *                       kernel.  budget_bytes as jg_dc_pair_build, for Phi + Psi + A + F0 + the scratch: return code 5 with the sizes in the message and
 *                       nothing allocated when they do not fit.  info [16]: the eight of jg_dc_pair_build, bytes of F0, the milliseconds of Psi's build:
 *                       total, sweep pairs, flow kernel, bytes of Psi, the milliseconds of the F0 kernel, generator buses swept, entries of A.  A second
 *                       build replaces the first.
 *   jg_dc_generator_screen  the cases (k, g) of the candidate POSITIONS k in [k0, k1) (0-based; the row block bounds the memory of a call, 16 bytes per
 *                       case) x all generators against the ratings of jg_dc_set_rating; a call with k0 = 0 also walks row 0, the G-1 cases.
 *                       records [capacity][5]: the cases whose worst loading exceeds threshold, sorted by (k, g) with row 0 first: branch k (1-based;
 *                       0: the G-1 case), generator column g (0-based), worst branch, worst |from| / rating, number of monitored branches above
 *                       threshold.  islanding [k1 - k0] (nullable): the candidates of the block that are bridges, as jg_dc_series_screen.
 *                       totals [5]: cases screened (row 0 counted where walked), violating, bridge candidates, records written, 1 when the record list
 *                       overflowed -- the counts are exact also then, and the records kept are the FIRST by (k, g).
 *                       worst [nk] (nullable): positions k0 .. k1 - 1 get the worst loading over the generators.  worst_generator [generators]
 *                       (nullable, in/out): max-merged with the worst loading over the rows walked, row 0 included; violating_generator [generators]
 *                       (nullable, in/out): the block's candidates whose outage beside the unit's violates are added.  base [generators][3] (nullable):
 *                       the G-1 cases -- worst loading, its branch, branches above threshold.  dense_* (each nullable) [k1 - k0][generators].
 *   jg_dc_generator_get_flows  flows [rows][generators]: F0, the from-end flows of every G-1 case on the rows of the build (info [0]: monitored and
 *                       candidate branches, ascending)
 *   jg_dc_generator_time_kernel  milliseconds of `reps` runs: 0 the screen kernel and 1 the summaries on rows [k0, k1) (a block
 *                       jg_dc_generator_screen has held), 2 the F0 kernel (k0, k1 ignored)
 *   jg_dc_generator_release  frees what the screen holds on the device
 *   jg_dc_generator_set_island_mode / _get_shed_table / _get_shed   as jg_dc_series_set_island_mode / _get_shed_table / _get_shed, with flow
 *                       [count][generators]: a unit behind a bridge candidate leaves with it, and its column is the shed case without the outage.
 */
int jg_dc_generator_build(int64_t h, int64_t nk, const int64_t* candidates, int64_t nm, const int64_t* monitored, int64_t generators, int64_t nbus,
                          const int64_t* buses, const int64_t* colptr, const int64_t* rowidx, const double* values, int64_t budget_bytes, double* info16);
int jg_dc_generator_screen(int64_t h, int64_t k0, int64_t k1, double threshold, int64_t capacity, double* records, int64_t* islanding, int64_t* totals5,
                           double* worst, double* worst_generator, int64_t* violating_generator, double* base, double* dense_load, int32_t* dense_branch,
                           int32_t* dense_count);
int jg_dc_generator_get_flows(int64_t h, double* flows);
int jg_dc_generator_time_kernel(int64_t h, int kernel, int64_t k0, int64_t k1, int reps, double* ms);
int jg_dc_generator_release(int64_t h);
int jg_dc_generator_set_island_mode(int64_t h, int mode);
int jg_dc_generator_get_shed_table(int64_t h, int64_t k0, int64_t k1, int64_t* count, int64_t* branches, int64_t* buses, int64_t* m, int64_t* side);
int jg_dc_generator_get_shed(int64_t h, int64_t k0, int64_t k1, double* flow);

/* ---------------------------------------------------------------------------------------------
 * DC state estimation with batched bad-data removal (csrc/jg_dcse.hip)
 * ------------------------------------------------------------------------------------------- */

/*
 * The handle is an int64 TOKEN (0 = none), like the DC power flow's.
 *
 * dcStateEstimation(monitoring)  -- src/stateEstimation/dcStateEstimation.jl:42-151 with the factorisation of the first solve! (:342-371): the slack's
 * column leaves the coefficient matrix H, G = H' W H with G[slack, slack] = 1 is assembled on the device from H's values x status x precision and
 * factorised ONCE (scalar LU on the elimination order and dependency levels of G's pattern, no pivoting: G is positive definite for an observable set).
 *   n, m            buses, rows of se.coefficient (wattmeters in stored order, then PMUs at buses)
 *   rowptr,col,val  H by rows: rowptr 0-based [m + 1], col 1-based and ascending inside a row, val with every status taken as 1 (the stored zeros of an
 *                   out-of-service row keep their pattern: a status change needs no new symbolic analysis)
 *   precision       1 / variance per row, out-of-service rows included;  status 0 / 1 per row
 *   slack           bus.layout.slack (1-based);  slack_angle = bus.voltage.angle[slack] (addSlackAngle!, src/backend/utility.jl:610-622)
 *   batch           realisations resident on the device (lanes, batch-minor with a leading dimension of batch rounded up to 64)
 * Return code 3: zero / non-finite pivot -- the set does not make the grid observable.
 * jg_dcse_dims: {n, m, batch, ld, entries of G, factor entries, factorisation levels, forward levels, backward levels, launches of a sweep pair, padded
 * sweep terms, numeric refactorisations since create, runs of the Omega diagonal, largest number of removed rows per lane}.
 * jg_dcse_set_weights: updateWattmeter! / updatePmu! of a status or a variance (src/measurement/powermeter.jl:704-757, pmu.jl:877-899, signature[:run]):
 * re-assembles G and refactorises numerically; the lanes' removed rows are forgotten.  A changed READING is jg_dcse_set_readings alone.
 */
int jg_dcse_create(int64_t* h, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* col, const double* val, const double* precision,
                   const int32_t* status, int64_t slack, double slack_angle, int64_t batch, int device);
void jg_dcse_destroy(int64_t h);
int jg_dcse_dims(int64_t h, int64_t* dims14);
int jg_dcse_set_weights(int64_t h, const double* precision, const int32_t* status);
/*
 * se.mean of lanes lane0 .. lane0 + count - 1, z [count][m] in row order (meanPi / meanPij / meanθi already applied, src/backend/equations.jl:121, 178,
 * 461; rows out of service are ignored).
 * jg_dcse_solve: solve!(analysis) for every lane (:342-371): b = H' W z, one sweep pair on the shared factor, one residual pass (objective).  correct = 1
 * (the Orthogonal / PetersWilkinson tags, :373-434): one more step theta += G^-1 H' W (z - H theta) on the same factor.  A lane with removed rows gets
 * theta' = x - U Omega_SS^-1 r_S (csrc/jg_dcse.hpp) instead of a refactorisation.
 *   jg_dcse_get_angle   theta [batch][n] = analysis.voltage.angle, status [batch] (0; 1: a removed row was critical -- without it the grid is unobservable;
 *                       2: more than the largest number of removed rows; both with NaN angles), objective [batch] = sum w r^2 of chiTest
 *                       (src/stateEstimation/badData.jl:963-977); each may be NULL
 * jg_dcse_residual_test: residualTest!(analysis; threshold) (badData.jl:48-117) for every lane: the largest normalised residual
 * |r_i| / sqrt(|1 / w_i - h_i G^-1 h_i'|) and its row (1-based, first on ties, 0: every residual is 0; rows out of service or with r == 0 are skipped).
 * The Omega diagonal is formed once per factor and shared by all lanes.  remove = 1: a lane whose maximum exceeds the threshold drops that row -- one
 * more sweep pair for its column of U; the next jg_dcse_solve compensates.  remove = 0 (a handle of batch 1 follows the reference: the caller sets the
 * status to 0 and calls jg_dcse_set_weights).
 *   jg_dcse_remove_rows               lane s drops row rows[s] (1-based, 0: none) whatever its residual: the caller knows the meter is bad
 *   jg_dcse_get_normalized_residual   every normalised residual of the current estimate, [batch][m]
 *   jg_dcse_get_removed               rows [batch][largest number] (1-based, 0: none), count [batch]
 *   jg_dcse_set_branches / jg_dcse_get_flows   power!(analysis) branch part (src/postprocessing/dcAnalysis.jl:106-131 with allPowerBranch): the arguments
 *                                     of jg_dc_set_branches; from [batch][branches], to = -from
 *   jg_dcse_time_kernel   milliseconds (HIP events) of `reps` runs of: 0 the chain of a batch, 1 the right-hand side, 2 the sweep pair, 3 the residual
 *                         pass, 4 the normalised residual pass, 5 the Omega diagonal + that pass; ms [reps]
 */
int jg_dcse_set_readings(int64_t h, int64_t lane0, int64_t count, const double* z);
int jg_dcse_solve(int64_t h, int correct);
int jg_dcse_get_angle(int64_t h, double* theta, int32_t* status, double* objective);
int jg_dcse_residual_test(int64_t h, double threshold, int remove, double* maximum, int32_t* index);
int jg_dcse_remove_rows(int64_t h, const int32_t* rows);
int jg_dcse_get_normalized_residual(int64_t h, double* r);
int jg_dcse_get_removed(int64_t h, int32_t* rows, int32_t* count);
int jg_dcse_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, const double* shift_angle);
int jg_dcse_get_flows(int64_t h, double* from);
int jg_dcse_time_kernel(int64_t h, int kernel, int reps, double* ms);
/* The critical-measurement and critical-pair screen of the handle's measurement set (csrc/jg_dcse_critical.hpp), on the same factor.  With
 * Omega = W^-1 - H G^-1 H': row i is CRITICAL when w_i Omega_ii <= 1e-6 (its residual is always 0; it takes part in no pair and is nobody's partner); a
 * pair i < j of other rows in service is CRITICAL when w_j (Omega_jj - Omega_ij^2 / Omega_ii) <= 1e-6 -- the pivot a lane meets that removes i, then j
 * (status 1); gamma_ij = Omega_ij / sqrt(Omega_ii Omega_jj) otherwise.
 *   jg_dcse_critical_screen   correlation < 0: critical pairs only; otherwise also the pairs with |gamma| >= correlation.  records [capacity][3]: the first
 *                             min(total, capacity) records (i, j, gamma), rows 1-based, sorted by (i, j), gamma = +-1 for the critical pairs and only for
 *                             them; totals [3] = {critical rows, critical pairs, further pairs at or above the correlation}, exact whatever the capacity;
 *                             single [m] (1: critical); partner [m] (the row of the largest |gamma_ij|, first on ties, 0: none -- out of service, critical,
 *                             or alone) and partner_gamma [m] (NaN where partner is 0).  records (capacity 0), single, partner, partner_gamma may be NULL.
 *                             Code 4 when lanes have removed rows: the screen is a property of the full set (jg_dcse_set_weights forgets the removals
 *                             and the screen then sees the new set).
 *   jg_dcse_critical_time_kernel   milliseconds (HIP events) of `reps` runs of the cross pass over all rows of H against the first block of 512 columns
 *   jg_dcse_get_variance      omega [m]: the Omega_ii of the full set the test and the screen use (formed if the factor is new; 1 / w_i for a row out
 *                             of service)
 */
int jg_dcse_critical_screen(int64_t h, double correlation, int64_t capacity, double* records, int64_t* totals, int32_t* single, int32_t* partner,
                            double* partner_gamma);
int jg_dcse_critical_time_kernel(int64_t h, int reps, double* ms);
int jg_dcse_get_variance(int64_t h, double* omega);
/* Branch status tests of the handle's measurement set (topology errors; csrc/jg_dcse_topology.hpp), on the same factor.  The hypothesis for branch k adds
 * ONE unknown phi to the model, z = c + H theta + m_k phi + e: the flow k really carries from -> to minus the flow the model gives it; m_k is +1 on the
 * from-end wattmeters of k and the injection wattmeters on from(k), -1 on the to-end wattmeters and the injection wattmeters on to(k).  With r the
 * residuals of the full set's estimate: D_k = m_k' W m_k - (H' W m_k)' G^-1 (H' W m_k), c_kl = m_k' W r_l, phi^_kl = c_kl / D_k, t_kl = c_kl / sqrt(D_k)
 * (N(0, 1) under "no error"; t^2 is the drop of the objective when phi is freed).  Candidates are numbered 1 .. count in the order of the call.
 *   jg_dcse_topology_set           the candidates: branch [count] (1-based, for messages), ptr [count + 1] (0-based offsets), row [] (1-based rows of the
 *                                  set, ascending in a column) and sign [] (+-1).  Rows out of service on the handle are masked by the library, so a
 *                                  changed status needs no new call.  Forgets the denominators (unless the candidates are the ones the handle holds), as
 *                                  every refactorisation does.
 *   jg_dcse_topology_denominators  D [count], norm [count] = m_k' W m_k, status [count] (0 testable: D > 1e-6 norm; 1 critical branch: a status error on it
 *                                  leaves no residual; 2 unseen: no meter in service sees it), formed per block of 512 candidates by one sweep pair if the
 *                                  candidates or the factor are new and kept on the handle; runs: how often they were formed.  Every pointer may be NULL; with `runs` alone nothing is formed.
 *   jg_dcse_topology_screen        needs a solved handle whose lanes removed nothing (code 1 otherwise).  records [capacity][4]: the first
 *                                  min(total, capacity) records (lane, candidate, t, phi^) with |t| >= threshold, 1-based, sorted by (lane, candidate);
 *                                  totals [2] = {records, lanes with at least one}, exact whatever the capacity; lane_best [batch] the candidate of the
 *                                  largest |t| (the lowest on ties; 0: none is testable), lane_t, lane_phi [batch] (NaN there), lane_count [batch];
 *                                  dense_t [count][batch] every statistic (NaN where the status is not 0).  records (capacity 0) and everything after
 *                                  totals may be NULL.
 *   jg_dcse_topology_correct       angle [batch][n]: the estimate of lane l corrected for candidate[l], theta' = theta^ - G^-1 H' W m_k phi^_kl, the WLS
 *                                  estimate of the augmented problem; candidate <= 0 or not testable: the lane's estimate bit for bit as
 *                                  jg_dcse_get_angle gives it.  The handle's estimate is left as it is.
 *   jg_dcse_topology_time          milliseconds (HIP events) of `reps` runs of: 0 all denominators, 1 the right-hand sides, 2 the sweep pair, 3 the
 *                                  denominator kernel (1-3: the first block of 512 candidates), 4 the screen's statistic pass, 5 the correction
 */
int jg_dcse_topology_set(int64_t h, int64_t count, const int64_t* branch, const int64_t* ptr, const int64_t* row, const int32_t* sign);
int jg_dcse_topology_denominators(int64_t h, double* D, double* norm, int32_t* status, int64_t* runs);
int jg_dcse_topology_screen(int64_t h, double threshold, int64_t capacity, double* records, int64_t* totals, int32_t* lane_best, double* lane_t,
                            double* lane_phi, int32_t* lane_count, double* dense_t);
int jg_dcse_topology_correct(int64_t h, const int32_t* candidate, double* angle);
int jg_dcse_topology_time(int64_t h, int kernel, int reps, double* ms);

/* ---------------------------------------------------------------------------------------------
 * Gauss-Seidel AC power flow, one scenario per lane (csrc/jg_gs.hip).  The handle is an int64 token, as for jg_dc_*.
 *
 * A sweep is sequential over the buses of a scenario and scenarios are independent, so a lane runs the reference's update sequence unchanged on its own
 * column of the batch-minor voltages, and a whole powerFlow! is ONE launch: every lane runs mismatch, verdict, sweep until it converges, reaches the
 * limit or turns non-finite.  Indices and positions are 1-based; complex values are (re, im) pairs; per-lane arrays are [batch][n].
 *
 *   jg_gs_create         gaussSeidel(system) (src/powerFlow/acPowerFlow.jl:563-619).  colptr / rowval: the pattern of nodalMatrix; yt: the values of
 *                        nodalMatrixTranspose -- row i of Ybus is yt[j], rowval[j] for j in colptr[i] .. colptr[i + 1] - 1, the walk of :742-744 and
 *                        :1002-1009; type [n]: 1 demand, 2 generator, 3 on the slack bus alone (pq / pv of :575-584 are the buses of type 1 / 2 in bus
 *                        order); setpoint [n]: generator.voltage.magnitude of the FIRST in-service generator of a bus (:1032-1033), read at type-2 buses
 *   jg_gs_destroy
 *   jg_gs_set_ybus       new values on the same pattern, after updateBranch! / updateBus!(shunt) (src/powerSystem/branch.jl:473-475: the analysis reads
 *                        the system's matrix)
 *   jg_gs_set_injection  bus.supply - bus.demand (active, reactive) of lanes lane0 .. lane0 + count - 1, as :747-750 and :998-1000 read them; stride 0:
 *                        one [n] pair for every lane of the range, stride n: [count][n]
 *   jg_gs_set_setpoint   setpoint [n] again, after updateGenerator!(...; magnitude) (src/powerSystem/generator.jl:410-431)
 *   jg_gs_set_voltage    method.voltage = magnitude * cis(angle) (:576, setInitialPoint! :1243-1245, :1289-1291); stride 0: one [n] pair for all lanes
 *   jg_gs_set_voltage_rect  method.voltage = re + i im, bit for bit: what moves the state of a live analysis to a new handle when the pattern of the
 *                        nodal matrix grew (addBranch! between two buses without an entry); strides as jg_gs_set_voltage
 *   jg_gs_set_bus_voltage  method.voltage[bus] = magnitude[s] * cis(angle[s]) of every lane s, the other buses untouched: _updateBus!
 *                        (src/powerSystem/bus.jl:350-362) and _updateGenerator! (generator.jl:425-430)
 *   jg_gs_get_voltage    magnitude, angle = absang(method.voltage) (:1012, :1035) and / or method.voltage itself as re, im; either pair may be NULL
 *   jg_gs_set_outages    lane lane0 + s = the grid with one branch out of service (updateBranch!(analysis; label, status = 0), branch.jl:344-350): its 4
 *                        positions in yt (0: none) and the 4 complex values added there.  The position of Ybus entry (row, col) in yt is the position of
 *                        (col, row) in nodalMatrix
 *   jg_gs_mismatch       mismatch!(analysis) (:732-764) of every lane -> stop_p, stop_q [batch]
 *   jg_gs_solve          solve!(analysis) (:997-1038) of every lane: one sweep, the lanes' iteration counts go up by one
 *   jg_gs_run            powerFlow!(analysis; iteration, tolerance) (:1389-1433) of every lane in one launch -> iterations, status [batch]: 0 converged,
 *                        1 the iteration limit, 3 a mismatch maximum that is not finite (an outage left a bus without admittance)
 *   jg_gs_get_mismatch   the maxima of the last jg_gs_mismatch / the last check of jg_gs_run
 *   jg_gs_time_kernel    milliseconds (HIP events) of `reps` runs of: 0 jg_gs_run's launch with `sweeps` as the limit and tolerance 0 (no lane leaves
 *                        early), 1 the mismatch, 2 one sweep; ms [reps].  The voltages move on as they do in the calls timed
 * ------------------------------------------------------------------------------------------- */
int jg_gs_create(int64_t* h, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* yt, const int8_t* type, int64_t slack,
                 const double* setpoint, int64_t batch, int device);
void jg_gs_destroy(int64_t h);
int jg_gs_set_ybus(int64_t h, const double* yt);
int jg_gs_set_injection(int64_t h, int64_t lane0, int64_t count, const double* active, const double* reactive, int64_t stride);
int jg_gs_set_setpoint(int64_t h, const double* setpoint);
int jg_gs_set_voltage(int64_t h, const double* magnitude, const double* angle, int64_t stride);
int jg_gs_set_voltage_rect(int64_t h, const double* re, const double* im, int64_t stride);
int jg_gs_set_bus_voltage(int64_t h, int64_t bus, const double* magnitude, const double* angle);
int jg_gs_get_voltage(int64_t h, double* magnitude, double* angle, double* re, double* im);
int jg_gs_set_outages(int64_t h, int64_t lane0, int64_t count, const int64_t* position, const double* delta);
int jg_gs_mismatch(int64_t h, double* stop_p, double* stop_q);
int jg_gs_solve(int64_t h);
int jg_gs_run(int64_t h, int64_t iteration, double tolerance, int32_t* iterations, int32_t* status);
int jg_gs_get_mismatch(int64_t h, double* stop_p, double* stop_q);
int jg_gs_time_kernel(int64_t h, int kernel, int64_t sweeps, int reps, double* ms);

/* ---------------------------------------------------------------------------------------------
 * Batched DC optimal power flow: ADMM (OSQP's reduced form) on one shared factor (csrc/jg_dcopf.hip).  The handle is an int64 token.
 *
 * Every lane solves  min 1/2 x' P x + q' x  subject to  l <= A x <= u  with P (its diagonal), q and A shared and l, u its own.  Indices are 1-based;
 * per-lane arrays are [batch][rows or variables].  A bound at or beyond +-1e20 (or infinite) is none.
 *
 *   jg_dcopf_create      P [n] >= 0, q [n], A [m][n] as CSR (columns of a row ascending), equality [m] 1 on rows that are equalities in every lane (they
 *                        get 1e3 rho); rho, sigma, alpha: the step sizes and the relaxation.  The objective is scaled by 1 / max(|P|, |q|), the rows
 *                        of A to unit 2-norm; K = P + sigma I + A' rho A is analysed, assembled from its term lists and factorised once.
 *   jg_dcopf_host_model  no device: the same host set-up -> K [n][n] dense from the term lists at (rho, sigma), the objective's scale, the rows' scales [m]
 *   jg_dcopf_dims        n, m, batch, ld, entries of K, entries of the factor, factorisation levels, refactorisations, 1 if K is singular but for sigma
 *   jg_dcopf_set_bounds  l, u [batch][m]
 *   jg_dcopf_set_start   x [batch][n], y [batch][m] as jg_dcopf_get returns them; z = A x.  Without it a handle starts at 0 and a later run goes on
 *                        from where the last one ended
 *   jg_dcopf_run         iterates until every lane is solved (both residuals of the scaled problem <= tolerance + tolerance x their norms), shown
 *                        primal infeasible, or at max_iteration; the residuals are formed every `check` iterations, rho follows the unfinished
 *                        lanes' median residual ratio at multiples of adapt_every (0: never; a multiple of check) -> iterations, status [batch]:
 *                        0 solved, 2 primal infeasible, 5 iteration limit, 3 K singular; the count of numeric refactorisations so far
 *   jg_dcopf_get         x [batch][n], y, z [batch][m] and the objective [batch] of the unscaled problem (each may be NULL)
 *   jg_dcopf_time        milliseconds (HIP events) of `reps` runs of: 0 one iteration, 1 the right-hand side, 2 the sweep pair, 3 the projection step,
 *                        4 the residual pass and verdict, 5 assembly of K and refactorisation, 6 the outaged lanes' correction of the solve, 7 the build
 *                        of their W = K^-1 [a d] and 2 x 2 inverses (6, 7: with a set of outages); ms [reps].  The iterates move on as they do in the
 *                        calls timed
 *   jg_dcopf_set_branch_outages  one branch out per lane, without a factorisation of its own: from_variable, to_variable [batch] the variables of the
 *                        branch's buses f, t; from_row, to_row [batch] their balance rows r_f, r_t (equality rows); admittance [batch] y_k as A holds it
 *                        (unscaled: the library applies the rows' scales and rho); state [batch] 0 none, 1 outage, 3 the outage is a bridge (the
 *                        lane is not run: status 3, NaN).  The lane's matrix is A + p d', p = -y_k (e_rf - e_rt), d = e_f - e_t, solved on the shared
 *                        factor by a rank-2 correction; the caller frees the branch's own rows through their bounds.  A call replaces the set; state
 *                        NULL clears it.  x, y, z stay (the warm start)
 * ------------------------------------------------------------------------------------------- */
int jg_dcopf_create(int64_t* h, int64_t n, int64_t m, const double* P, const double* q, const int64_t* rowptr, const int64_t* col, const double* val,
                    const int32_t* equality, int64_t batch, double rho, double sigma, double alpha, int device);
void jg_dcopf_destroy(int64_t h);
int jg_dcopf_host_model(int64_t n, int64_t m, const double* P, const double* q, const int64_t* rowptr, const int64_t* col, const double* val,
                        const int32_t* equality, double rho, double sigma, double* K, double* cscale, double* E);
int jg_dcopf_dims(int64_t h, int64_t* dims);
int jg_dcopf_get_rho(int64_t h, double* rho);
int jg_dcopf_set_bounds(int64_t h, const double* l, const double* u);
int jg_dcopf_set_start(int64_t h, const double* x, const double* y);
int jg_dcopf_run(int64_t h, double tolerance, int64_t max_iteration, int64_t check, int64_t adapt_every, int32_t* iterations, int32_t* status,
                 int64_t* refactorisations);
int jg_dcopf_get(int64_t h, double* x, double* y, double* z, double* objective);
int jg_dcopf_time(int64_t h, int kernel, int reps, double* ms);
int jg_dcopf_set_branch_outages(int64_t h, const int64_t* from_variable, const int64_t* to_variable, const int64_t* from_row, const int64_t* to_row,
                                const double* admittance, const int32_t* state);

/* ---------------------------------------------------------------------------------------------
 * Batched DC least-absolute-value state estimation: a primal-dual interior-point method per lane on a lane-valued factor of the gain
 * (csrc/jg_dclav.hip, csrc/jg_dc_lanefactor.hip).  The handle is an int64 token.
 *
 * Every lane solves  min |z - H theta|_1  over the in-service rows of ONE coefficient matrix H with readings z of its own, the slack's angle fixed
 * (the reference's dcLavStateEstimation, unweighted; a weighted model is a scaled H and z).  Indices are 1-based; per-lane arrays are [batch][rows or
 * buses].  The gain H' Q H has a diagonal Q per lane and iteration: its pattern is analysed once, its values are assembled and factorised per lane.
 *
 *   jg_dclav_create        rows of H as CSR (columns of a row ascending), status [m] 0 / 1, the slack bus and its angle.  The device memory of `batch`
 *                          lanes is computed first: a batch that does not fit is refused with code 5 and the sizes in the message
 *   jg_dclav_dims          n, m, batch, ld, entries of G, entries of the factor, factorisation levels, forward levels, backward levels, launches of a
 *                          sweep pair, bytes per lane, in-service rows, lane-valued factorisations so far, iterations of the last solve: dims [14]
 *   jg_dclav_set_readings  z [count][m] of lanes lane0 .. (se.mean: the constants of the rows already taken out)
 *   jg_dclav_set_status    status [m]: a changed row set re-runs the start of the next solve and nothing symbolic
 *   jg_dclav_set_initial   theta [batch][n] (the slack's angle included) replaces the unit-weight least-squares estimate in the start of the NEXT solve
 *   jg_dclav_solve         iterates until every lane is finished or at `iteration`: max |rp| <= tol (1 + max |z|), max |rd| <= tol max_j sum_i |H_ij|,
 *                          gap <= tol (1 + |z - H theta|_1).  Every call starts anew (interior-point iterations are not warm-started)
 *   jg_dclav_get_angle     theta [batch][n], status [batch] (0 solved, 5 iteration limit, 1 the in-service rows do not observe the grid: every lane,
 *                          NaN; 3 a zero or non-finite pivot in a later iteration of that lane, frozen at its last iterate), objective [batch],
 *                          iterations [batch] (each may be NULL)
 *   jg_dclav_get_residual  z - H theta [batch][m] on in-service rows, 0 elsewhere
 *   jg_dclav_get_dual      y [batch][m] and the complementarity gap [batch] (each may be NULL)
 *   jg_dclav_set_branches / jg_dclav_get_flows   as jg_dcse_set_branches / jg_dcse_get_flows
 *   jg_dclav_factor_solve  the lane-valued factor alone: q [batch][m] the lanes' weights, rhs [batch][n] -> x = (H' Q H)^-1 rhs [batch][n] (the slack's
 *                          row and column the identity), bad [batch] 1 where the lane met a zero or non-finite pivot.  The handle needs a new solve
 *   jg_dclav_time_kernel   milliseconds (HIP events) of `reps` runs, every lane running, of: 0 a whole iteration but its update, 1 the assembly, 2 the
 *                          factorisation, 3 one sweep pair, 4 the row, column and step passes; ms [reps].  The iterates stay
 * ------------------------------------------------------------------------------------------- */
int jg_dclav_create(int64_t* h, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, int64_t slack,
                    double slack_angle, int64_t batch, int device);
void jg_dclav_destroy(int64_t h);
int jg_dclav_dims(int64_t h, int64_t* dims);
int jg_dclav_set_readings(int64_t h, int64_t lane0, int64_t count, const double* z);
int jg_dclav_set_status(int64_t h, const int32_t* status);
int jg_dclav_set_initial(int64_t h, const double* theta);
int jg_dclav_solve(int64_t h, int iteration, double tolerance);
int jg_dclav_get_angle(int64_t h, double* theta, int32_t* status, double* objective, int32_t* iterations);
int jg_dclav_get_residual(int64_t h, double* r);
int jg_dclav_get_dual(int64_t h, double* y, double* gap);
int jg_dclav_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, const double* shift);
int jg_dclav_get_flows(int64_t h, double* from);
int jg_dclav_factor_solve(int64_t h, const double* q, const double* rhs, double* x, int32_t* bad);
int jg_dclav_time_kernel(int64_t h, int kernel, int reps, double* ms);

/* ---------------------------------------------------------------------------------------------
 * Batched DC Huber / Schweppe-Huber state estimation: the interior-point method of jg_dclav_* on the Huber QP, per lane, on the same lane-valued factor
 * (csrc/jg_dchuber.hip, csrc/jg_dc_lanefactor.hip).  The handle is an int64 token.
 *
 * Every lane solves  min sum_i rho_kappa_i(z_i - h_i theta)  (rho Huber's function: r^2 / 2 up to kappa, kappa |r| - kappa^2 / 2 beyond) over the in-service
 * rows of ONE coefficient matrix H with readings z of its own, the slack's angle fixed.  The caller scales row i of H and z by 1 / sigma_i, so the
 * weights are 1; kappa [m] > 0 is shared by the lanes (c for Huber, c omega_i for Schweppe's leverage weights).  Shapes are those of jg_dclav_*.
 *
 *   jg_dchuber_create        as jg_dclav_create, with kappa [m] and sigma [m] (NULL: 1; what a scaled residual is multiplied by on its way out)
 *   jg_dchuber_dims          as jg_dclav_dims: dims [14]
 *   jg_dchuber_set_readings  scaled z [count][m] of lanes lane0 ..
 *   jg_dchuber_set_status    status [m]: a changed row set re-runs the start of the next solve and nothing symbolic
 *   jg_dchuber_set_bounds    kappa [m]: new bounds; the next solve starts anew, as every solve does
 *   jg_dchuber_solve         iterates until every lane is finished or at `iteration`: max |rp| <= tol (1 + max |z|), max |rd| <= tol max_j sum_i |H_ij|
 *                            max kappa, gap <= tol (1 + y'y / 2 + kappa'(u + v))
 *   jg_dchuber_get_angle     theta [batch][n], status [batch] (0 solved, 5 iteration limit, 1 the in-service rows do not observe the grid: every lane,
 *                            NaN; 3 a zero or non-finite pivot in a later iteration of that lane, frozen at its last iterate), objective [batch] (the
 *                            Huber loss of the scaled residuals), iterations [batch] (each may be NULL)
 *   jg_dchuber_get_residual  sigma_i (z_i - h_i theta) [batch][m], the UNSCALED residual, on in-service rows, 0 elsewhere
 *   jg_dchuber_get_weight    min(1, kappa_i / |scaled residual|) [batch][m], 1 on rows out of service
 *   jg_dchuber_get_dual      y [batch][m] (the clipped scaled residual at the optimum) and the complementarity gap [batch] (each may be NULL)
 *   jg_dchuber_set_branches / jg_dchuber_get_flows   as jg_dcse_set_branches / jg_dcse_get_flows
 *   jg_dchuber_time_kernel   as jg_dclav_time_kernel
 * ------------------------------------------------------------------------------------------- */
int jg_dchuber_create(int64_t* h, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, const double* kappa,
                      const double* sigma, int64_t slack, double slack_angle, int64_t batch, int device);
void jg_dchuber_destroy(int64_t h);
int jg_dchuber_dims(int64_t h, int64_t* dims);
int jg_dchuber_set_readings(int64_t h, int64_t lane0, int64_t count, const double* z);
int jg_dchuber_set_status(int64_t h, const int32_t* status);
int jg_dchuber_set_bounds(int64_t h, const double* kappa);
int jg_dchuber_solve(int64_t h, int iteration, double tolerance);
int jg_dchuber_get_angle(int64_t h, double* theta, int32_t* status, double* objective, int32_t* iterations);
int jg_dchuber_get_residual(int64_t h, double* r);
int jg_dchuber_get_weight(int64_t h, double* w);
int jg_dchuber_get_dual(int64_t h, double* y, double* gap);
int jg_dchuber_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, const double* shift);
int jg_dchuber_get_flows(int64_t h, double* from);
int jg_dchuber_time_kernel(int64_t h, int kernel, int reps, double* ms);

/* ---------------------------------------------------------------------------------------------
 * Batched PMU least-absolute-value state estimation: the interior-point method of jg_dclav_* on the linear phasor model, WITHOUT a fixed state, per
 * lane (csrc/jg_pmulav.hip, csrc/jg_dclav.hip, csrc/jg_dc_lanefactor.hip).  The handle is an int64 token.
 *
 * Every lane solves  min sum_i |z_i - h_i x|  over the in-service rows of ONE coefficient matrix H [2 pmus][2 buses] with phasor readings of its own.
 * States: re(1 .. buses) then im(1 .. buses).  Rows: 2 i the real, 2 i + 1 the imaginary part of PMU i (0-based); status is per PMU (a PMU whose magnitude
 * or angle channel is off leaves with both rows).  Arrays are [batch][...] on the host.
 *
 *   jg_pmulav_create        rows of H as CSR (columns of a row ascending, 1-based), status [pmus] 0 / 1.  The device memory of `batch` lanes is computed
 *                           first and refused with the sizes (code 5) before anything is allocated
 *   jg_pmulav_dims          dims [14] as jg_dclav_dims, with buses, pmus in [0], [1] and the in-service PMUs in [11]
 *   jg_pmulav_set_readings  magnitude, angle [count][pmus] of lanes lane0 ..: z_re = magnitude cos(angle), z_im = magnitude sin(angle) are formed on the device
 *   jg_pmulav_set_status    status [pmus]: a changed set re-runs the start of the next solve and nothing symbolic
 *   jg_pmulav_set_scale     scale [2 pmus] > 0, ONE for every lane: what a row's reading is multiplied by (the caller scales the rows of H); the residuals
 *                           of jg_pmulav_get_residual and the objective are the scaled rows', rho of jg_pmulav_suspect is unscaled
 *   jg_pmulav_set_initial   magnitude, angle [batch][buses] replace the unit-weight least-squares estimate in the start of the NEXT solve
 *   jg_pmulav_solve         as jg_dclav_solve
 *   jg_pmulav_get_voltage   magnitude, angle [batch][buses], status [batch] (0 solved, 5 iteration limit, 1 a state no in-service row touches -- an exact
 *                           zero pivot of the unit-weight start: every lane, NaN; 3 a zero or non-finite pivot in a later iteration of that lane),
 *                           objective [batch], iterations [batch] (each may be NULL)
 *   jg_pmulav_get_residual  z - H x [batch][2 pmus] on in-service rows, 0 elsewhere
 *   jg_pmulav_get_dual      y [batch][2 pmus] and the complementarity gap [batch] (each may be NULL)
 *   jg_pmulav_set_branches  from, to (1-based), status and param [nbr][16] as jg_nr_set_branches; the buses' shunt conductance and susceptance
 *   jg_pmulav_get_flows     per lane and branch [batch][nbr][2]: from, to and series current (magnitude, angle), from, to, series and charging power
 *                           (active, reactive); per lane and bus [batch][buses][2] the injected power.  Out-of-service branches give 0.  Each may be NULL
 *   jg_pmulav_suspect       rho [batch][pmus] = |residual phasor| (0 for a PMU outside the model), flag [batch][pmus] = rho > threshold (per unit),
 *                           count [batch] the flagged devices, worst [batch] the device (0-based) of the largest rho, the lowest on ties (each may be NULL)
 *   jg_pmulav_time_kernel   milliseconds (HIP events) of `reps` runs: 0 .. 4 the parts of jg_dclav_time_kernel, 5 the polar -> rectangular pass, 6 the
 *                           rectangular -> polar pass, 7 the branch and bus pass, 8 the suspect pass
 * ------------------------------------------------------------------------------------------- */
int jg_pmulav_create(int64_t* h, int64_t buses, int64_t pmus, const int64_t* rowptr, const int64_t* col, const double* val, const int32_t* status, int64_t batch,
                     int device);
void jg_pmulav_destroy(int64_t h);
int jg_pmulav_dims(int64_t h, int64_t* dims);
int jg_pmulav_set_readings(int64_t h, int64_t lane0, int64_t count, const double* magnitude, const double* angle);
int jg_pmulav_set_status(int64_t h, const int32_t* status);
int jg_pmulav_set_scale(int64_t h, const double* scale);
int jg_pmulav_set_initial(int64_t h, const double* magnitude, const double* angle);
int jg_pmulav_solve(int64_t h, int iteration, double tolerance);
int jg_pmulav_get_voltage(int64_t h, double* magnitude, double* angle, int32_t* status, double* objective, int32_t* iterations);
int jg_pmulav_get_residual(int64_t h, double* r);
int jg_pmulav_get_dual(int64_t h, double* y, double* gap);
int jg_pmulav_set_branches(int64_t h, int64_t nbr, const int64_t* from, const int64_t* to, const int8_t* status, const double* param, const double* shunt_g,
                           const double* shunt_b);
int jg_pmulav_get_flows(int64_t h, double* from_i, double* to_i, double* series_i, double* from_pq, double* to_pq, double* series_pq, double* charging_pq,
                        double* injection_pq);
int jg_pmulav_suspect(int64_t h, double threshold, double* rho, int32_t* flag, int32_t* count, int32_t* worst);
int jg_pmulav_time_kernel(int64_t h, int kernel, int reps, double* ms);

/* ---------------------------------------------------------------------------------------------
 * Symbolic analysis only (no device needed): the static schedule that replaces the symbolic half
 * of `lu`/`klu` (src/backend/utility.jl:470-476, 486-492).  Used by the CPU test-suite to replay
 * and race-check the schedule.  pattern: 0-based int32 block CSR, structurally symmetric, full
 * diagonal.  policy: bit 0 in-place factor storage, bit 1 symmetric values (LDL'), bit 2 the producer finishes level 0 (the
 * leaf pivots: factorised diagonal blocks + rhs rows; csrc/jg_symbolic.hpp), bits 4-7 / 8-15 / 16-23 / 24-30 where the
 * multifrontal top starts and how large its fronts get (0 = defaults), bits 32-39 / 40-47 / 48 the grouped tasks below the
 * top (csrc/jg_symbolic.hpp: "mid"), bit 49 Jordan rows for the pivots of the top tasks + the backward tables over them (what
 * jg_nr_create / jg_gn_create ask for; csrc/jg_symbolic.hpp).  jg_plan_export(which): see csrc/jg_plan_api.cpp;
 * out == NULL returns the length.
 * ------------------------------------------------------------------------------------------- */
typedef struct jg_plan jg_plan;
int jg_plan_create(jg_plan** p, int64_t n, const int32_t* rowptr, const int32_t* col, int64_t policy);
void jg_plan_destroy(jg_plan* p);
int64_t jg_plan_export(jg_plan* p, int which, int32_t* out, int64_t cap);
/* The tables of the shared-factor solve behind jg_nr_base_create (csrc/jg_symbolic.hpp: CompTables) for a dense top of at most top_cap pivots (< 0: none):
 * which = 0 {top pivots, split level, forward levels, backward levels}, 1 the top's pivots, 2 / 3 forward segments (x 8) / records (x 16), 4 / 5 backward. */
int64_t jg_plan_comp_export(jg_plan* p, int64_t top_cap, int which, int32_t* out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* JGRID_H */
