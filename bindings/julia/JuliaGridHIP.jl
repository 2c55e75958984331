# JuliaGridHIP.jl -- ccall shim that plugs libjgrid_hip.so (include/jgrid.h) behind JuliaGrid's own
# newtonRaphson() / mismatch!() / solve!() / powerFlow!() and gaussNewton() / increment!() / solve!() / stateEstimation!()
# surface.  Written against JuliaGrid v0.6.2; it has NOT been executed (no Julia toolchain in the build containers) --
# see INTEGRATION.md for the one-token patch of the reference it needs and for how every row below maps to the C ABI.
#
# The analyses are the REFERENCE'S OWN structs, parametrised by a new solver tag:
#     AcPowerFlow{NewtonRaphson{HIP}}          (src/definition/analysis.jl:154-164, 252-258)
#     AcStateEstimation{GaussNewton{HIP}}      (src/definition/analysis.jl:532-545, 643-650)
# so the reference's generic loops powerFlow! (src/powerFlow/acPowerFlow.jl:1389-1433) and stateEstimation!
# (src/stateEstimation/acStateEstimation.jl:1286-1329), its printing, power!/current! and every reader of
# analysis.voltage.{magnitude,angle} / analysis.method.{jacobian,mismatch,increment,residual,iteration} work unchanged;
# what dispatches here are the methods that do numerics.
#
#   reference method (file:line)                                        -> C ABI
#   newtonRaphson(system, T)             acPowerFlow.jl:39-87           -> jg_nr_create, jg_nr_set_injection, jg_nr_set_voltage
#   mismatch!(analysis)                  acPowerFlow.jl:645-685         -> jg_nr_mismatch, jg_nr_get_mismatch
#   solve!(analysis)                     acPowerFlow.jl:793-911         -> jg_nr_solve, jg_nr_get_increment, jg_nr_get_voltage
#   powerFlow!(analysis)  (fused)        acPowerFlow.jl:1389-1433       -> jg_nr_run, jg_nr_get_voltage, jg_nr_get_iteration
#   setInitialPoint!(analysis)           acPowerFlow.jl:1226-1249       -> jg_nr_set_voltage
#   updateBus!/Branch!/Generator!        bus.jl:286, branch.jl:453, generator.jl:382 -> jg_nr_set_injection, jg_nr_set_ybus
#   gaussNewton(monitoring, T)           acStateEstimation.jl:43-75     -> jg_gn_create, jg_gn_set_measurement, jg_gn_set_voltage
#   increment!(analysis)                 acStateEstimation.jl:878-904   -> jg_gn_increment, jg_gn_get_increment, jg_gn_get_residual
#   solve!(analysis)                     acStateEstimation.jl:1035-1047 -> jg_gn_solve, jg_gn_get_voltage
#   stateEstimation!(analysis) (fused)   acStateEstimation.jl:1286-1329 -> jg_gn_run, jg_gn_get_voltage
#   setInitialPoint!(analysis)           acStateEstimation.jl:1071      -> jg_gn_set_voltage
#   update<Meter>!(analysis; ...)        measurement/*.jl               -> jg_gn_set_status, jg_gn_set_measurement
#   residualTest!(analysis)  (numerics)  badData.jl:181-311             -> jg_gn_residual_test, jg_gn_get_normalized_residual
#   fastNewtonRaphsonBX/XB(system, T)    acPowerFlow.jl:215-537         -> jg_nr_create, jg_nr_fast_setup
#   mismatch!/solve!/powerFlow! (fast)   acPowerFlow.jl:687-730, 913-983 -> jg_nr_fast_mismatch, jg_nr_fast_solve, jg_nr_fast_run, jg_nr_fast_get_increment
#   power!(analysis), current!(analysis) postprocessing/acAnalysis.jl:30-169, 672-704 -> jg_nr_set_branches, jg_nr_bus_injection, jg_nr_branch_quantities
#   gaussNewton(monitoring, HIPOrthogonal)  (Orthogonal / PetersWilkinson rows) acStateEstimation.jl:906-971 -> jg_gn_set_method
#   pmuStateEstimation(monitoring, T), solve!  pmuStateEstimation.jl:43-177, 369-399 -> jg_gn_create (codes 22-27), jg_gn_increment, jg_gn_solve
#   chiTest(analysis)                    badData.jl:948-995             -> jg_gn_evaluate, jg_gn_get_residual (se.objective)
#   Monte-Carlo batch (user loop over add<Meter>!(noise = true) + stateEstimation!, measurement/utility.jl:70-73) -> jg_gn_run on a batch,
#                                        jg_gn_get_objective, jg_gn_pack_results_device, jg_gn_allgather_results
module JuliaGridHIP

using JuliaGrid
using SparseArrays
import JuliaGrid: newtonRaphson, fastNewtonRaphsonBX, fastNewtonRaphsonXB, gaussSeidel, gaussNewton, pmuStateEstimation, mismatch!, solve!, increment!,
                  powerFlow!, stateEstimation!, setInitialPoint!, power!, current!, chiTest,
                  updateBus!, updateBranch!, updateGenerator!, reactiveLimit!, adjustAngle!,
                  updateVoltmeter!, updateAmmeter!, updateWattmeter!, updateVarmeter!, updatePmu!,
                  AcPowerFlow, AcStateEstimation, PmuStateEstimation, NewtonRaphson, FastNewtonRaphson, FastNewtonRaphsonModel, GaussNewton, WLS,
                  PowerSystem, Measurement, LU

const lib = get(ENV, "JGRID_HIP_LIB", "libjgrid_hip.so")

"""
    HIP <: Normal

Solver tag: `newtonRaphson(system, HIP)`, `gaussNewton(monitoring, HIP)`.  `GaussNewton{T <: WlsMethod}` accepts it as it
is; `NewtonRaphson{T <: Union{LU, KLU, QR}}` needs its bound widened to `T <: Normal` (INTEGRATION.md, one token).
"""
struct HIP <: JuliaGrid.Normal end

"""
    HIPOrthogonal <: WlsMethod

`gaussNewton(monitoring, HIPOrthogonal)` / `pmuStateEstimation(monitoring, HIPOrthogonal)`: what the `Orthogonal` and `PetersWilkinson` tags of
the reference are for (acStateEstimation.jl:906-971: an increment whose error does not carry the squared condition number of the gain matrix), on the
device: the corrected semi-normal equations on the factor the engine holds (`jg_gn_set_method(h, 1)`, include/jgrid.h).  Diagonal precision only, as
in the reference (`sqrtPrecision!`).
"""
struct HIPOrthogonal <: JuliaGrid.WlsMethod end

# The structs type their `factorization` field with the FactorSparse union; the device factor lives behind the C handle, so the
# field keeps an (unused) LU placeholder and the handle is found through the method object.
JuliaGrid.selectFactorization(::Type{HIP}) = JuliaGrid.selectFactorization(LU)
JuliaGrid.selectFactorization(::Type{HIPOrthogonal}) = JuliaGrid.selectFactorization(LU)

mutable struct Handle
    ptr::Ptr{Cvoid}
    kind::Symbol                                  # :nr | :gn
    function Handle(p, kind)
        h = new(p, kind)
        finalizer(h) do x
            x.ptr == C_NULL && return
            x.kind === :nr ? ccall((:jg_nr_destroy, lib), Cvoid, (Ptr{Cvoid},), x.ptr) :
                             ccall((:jg_gn_destroy, lib), Cvoid, (Ptr{Cvoid},), x.ptr)
            x.ptr = C_NULL
        end
        return h
    end
end
const HANDLES = WeakKeyDict{Any, Handle}()        # analysis.method (a mutable struct) -> device handle
handle(analysis) = HANDLES[analysis.method].ptr

check(rc) = rc == 0 ? nothing :
    throw(ErrorException(unsafe_string(ccall((:jg_last_error, lib), Cstring, ()))))

reim(z::AbstractVector{ComplexF64}) = collect(reinterpret(Float64, z))

const HipTag = Union{HIP, HIPOrthogonal}
const HipPowerFlow = AcPowerFlow{NewtonRaphson{HIP}}
const HipFastPowerFlow = AcPowerFlow{FastNewtonRaphson{HIP}}          # needs `FastNewtonRaphson{T <: Normal}` / `FastNewtonRaphsonModel{T <: Normal}` (INTEGRATION.md)
const HipAnyPowerFlow = Union{HipPowerFlow, HipFastPowerFlow}
const HipStateEstimation = Union{AcStateEstimation{GaussNewton{HIP}}, AcStateEstimation{GaussNewton{HIPOrthogonal}}}
const HipPmuStateEstimation = Union{PmuStateEstimation{WLS{HIP}}, PmuStateEstimation{WLS{HIPOrthogonal}}}

# ------------------------------------------------------------------------------------------------------------------
# Newton-Raphson AC power flow
# ------------------------------------------------------------------------------------------------------------------
function pushInjection!(analysis::HipAnyPowerFlow)
    bus = analysis.system.bus
    p = bus.supply.active .- bus.demand.active
    q = bus.supply.reactive .- bus.demand.reactive
    check(ccall((:jg_nr_set_injection, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), handle(analysis), p, q, 0))
end

pushVoltage!(analysis::HipAnyPowerFlow) =
    check(ccall((:jg_nr_set_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64),
        handle(analysis), analysis.voltage.magnitude, analysis.voltage.angle, 0))

pullVoltage!(analysis::HipAnyPowerFlow) =
    check(ccall((:jg_nr_get_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
        handle(analysis), analysis.voltage.magnitude, analysis.voltage.angle))

function pushYbus!(analysis::HipAnyPowerFlow)
    ac = analysis.system.model.ac
    check(ccall((:jg_nr_set_ybus, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
        handle(analysis), reim(ac.nodalMatrix.nzval), reim(ac.nodalMatrixTranspose.nzval)))
end

"""
    newtonRaphson(system, HIP; device = 0)

Same set-up as `newtonRaphson(system, LU)` (bus-type normalisation, start voltages, index maps: done by the reference itself),
with the Jacobian pattern, the symbolic analysis and all per-iteration numerics on the GPU.  One scenario, like every
analysis of the reference; batches go through `NewtonRaphsonBatch`.
"""
function newtonRaphson(system::PowerSystem, ::Type{HIP}; device::Int = 0)
    base = newtonRaphson(system, LU)                          # host bookkeeping of the reference: maps, containers, start point
    m = base.method
    method = NewtonRaphson{HIP}(m.jacobian, m.mismatch, m.increment, JuliaGrid.selectFactorization(HIP), m.pq, m.pvpq, m.pcount,
        m.signature, 0)
    analysis = AcPowerFlow(base.voltage, base.power, base.current, method, system)
    ac = system.model.ac
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:jg_nr_create, lib), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int8}, Int64, Int64, Int64, Cint),
        h, system.bus.number, ac.nodalMatrix.colptr, ac.nodalMatrix.rowval,
        reim(ac.nodalMatrix.nzval), reim(ac.nodalMatrixTranspose.nzval),
        system.bus.layout.type, system.bus.layout.slack, 1, 0, device))
    HANDLES[method] = Handle(h[], :nr)
    pushInjection!(analysis)
    pushVoltage!(analysis)
    return analysis
end

function staleCheck(analysis::HipAnyPowerFlow)                  # acPowerFlow.jl:802-811
    rev, sig = analysis.system.model.revision, analysis.method.signature
    (rev.topology != sig.topology || rev.type != sig.type) && JuliaGrid.errorTypeConversion()
    if sig.acPattern != -1 && rev.acPattern != sig.acPattern  # addBranch!/dropZeros! changed the Ybus pattern: new handle
        throw(ErrorException("The Ybus pattern changed; build a new analysis with newtonRaphson(system, HIP)."))
    end
    sig.acPattern = rev.acPattern
end

function mismatch!(analysis::HipPowerFlow)                   # acPowerFlow.jl:645-685
    maxp = Ref(0.0); maxq = Ref(0.0)
    check(ccall((:jg_nr_mismatch, lib), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), handle(analysis), maxp, maxq))
    check(ccall((:jg_nr_get_mismatch, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), analysis.method.mismatch))
    return maxp[], maxq[]
end

function solve!(analysis::HipPowerFlow)                      # acPowerFlow.jl:793-911
    staleCheck(analysis)
    check(ccall((:jg_nr_solve, lib), Cint, (Ptr{Cvoid},), handle(analysis)))     # code 3 = singular Jacobian -> ErrorException
    check(ccall((:jg_nr_get_increment, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), analysis.method.increment))
    pullVoltage!(analysis)
    analysis.method.iteration += 1
    return nothing
end

"method.jacobian at the current state, in the reference's CSC order (only when somebody looks: it stays on the device)"
function jacobian!(analysis::HipPowerFlow)
    check(ccall((:jg_nr_get_jacobian, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), analysis.method.jacobian.nzval))
    return analysis.method.jacobian
end

"""
    powerFlow!(analysis::AcPowerFlow{NewtonRaphson{HIP}}; iteration, tolerance, power, current)

The reference's loop (acPowerFlow.jl:1389-1433) with the same accounting, run on the device without a host round trip per
iteration.  The generic `powerFlow!` of the reference also works on this analysis (it only calls `mismatch!` / `solve!`).
"""
function powerFlow!(analysis::HipPowerFlow; iteration::Int64 = 20, tolerance::Float64 = 1e-8, power::Bool = false,
                    current::Bool = false, verbose::Int64 = 0)
    staleCheck(analysis)
    iters = Vector{Int32}(undef, 1); status = Vector{Int32}(undef, 1)
    check(ccall((:jg_nr_run, lib), Cint, (Ptr{Cvoid}, Int64, Float64, Ptr{Int32}, Ptr{Int32}),
        handle(analysis), iteration, tolerance, iters, status))
    pullVoltage!(analysis)
    check(ccall((:jg_nr_get_mismatch, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), analysis.method.mismatch))
    check(ccall((:jg_nr_get_increment, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), analysis.method.increment))
    analysis.method.iteration = iters[1]
    status[1] == 3 && throw(ErrorException("The Jacobian is singular."))        # SingularException of the reference's lu!
    power && power!(analysis)
    current && current!(analysis)
    return nothing
end

# ---- fast Newton-Raphson BX / XB (acPowerFlow.jl:215-537): the two constant matrices go to the device as values per stored Ybus entry and
# ---- are factorised there once; an iteration is two forward / backward sweeps on the device
function fastModel(system::PowerSystem, bx::Bool, device::Int)
    base = bx ? fastNewtonRaphsonBX(system, LU) : fastNewtonRaphsonXB(system, LU)     # B', B'', numbering, start point: the reference's own set-up
    m = base.method
    act = FastNewtonRaphsonModel{HIP}(m.active.jacobian, m.active.mismatch, m.active.increment, JuliaGrid.selectFactorization(HIP))
    rea = FastNewtonRaphsonModel{HIP}(m.reactive.jacobian, m.reactive.mismatch, m.reactive.increment, JuliaGrid.selectFactorization(HIP))
    method = FastNewtonRaphson{HIP}(act, rea, m.pq, m.pvpq, m.signature, bx, 0)
    analysis = AcPowerFlow(base.voltage, base.power, base.current, method, system)
    ac, bus = system.model.ac, system.bus
    Y = ac.nodalMatrix
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:jg_nr_create, lib), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int8}, Int64, Int64, Int64, Cint),
        h, bus.number, Y.colptr, Y.rowval, reim(Y.nzval), reim(ac.nodalMatrixTranspose.nzval), bus.layout.type, bus.layout.slack, 1, 0, device))
    HANDLES[method] = Handle(h[], :nr)
    pushFast!(analysis)
    pushInjection!(analysis)
    pushVoltage!(analysis)
    return analysis
end

"B'[pvpq r, pvpq c] and B''[pq r, pq c] at every stored Ybus entry (r, c); identity on the diagonal / zero elsewhere outside the reduced matrices"
function pushFast!(analysis::HipFastPowerFlow)
    system, m = analysis.system, analysis.method
    Y, typ, slack = system.model.ac.nodalMatrix, system.bus.layout.type, system.bus.layout.slack
    bp = zeros(nnz(Y)); bq = zeros(nnz(Y))
    for c = 1:system.bus.number, p = Y.colptr[c]:(Y.colptr[c + 1] - 1)
        r = Y.rowval[p]
        bp[p] = (typ[r] != 3 && c != slack) ? m.active.jacobian[m.pvpq[r], m.pvpq[c]] : (r == c ? 1.0 : 0.0)
        bq[p] = (typ[r] == 1 && typ[c] == 1) ? m.reactive.jacobian[m.pq[r], m.pq[c]] : (r == c ? 1.0 : 0.0)
    end
    check(ccall((:jg_nr_fast_setup, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), handle(analysis), bp, bq))
end

fastNewtonRaphsonBX(system::PowerSystem, ::Type{HIP}; device::Int = 0) = fastModel(system, true, device)
fastNewtonRaphsonXB(system::PowerSystem, ::Type{HIP}; device::Int = 0) = fastModel(system, false, device)

function mismatch!(analysis::HipFastPowerFlow)               # acPowerFlow.jl:687-730
    m = analysis.method
    maxp = Ref(0.0); maxq = Ref(0.0)
    check(ccall((:jg_nr_fast_mismatch, lib), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), handle(analysis), maxp, maxq))
    both = Vector{Float64}(undef, length(m.active.mismatch) + length(m.reactive.mismatch))       # [active.mismatch | reactive.mismatch]
    check(ccall((:jg_nr_get_mismatch, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), both))
    m.active.mismatch .= view(both, 1:length(m.active.mismatch))
    m.reactive.mismatch .= view(both, (length(m.active.mismatch) + 1):length(both))
    return maxp[], maxq[]
end

function pullFastIncrement!(analysis::HipFastPowerFlow)
    m = analysis.method
    both = Vector{Float64}(undef, length(m.active.increment) + length(m.reactive.increment))     # [active.increment | reactive.increment]
    check(ccall((:jg_nr_fast_get_increment, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), both))
    m.active.increment .= view(both, 1:length(m.active.increment))
    m.reactive.increment .= view(both, (length(m.active.increment) + 1):length(both))
end

function solve!(analysis::HipFastPowerFlow)                  # acPowerFlow.jl:913-983
    staleCheck(analysis)
    check(ccall((:jg_nr_fast_solve, lib), Cint, (Ptr{Cvoid},), handle(analysis)))
    pullFastIncrement!(analysis)
    pullVoltage!(analysis)
    analysis.method.iteration += 1
    return nothing
end

function powerFlow!(analysis::HipFastPowerFlow; iteration::Int64 = 20, tolerance::Float64 = 1e-8, power::Bool = false,
                    current::Bool = false, verbose::Int64 = 0)
    staleCheck(analysis)
    iters = Vector{Int32}(undef, 1); status = Vector{Int32}(undef, 1)
    check(ccall((:jg_nr_fast_run, lib), Cint, (Ptr{Cvoid}, Int64, Float64, Ptr{Int32}, Ptr{Int32}),
        handle(analysis), iteration, tolerance, iters, status))
    pullVoltage!(analysis)
    pullFastIncrement!(analysis)
    analysis.method.iteration = iters[1]
    status[1] == 3 && throw(ErrorException("The Jacobian is singular."))
    power && power!(analysis)
    current && current!(analysis)
    return nothing
end

# ---- power!(analysis) / current!(analysis) (postprocessing/acAnalysis.jl:30-169, 672-704): the Ybus row walk (injections) and the branch formulas run on
# ---- the device at the state the handle holds; the O(n) bus / generator bookkeeping is the reference's own (its power! runs first, the device
# ---- quantities then replace what it computed for injections and branches)
const BRANCHES = WeakKeyDict{Any, Bool}()                    # analysis.method -> the branch table is on the device

function pushBranches!(analysis::HipAnyPowerFlow)
    get(BRANCHES, analysis.method, false) && return
    system = analysis.system
    ac, br = system.model.ac, system.branch
    nb = br.number
    param = zeros(16, nb)                                     # [nb][16] row-major (jgrid.h: jg_nr_set_branches)
    for k = 1:nb
        tij = (1.0 / br.parameter.turnsRatio[k]) * cis(-br.parameter.shiftAngle[k])      # acAnalysis.jl:846-851
        for (c, z) in enumerate((ac.nodalFromFrom[k], ac.nodalFromTo[k], ac.nodalToFrom[k], ac.nodalToTo[k], ac.admittance[k], tij))
            param[2c - 1, k] = real(z); param[2c, k] = imag(z)
        end
        param[13, k] = br.parameter.conductance[k]; param[14, k] = br.parameter.susceptance[k]; param[15, k] = 1.0 / br.parameter.turnsRatio[k]
    end
    check(ccall((:jg_nr_set_branches, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int8}, Ptr{Float64}),
        handle(analysis), nb, br.layout.from, br.layout.to, Int8.(br.layout.status), param))
    BRANCHES[analysis.method] = true
end

function power!(analysis::HipAnyPowerFlow)
    invoke(power!, Tuple{AcPowerFlow}, analysis)              # containers, shunt, supply, generator allocation: the reference's bookkeeping
    pushBranches!(analysis)
    n, nb, pw = analysis.system.bus.number, analysis.system.branch.number, analysis.power
    inj = Matrix{Float64}(undef, 2, n)                        # [n][2] row-major
    check(ccall((:jg_nr_bus_injection, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), inj))
    pw.injection.active .= view(inj, 1, :); pw.injection.reactive .= view(inj, 2, :)
    from = Matrix{Float64}(undef, 2, nb); to = similar(from); series = similar(from); charging = similar(from)
    check(ccall((:jg_nr_branch_quantities, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        handle(analysis), from, to, series, charging, C_NULL, C_NULL, C_NULL))
    for (dst, src) in ((pw.from, from), (pw.to, to), (pw.series, series), (pw.charging, charging))
        dst.active .= view(src, 1, :); dst.reactive .= view(src, 2, :)
    end
    return nothing
end

function current!(analysis::HipAnyPowerFlow)
    invoke(current!, Tuple{JuliaGrid.AC}, analysis)           # containers + injection currents (O(n) from the injections)
    pushBranches!(analysis)
    nb, cu = analysis.system.branch.number, analysis.current
    from = Matrix{Float64}(undef, 2, nb); to = similar(from); series = similar(from)
    check(ccall((:jg_nr_branch_quantities, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        handle(analysis), C_NULL, C_NULL, C_NULL, C_NULL, from, to, series))
    for (dst, src) in ((cu.from, from), (cu.to, to), (cu.series, series))
        dst.magnitude .= view(src, 1, :); dst.angle .= view(src, 2, :)
    end
    return nothing
end

function setInitialPoint!(analysis::HipPowerFlow)            # acPowerFlow.jl:1226-1249
    invoke(setInitialPoint!, Tuple{AcPowerFlow}, analysis)
    pushVoltage!(analysis)
end

function setInitialPoint!(target::HipPowerFlow, source::JuliaGrid.AC)   # acPowerFlow.jl:1281-1295
    invoke(setInitialPoint!, Tuple{AcPowerFlow, JuliaGrid.AC}, target, source)
    pushVoltage!(target)
end

function updateBus!(analysis::HipPowerFlow; label, kwargs...)           # bus.jl:286-298
    invoke(updateBus!, Tuple{AcPowerFlow}, analysis; label, kwargs...)
    pushInjection!(analysis); pushYbus!(analysis)                       # demand / shunt edits
    pushVoltage!(analysis)                                              # magnitude / angle keywords
end

function updateBranch!(analysis::HipPowerFlow; label, kwargs...)        # branch.jl:453-459 (pattern kept: stored zeros, model.jl:70-71)
    invoke(updateBranch!, Tuple{JuliaGrid.PowerFlow}, analysis; label, kwargs...)
    pushYbus!(analysis)
    delete!(BRANCHES, analysis.method)                                  # the branch table of power! / current! goes up again on the next call
end

function updateGenerator!(analysis::HipPowerFlow; label, kwargs...)     # generator.jl:382-388
    invoke(updateGenerator!, Tuple{JuliaGrid.PowerFlow}, analysis; label, kwargs...)
    pushInjection!(analysis)
    pushVoltage!(analysis)
end

# ---- batched scenarios (no counterpart in the reference, which loops updateBranch!/powerFlow! per outage, SURVEY.md 3.5) ----
"""
    NewtonRaphsonBatch(system, batch; device = 0, maxPatch = 4)

`batch` scenarios of one grid that share the Ybus pattern: per-scenario injections, start points and up to `maxPatch` Ybus
edits (an outage = the 4 edits acNodalUpdate! makes, model.jl:93-101).  Results are [n, batch] matrices / [batch] vectors.
"""
mutable struct NewtonRaphsonBatch
    system::PowerSystem
    batch::Int
    handle::Handle
    magnitude::Matrix{Float64}
    angle::Matrix{Float64}
    iteration::Vector{Int32}
    status::Vector{Int32}                          # 0 converged, 1 iteration limit, 3 numeric failure (singular Jacobian / NaN)
    outage::Vector{Int64}                          # branch out of service per scenario (0: none), for branchQuantities
end

function NewtonRaphsonBatch(system::PowerSystem, batch::Int; device::Int = 0, maxPatch::Int = 4)
    base = newtonRaphson(system, LU)
    ac = system.model.ac
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:jg_nr_create, lib), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int8}, Int64, Int64, Int64, Cint),
        h, system.bus.number, ac.nodalMatrix.colptr, ac.nodalMatrix.rowval, reim(ac.nodalMatrix.nzval),
        reim(ac.nodalMatrixTranspose.nzval), system.bus.layout.type, system.bus.layout.slack, batch, maxPatch, device))
    b = NewtonRaphsonBatch(system, batch, Handle(h[], :nr), zeros(system.bus.number, batch), zeros(system.bus.number, batch),
        zeros(Int32, batch), zeros(Int32, batch), zeros(Int64, batch))
    bus = system.bus
    check(ccall((:jg_nr_set_injection, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), b.handle.ptr,
        bus.supply.active .- bus.demand.active, bus.supply.reactive .- bus.demand.reactive, 0))
    check(ccall((:jg_nr_set_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), b.handle.ptr,
        base.voltage.magnitude, base.voltage.angle, 0))
    return b
end

"""
    shareDevice!(batch, on = true)

Hint for a pipeline of several batches in flight on one GPU (`jg_nr_set_shared`): the top of the factorisation runs the kernel variant that
leaves room on a compute unit for the other batches' workgroups.  Results are bitwise unchanged.
"""
shareDevice!(b::NewtonRaphsonBatch, on::Bool = true) =
    check(ccall((:jg_nr_set_shared, lib), Cint, (Ptr{Cvoid}, Cint), b.handle.ptr, on ? 1 : 0))

"""
    keepIncrement!(batch, on = true)

`on = false`: the batch no longer stores `method.increment` in bus order (`jg_nr_set_keep_increment`): every sweep and lane compaction moves 16 bytes per
bus and scenario less, voltages, iteration counts and status are bitwise unchanged, and reading the increment raises until the switch is on again and
the batch has run.  A screen that reads voltages and branch records only switches it off.
"""
keepIncrement!(b::NewtonRaphsonBatch, on::Bool = true) =
    check(ccall((:jg_nr_set_keep_increment, lib), Cint, (Ptr{Cvoid}, Cint), b.handle.ptr, on ? 1 : 0))

"scenario s (1-based) = base grid with branch labels[s] out of service (0: base case); one upload for the whole batch"
function setOutages!(b::NewtonRaphsonBatch, labels::Vector{Int64})
    length(labels) == b.batch || throw(DimensionMismatch("one label per scenario"))
    ac, Y, lay = b.system.model.ac, b.system.model.ac.nodalMatrix, b.system.branch.layout
    ptr = zeros(Int64, 4, b.batch); dy = zeros(Float64, 2, 4, b.batch)
    position(r, c) = Y.colptr[c] + searchsortedfirst(view(Y.rowval, Y.colptr[c]:(Y.colptr[c + 1] - 1)), r) - 1
    for (s, k) in enumerate(labels)
        k == 0 && continue
        i, j = lay.from[k], lay.to[k]
        ptr[:, s] = [position(i, i), position(j, j), position(i, j), position(j, i)]
        for (m, v) in enumerate((ac.nodalFromFrom[k], ac.nodalToTo[k], ac.nodalFromTo[k], ac.nodalToFrom[k]))
            dy[1, m, s], dy[2, m, s] = -real(v), -imag(v)
        end
    end
    check(ccall((:jg_nr_patch_ybus_batch, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
        b.handle.ptr, 0, b.batch, 4, ptr, dy))
    b.outage .= labels
    return nothing
end

function powerFlow!(b::NewtonRaphsonBatch; iteration::Int64 = 20, tolerance::Float64 = 1e-8)
    check(ccall((:jg_nr_run, lib), Cint, (Ptr{Cvoid}, Int64, Float64, Ptr{Int32}, Ptr{Int32}),
        b.handle.ptr, iteration, tolerance, b.iteration, b.status))              # [batch] outputs
    check(ccall((:jg_nr_get_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
        b.handle.ptr, b.magnitude, b.angle))                                     # [batch][n] row-major = [n, batch] column-major
    return nothing
end

"""
    branchQuantities(batch; currents = false) -> (from, to, series, charging) | (from, to, series)

`power!` / `current!` of the branches for EVERY scenario of the batch at its current state (acAnalysis.jl:898-931), each `[2, nb, batch]`
(active | reactive resp. magnitude | angle); the branch that is out of service in a scenario (`setOutages!`) reads zero there.
"""
function branchQuantities(b::NewtonRaphsonBatch; currents::Bool = false)
    system = b.system
    ac, br = system.model.ac, system.branch
    nb = br.number
    param = zeros(16, nb)
    for k = 1:nb
        tij = (1.0 / br.parameter.turnsRatio[k]) * cis(-br.parameter.shiftAngle[k])
        for (c, z) in enumerate((ac.nodalFromFrom[k], ac.nodalFromTo[k], ac.nodalToFrom[k], ac.nodalToTo[k], ac.admittance[k], tij))
            param[2c - 1, k] = real(z); param[2c, k] = imag(z)
        end
        param[13, k] = br.parameter.conductance[k]; param[14, k] = br.parameter.susceptance[k]; param[15, k] = 1.0 / br.parameter.turnsRatio[k]
    end
    check(ccall((:jg_nr_set_branches, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int8}, Ptr{Float64}),
        b.handle.ptr, nb, br.layout.from, br.layout.to, Int8.(br.layout.status), param))
    check(ccall((:jg_nr_set_outage_labels, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), b.handle.ptr, b.outage))
    out = [Array{Float64}(undef, 2, nb, b.batch) for _ = 1:(currents ? 3 : 4)]
    if currents
        check(ccall((:jg_nr_branch_quantities, lib), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            b.handle.ptr, C_NULL, C_NULL, C_NULL, C_NULL, out[1], out[2], out[3]))
    else
        check(ccall((:jg_nr_branch_quantities, lib), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            b.handle.ptr, out[1], out[2], out[3], out[4], C_NULL, C_NULL, C_NULL))
    end
    return Tuple(out)
end

"""
    screenSummary(batch; rating = nothing, record = nothing) -> Matrix [10, batch]

Contingency screen summary on the device (jgrid.h: jg_nr_screen): per scenario the worst branch loading against `rating` (pu of apparent power per branch,
0 = no limit) and its branch, the largest apparent power at a branch end and its branch, the lowest / highest voltage magnitude and their buses,
iterations, status -- what the user loop of branch.jl:453-459 reads off power!(analysis) after every powerFlow!, reduced where the states are.
`record`: a DEVICE pointer for `10 * batch` doubles instead (the operand of `allgatherDevice` in a sharded screen).
"""
function screenSummary(b::NewtonRaphsonBatch; rating::Union{Nothing, Vector{Float64}} = nothing, record::Union{Nothing, Ptr{Float64}} = nothing)
    branchQuantities(b; currents = true)                      # uploads the branch table and the outage labels (and is cheap: three outputs)
    if rating === nothing
        check(ccall((:jg_nr_set_screen, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, C_NULL))
    else
        check(ccall((:jg_nr_set_screen, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, rating))
    end
    if record !== nothing
        check(ccall((:jg_nr_screen_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, record))
        return nothing
    end
    rec = Matrix{Float64}(undef, 10, b.batch)
    check(ccall((:jg_nr_screen, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, rec))
    return rec
end

# ---- straggler hand-off between batches (jgrid.h: jg_nr_run_defer ...): a pipeline of batches stops a batch once <= deferAt
# scenarios are active, moves them into a POOL batch that collects the stragglers of several batches, and finishes them together
# (what ContingencyPipeline(pool = ...) does on the Python side; a Julia driver runs batches from Threads.@spawn tasks).
"runs until at most `deferAt` (<= 64) scenarios are still active; returns their number (0: the batch is done).  Follow with
moveLanes!(pool, lane0, b) if any are left, then finish!(b)."
function powerFlowDefer!(b::NewtonRaphsonBatch; iteration::Int64 = 20, tolerance::Float64 = 1e-8, deferAt::Int64 = 64)
    left = Ref{Int32}(0)
    check(ccall((:jg_nr_run_defer, lib), Cint, (Ptr{Cvoid}, Int64, Float64, Int64, Ref{Int32}),
        b.handle.ptr, iteration, tolerance, deferAt, left))
    return Int(left[])
end

"the still-active scenarios of the paused batch `src` continue in lanes lane0 + 1, ... of `pool`; returns their (1-based)
scenario numbers in `src`, in lane order; in `src` they end with status 4 (deferred)"
function moveLanes!(pool::NewtonRaphsonBatch, lane0::Int, src::NewtonRaphsonBatch)
    home = zeros(Int32, 64); count = Ref{Int32}(0)
    check(ccall((:jg_nr_move_lanes, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int32}, Ref{Int32}),
        pool.handle.ptr, lane0, src.handle.ptr, home, count))
    return Int.(home[1:count[]]) .+ 1
end

"ends a paused run: iteration / status of every scenario (4 = handed to a pool), voltages of the others"
function finish!(b::NewtonRaphsonBatch)
    check(ccall((:jg_nr_finish, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}), b.handle.ptr, b.iteration, b.status))
    check(ccall((:jg_nr_get_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), b.handle.ptr, b.magnitude, b.angle))
    return nothing
end

"runs the scenarios in lanes 1:lanes of a pool to the end, each with the iteration count it arrived with"
function resume!(pool::NewtonRaphsonBatch, lanes::Int; iteration::Int64 = 20, tolerance::Float64 = 1e-8)
    check(ccall((:jg_nr_resume, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Float64, Ptr{Int32}, Ptr{Int32}),
        pool.handle.ptr, lanes, iteration, tolerance, pool.iteration, pool.status))    # first `lanes` entries are written
    check(ccall((:jg_nr_get_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), pool.handle.ptr, pool.magnitude, pool.angle))
    return nothing
end

# ---- the first iteration of a screen on ONE shared factor (jgrid.h: jg_nr_base_*): the reference refactorises per scenario of its loop
# (branch.jl:453-459 + acPowerFlow.jl:890-897); batches whose scenarios all start from one base case pay one factorisation per BASE CASE
"""
    BaseCase(system; device = 0, topCap = 0, iteration = 20, tolerance = 1e-8)

Solves the power flow of `system` (one instance on the device), then factorises the Jacobian at that solution ONCE and keeps what the batches
attached to it need for a compensated first iteration (J0^-1 on the Ybus pattern, J0^-1 f0, the dense inverse of the top of the elimination tree:
`topCap` pivots at most, 0 = default).  The state it was built at is the start of every attached batch (`startFromBase!`).
"""
mutable struct BaseCase
    system::PowerSystem
    ptr::Ptr{Cvoid}
    function BaseCase(system::PowerSystem; device::Int = 0, topCap::Int = 0, iteration::Int64 = 20, tolerance::Float64 = 1e-8)
        single = NewtonRaphsonBatch(system, 1; device = device, maxPatch = 0)
        powerFlow!(single; iteration = iteration, tolerance = tolerance)
        single.status[1] == 0 || throw(ErrorException("BaseCase: the power flow of the base case did not converge"))
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:jg_nr_base_create, lib), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64), h, single.handle.ptr, topCap))
        b = new(system, h[])
        finalizer(x -> (x.ptr == C_NULL || ccall((:jg_nr_base_destroy, lib), Cvoid, (Ptr{Cvoid},), x.ptr); x.ptr = C_NULL), b)
        return b
    end
end

"(pivots in the dense top, split level, forward / backward level launches of a sweep pair, the same two without a top, creation time in microseconds, attached batches)"
function baseInfo(base::BaseCase)
    info = zeros(Int64, 8)
    check(ccall((:jg_nr_base_info, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), base.ptr, info))
    return info
end

"J0^-1 on the stored Ybus pattern, `[4, nnz]` (a 2 x 2 block (theta_i, V_i) x (P_j, Q_j) per stored entry, row-major, in row-CSR order of the pattern) -- test access"
function baseInverseOnPattern(base::BaseCase)
    nnz = length(base.system.model.ac.nodalMatrix.nzval)
    out = zeros(Float64, 4, nnz)
    check(ccall((:jg_nr_base_get, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64), base.ptr, 0, out, length(out)))
    return out
end

"the scenarios of `b` may start from `base` (same grid and device); `nothing` detaches"
function attach!(b::NewtonRaphsonBatch, base::Union{BaseCase, Nothing})
    check(ccall((:jg_nr_attach_base, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), b.handle.ptr, base === nothing ? C_NULL : base.ptr))
    return nothing
end

"every scenario of `b` starts from the attached base case's state (what setInitialPoint!(analysis, base) is per scenario of the reference's loop,
acPowerFlow.jl:1271-1295); the next powerFlow! / powerFlowDefer! takes its first iteration on the base's shared factor when it can (jgrid.h lists the conditions)"
function startFromBase!(b::NewtonRaphsonBatch)
    check(ccall((:jg_nr_start_from_base, lib), Cint, (Ptr{Cvoid},), b.handle.ptr))
    return nothing
end

"shared = false: the first iteration refactorises like every other (A/B switch)"
firstIteration!(b::NewtonRaphsonBatch, shared::Bool = true) =
    check(ccall((:jg_nr_set_first_iteration, lib), Cint, (Ptr{Cvoid}, Cint), b.handle.ptr, shared ? 1 : 0))

"(runs of `b` that started on the shared factor, runs that refactorised)"
function firstIterationCounts(b::NewtonRaphsonBatch)
    a = Ref{Int64}(0); r = Ref{Int64}(0)
    check(ccall((:jg_nr_first_iteration_counts, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), b.handle.ptr, a, r))
    return Int(a[]), Int(r[])
end

# ------------------------------------------------------------------------------------------------------------------
# Gauss-Newton WLS state estimation
# ------------------------------------------------------------------------------------------------------------------
# Type code of every Jacobian row BEFORE status masking, in acWLS's row order (acStateEstimation.jl:135-235): the library
# rebuilds the H pattern from (code, index) and needs the code of a masked row as well (se.type holds status * code).
function typeCodes(monitoring::Measurement)
    volt, amp, watt, var, pmu = monitoring.voltmeter, monitoring.ammeter, monitoring.wattmeter, monitoring.varmeter, monitoring.pmu
    code = Int8[]; status = Int8[]; corr = Int64[]
    for i = 1:volt.number
        push!(code, 1); push!(status, volt.magnitude.status[i])
    end
    for i = 1:amp.number
        sq, from = amp.layout.square[i], amp.layout.from[i]
        push!(code, sq ? (from ? 4 : 5) : (from ? 2 : 3)); push!(status, amp.magnitude.status[i])
    end
    for i = 1:watt.number
        push!(code, watt.layout.bus[i] ? 6 : (watt.layout.from[i] ? 7 : 8)); push!(status, watt.active.status[i])
    end
    for i = 1:var.number
        push!(code, var.layout.bus[i] ? 9 : (var.layout.from[i] ? 10 : 11)); push!(status, var.reactive.status[i])
    end
    for i = 1:pmu.number
        sm, sa, from = pmu.magnitude.status[i], pmu.angle.status[i], pmu.layout.from[i]
        if pmu.layout.polar[i]
            if pmu.layout.bus[i]
                append!(code, (12, 13))
            else
                append!(code, (pmu.layout.square[i] ? (from ? 4 : 5) : (from ? 2 : 3), from ? 14 : 15))
            end
            append!(status, (sm, sa))
        else
            pmu.layout.correlated[i] && push!(corr, length(code) + 1)
            append!(code, pmu.layout.bus[i] ? (16, 17) : (from ? (18, 20) : (19, 21)))
            append!(status, (sm * sa, sm * sa))
        end
    end
    return code, status, corr
end

function pushMeasurement!(analysis::HipStateEstimation)       # se.mean, se.precision (diagonal + W[r, r+1] of correlated pairs)
    se = analysis.method
    _, _, corr = typeCodes(analysis.monitoring)
    W = se.precision
    wdiag = [W[r, r] for r = 1:length(se.mean)]
    woff = Float64[W[r, r + 1] for r in corr]
    check(ccall((:jg_gn_set_measurement, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64),
        handle(analysis), se.mean, wdiag, isempty(woff) ? [0.0] : woff, 0, 0))
end

function pushStatus!(analysis::HipStateEstimation)            # update<Meter>!(...; status, square): se.type = status * code
    code, status, _ = typeCodes(analysis.monitoring)
    check(ccall((:jg_gn_set_status, lib), Cint, (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int8}), handle(analysis), status, code))
end

pushVoltage!(analysis::HipStateEstimation) =
    check(ccall((:jg_gn_set_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64),
        handle(analysis), analysis.voltage.magnitude, analysis.voltage.angle, 0))

pullVoltage!(analysis::HipStateEstimation) =
    check(ccall((:jg_gn_get_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
        handle(analysis), analysis.voltage.magnitude, analysis.voltage.angle))

"""
    gaussNewton(monitoring, HIP; device = 0)

`gaussNewton(monitoring, LU)` of the reference builds the model (acWLS: type, index, range, mean, precision, Jacobian pattern);
the device gets what acWLS derived, row by row, and rebuilds pattern, gain pattern and symbolic analysis from it.
"""
function gaussNewton(monitoring::Measurement, ::Type{T}; device::Int = 0) where {T <: HipTag}
    base = gaussNewton(monitoring, LU)
    m = base.method
    method = GaussNewton{T}(m.jacobian, m.precision, m.mean, m.residual, m.increment, JuliaGrid.selectFactorization(T),
        m.type, m.index, m.range, m.signature, 0.0, 0)
    system = monitoring.system
    analysis = AcStateEstimation(base.voltage, base.power, base.current, method, system, monitoring)
    ac, br = system.model.ac, system.branch
    code, status, corr = typeCodes(monitoring)
    param = Matrix{Float64}(undef, 6, br.number)                          # [nb][6] row-major
    for k = 1:br.number
        param[:, k] .= (real(ac.admittance[k]), imag(ac.admittance[k]), br.parameter.conductance[k],
                        br.parameter.susceptance[k], br.parameter.turnsRatio[k], br.parameter.shiftAngle[k])
    end
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:jg_gn_create, lib), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
         Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Cint),
        h, system.bus.number, ac.nodalMatrix.colptr, ac.nodalMatrix.rowval, reim(ac.nodalMatrix.nzval),
        reim(ac.nodalMatrixTranspose.nzval), br.number, br.layout.from, br.layout.to, param,
        system.bus.layout.slack, length(code), code, status, m.index, length(corr), isempty(corr) ? Int64[0] : corr, 1, device))
    HANDLES[method] = Handle(h[], :gn)
    if T === HIPOrthogonal                                                # the Orthogonal / PetersWilkinson rows: corrected semi-normal equations;
        check(ccall((:jg_gn_set_method, lib), Cint, (Ptr{Cvoid}, Cint), h[], 1))   # returns 1 (-> ErrorException) on correlated PMUs, like the reference
    end
    pushMeasurement!(analysis)
    pushVoltage!(analysis)
    return analysis
end

"se.residual from the device and se.objective = r' W r (equations.jl:689-698: what chiTest reads, badData.jl:948-961)"
function pullResidual!(analysis::HipStateEstimation)
    se = analysis.method
    check(ccall((:jg_gn_get_residual, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), se.residual))
    se.objective = transpose(se.residual) * (se.precision * se.residual)
    return nothing
end

function increment!(analysis::HipStateEstimation)             # acStateEstimation.jl:878-904 (HIPOrthogonal: :906-971)
    se = analysis.method
    maxInc = Vector{Float64}(undef, 1)
    check(ccall((:jg_gn_increment, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), maxInc))   # code 3: singular gain
    check(ccall((:jg_gn_get_increment, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), se.increment))
    pullResidual!(analysis)
    se.signature[:pattern] = 0
    return maxInc[1]
end

function solve!(analysis::HipStateEstimation)                 # acStateEstimation.jl:1035-1047
    check(ccall((:jg_gn_solve, lib), Cint, (Ptr{Cvoid},), handle(analysis)))
    pullVoltage!(analysis)
    analysis.method.iteration += 1
    return nothing
end

"method.jacobian (H, m x 2n) at the current state in the reference's CSC order, on request"
function jacobian!(analysis::HipStateEstimation)
    check(ccall((:jg_gn_get_jacobian, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), analysis.method.jacobian.nzval))
    return analysis.method.jacobian
end

"""
    stateEstimation!(analysis::AcStateEstimation{GaussNewton{HIP}}; iteration, tolerance, power, current)

The reference's loop (acStateEstimation.jl:1286-1329) fused on the device; the generic `stateEstimation!` works as well.
"""
function stateEstimation!(analysis::HipStateEstimation; iteration::Int64 = 40, tolerance::Float64 = 1e-8, power::Bool = false,
                          current::Bool = false, verbose::Int64 = 0)
    se = analysis.method
    iters = Vector{Int32}(undef, 1); status = Vector{Int32}(undef, 1)
    check(ccall((:jg_gn_run, lib), Cint, (Ptr{Cvoid}, Int64, Float64, Ptr{Int32}, Ptr{Int32}),
        handle(analysis), iteration, tolerance, iters, status))
    pullVoltage!(analysis)
    check(ccall((:jg_gn_get_increment, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), se.increment))
    pullResidual!(analysis)
    se.iteration = iters[1]
    se.signature[:pattern] = 0
    status[1] == 3 && throw(ErrorException("The gain matrix is singular."))
    power && JuliaGrid.power!(analysis)
    current && JuliaGrid.current!(analysis)
    return nothing
end

"""
    chiTest(analysis::AcStateEstimation{GaussNewton{HIP}}; confidence = 0.95)

badData.jl:948-961 reads `se.objective`; here the residual (and with it the objective) is first re-evaluated on the device AT THE CURRENT STATE
(`jg_gn_evaluate`: after the last `solve!` the device holds the residual of the state before that step), then the reference's own test runs.
"""
function chiTest(analysis::HipStateEstimation; confidence::Float64 = 0.95)
    check(ccall((:jg_gn_evaluate, lib), Cint, (Ptr{Cvoid},), handle(analysis)))
    pullResidual!(analysis)
    return invoke(chiTest, Tuple{AcStateEstimation{<:GaussNewton}}, analysis; confidence)
end

"all normalised residuals of the last largestNormalizedResidual / residualTest! call (badData.jl:289-311), one per Jacobian row"
function normalizedResiduals(analysis::HipStateEstimation)
    out = Vector{Float64}(undef, length(analysis.method.mean))
    check(ccall((:jg_gn_get_normalized_residual, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), out))
    return out
end

# ---- pmuStateEstimation(monitoring, HIP) (pmuStateEstimation.jl:43-177): the LINEAR model z = H [Re V; Im V] + u.  The device runs it as one
# ---- Gauss-Newton step of linear rows (type codes 22-27, no slack) from the zero state: gain H' W H, block LU, solve (:369-399)
function pmuStateEstimation(monitoring::Measurement, ::Type{T}; device::Int = 0) where {T <: HipTag}
    base = pmuStateEstimation(monitoring, LU)                  # coefficient, precision, mean, inservice: the reference's pmuEstimationWls
    m = base.method
    method = WLS{T}(m.coefficient, m.precision, m.mean, JuliaGrid.selectFactorization(T), m.index, m.number, m.inservice, m.signature)
    system, pmu = monitoring.system, monitoring.pmu
    analysis = PmuStateEstimation(base.voltage, base.power, base.current, method, system, monitoring)
    ac, br = system.model.ac, system.branch
    code = Int8[]; status = Int8[]; index = Int64[]; corr = Int64[]
    for i = 1:pmu.number                                       # two rows (Re, Im) per device, in device order
        pmu.layout.correlated[i] && push!(corr, length(code) + 1)
        append!(code, pmu.layout.bus[i] ? (22, 23) : (pmu.layout.from[i] ? (24, 25) : (26, 27)))
        on = Int8(pmu.magnitude.status[i] * pmu.angle.status[i])
        append!(status, (on, on)); append!(index, (pmu.layout.index[i], pmu.layout.index[i]))
    end
    T === HIPOrthogonal && !isempty(corr) && throw(ErrorException("A non-diagonal precision matrix prevents the use of the select method."))
    param = Matrix{Float64}(undef, 6, br.number)
    for k = 1:br.number
        param[:, k] .= (real(ac.admittance[k]), imag(ac.admittance[k]), br.parameter.conductance[k],
                        br.parameter.susceptance[k], br.parameter.turnsRatio[k], br.parameter.shiftAngle[k])
    end
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:jg_gn_create, lib), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
         Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Cint),
        h, system.bus.number, ac.nodalMatrix.colptr, ac.nodalMatrix.rowval, reim(ac.nodalMatrix.nzval),
        reim(ac.nodalMatrixTranspose.nzval), br.number, br.layout.from, br.layout.to, param,
        0, length(code), code, status, index, length(corr), isempty(corr) ? Int64[0] : corr, 1, device))     # slack = 0: every variable is estimated
    HANDLES[method] = Handle(h[], :gn)
    T === HIPOrthogonal && check(ccall((:jg_gn_set_method, lib), Cint, (Ptr{Cvoid}, Cint), h[], 1))
    W = method.precision
    wdiag = [W[r, r] for r = 1:length(method.mean)]
    woff = Float64[W[r, r + 1] for r in corr]
    check(ccall((:jg_gn_set_measurement, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64),
        h[], method.mean, wdiag, isempty(woff) ? [0.0] : woff, 0, 0))
    return analysis
end

function solve!(analysis::HipPmuStateEstimation)              # pmuStateEstimation.jl:369-399
    n = analysis.system.bus.number
    zero = zeros(n)
    check(ccall((:jg_gn_set_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), handle(analysis), zero, zero, 0))
    maxInc = Vector{Float64}(undef, 1)
    check(ccall((:jg_gn_increment, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), handle(analysis), maxInc))    # residual = z at the zero state: H'WH, H'Wz
    check(ccall((:jg_gn_solve, lib), Cint, (Ptr{Cvoid},), handle(analysis)))
    im = Vector{Float64}(undef, n); re = Vector{Float64}(undef, n)
    check(ccall((:jg_gn_get_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), handle(analysis), im, re))   # the state arrays hold (Im V, Re V)
    resize!(analysis.voltage.magnitude, n); resize!(analysis.voltage.angle, n)
    analysis.voltage.magnitude .= hypot.(re, im)
    analysis.voltage.angle .= atan.(im, re)
    return nothing
end

function stateEstimation!(analysis::HipPmuStateEstimation; power::Bool = false, current::Bool = false, verbose::Int64 = 0)
    solve!(analysis)
    power && JuliaGrid.power!(analysis)
    current && JuliaGrid.current!(analysis)
    return nothing
end

function setInitialPoint!(analysis::HipStateEstimation)       # acStateEstimation.jl:1071-1077
    invoke(setInitialPoint!, Tuple{AcStateEstimation}, analysis)
    pushVoltage!(analysis)
end

# update<Meter>!(analysis; label, ...): the reference updates the monitoring container AND se.mean / se.precision / se.type of
# the analysis (measurement/*.jl: _update<Meter>!); the new values and masks follow to the device.  The Jacobian pattern stays.
for (fn, T) in ((:updateVoltmeter!, :AcStateEstimation), (:updateAmmeter!, :AcStateEstimation), (:updateVarmeter!, :AcStateEstimation),
                (:updateWattmeter!, :(Union{AcStateEstimation, JuliaGrid.DcStateEstimation})), (:updatePmu!, :(JuliaGrid.StateEstimation)))
    @eval function $fn(analysis::HipStateEstimation; label, kwargs...)
        invoke($fn, Tuple{$T}, analysis; label, kwargs...)
        pushStatus!(analysis)
        pushMeasurement!(analysis)
    end
end

"""
    largestNormalizedResidual(analysis) -> (value, row)

Numeric part of residualTest! (badData.jl:181-311) on the device: gain and its factor at the current state, selected inverse on
the factor pattern, normalised residuals, arg-max.  The label / status bookkeeping follows from `row` exactly as in
badData.jl:225-300.
"""
function largestNormalizedResidual(analysis::HipStateEstimation)
    mx = Vector{Float64}(undef, 1); idx = Vector{Int32}(undef, 1)
    check(ccall((:jg_gn_residual_test, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}), handle(analysis), mx, idx))
    return mx[1], Int64(idx[1])
end

# ---- sharded contingency screen: the ONE collective behind the C ABI (jgrid.h: jg_comm_*, jg_nr_allgather_results) --------------
# One Julia process per GPU.  Rank 0 draws the communicator id, the HOST ships its 128 bytes to the other ranks (MPI.bcast, a file,
# a socket -- the library does not care), every rank creates its communicator (a collective), solves its contiguous block of the
# scenario list and receives the record of the whole screen with ONE ncclAllGather of RCCL over xGMI.
const COMM_ID_BYTES = 128

"id of a new communicator (rank 0 calls this and ships the bytes to every rank)"
function commUniqueId()
    id = Vector{UInt8}(undef, COMM_ID_BYTES)
    check(ccall((:jg_comm_unique_id, lib), Cint, (Ptr{UInt8},), id))
    return id
end

mutable struct Comm
    ptr::Ptr{Cvoid}
    rank::Int
    world::Int
    device::Int
    function Comm(rank::Int, world::Int, id::Vector{UInt8}; device::Int = 0)
        length(id) == COMM_ID_BYTES || throw(DimensionMismatch("communicator id: $COMM_ID_BYTES bytes"))
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:jg_comm_create, lib), Cint, (Ptr{Ptr{Cvoid}}, Int64, Int64, Ptr{UInt8}, Cint), h, rank, world, id, device))
        c = new(h[], rank, world, device)
        finalizer(x -> (x.ptr == C_NULL || ccall((:jg_comm_destroy, lib), Cvoid, (Ptr{Cvoid},), x.ptr); x.ptr = C_NULL), c)
        return c
    end
end

"contiguous block of scenarios owned by `rank` of `world` (0-based rank; 1-based inclusive range): SURVEY 8(e)"
function shard(count::Int, rank::Int, world::Int)
    per, extra = divrem(count, world)
    lo = rank * per + min(rank, extra)
    return (lo + 1):(lo + per + (rank < extra ? 1 : 0))
end

"""
    contingencyAnalysis(system, labels, comm; iteration = 20, tolerance = 1e-8, record)

N-1 screen of `labels` (branch labels, 0 = base case) sharded over the ranks of `comm`: this rank solves `labels[shard(...)]` as one
batch on its GPU (every rank must hold the same number of scenarios: pad with 0), then ONE all-gather hands every rank the record of
the whole screen.  `record` is DEVICE memory of the caller for `world * batch` rows of `2n + 2` doubles (V | theta | iterations |
status per scenario, scenario order), e.g. an AMDGPU.jl `ROCArray{Float64}`; pass its pointer.  Replaces the reference's serial
user-level loop (src/powerSystem/branch.jl:453-459: updateBranch!(...; status = 0) -> powerFlow! -> updateBranch!(...; status = 1)).
"""
function contingencyAnalysis(system::PowerSystem, labels::Vector{Int64}, comm::Comm; iteration::Int64 = 20, tolerance::Float64 = 1e-8,
                             record::Ptr{Float64})
    mine = labels[shard(length(labels), comm.rank, comm.world)]
    b = NewtonRaphsonBatch(system, length(mine); device = comm.device)
    setOutages!(b, mine)
    check(ccall((:jg_nr_run, lib), Cint, (Ptr{Cvoid}, Int64, Float64, Ptr{Int32}, Ptr{Int32}), b.handle.ptr, iteration, tolerance, b.iteration, b.status))
    check(ccall((:jg_nr_allgather_results, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, comm.ptr, record))
    return b
end

# ---- sharded Monte-Carlo state estimation (jgrid.h: jg_gn_pack_results_device, jg_gn_allgather_results) ---------------------------------
"""
    GaussNewtonBatch(monitoring, batch; device = 0)

`batch` noisy realisations of ONE measurement set (the reference draws a realisation inside `add<Meter>!(...; noise = true)`,
src/measurement/utility.jl:70-73, and estimates them one after the other, acStateEstimation.jl:1286-1329): same rows, type codes and Jacobian
pattern, per-realisation means and precisions.  Results are [n, batch] matrices / [batch] vectors.
"""
mutable struct GaussNewtonBatch
    monitoring::Measurement
    batch::Int
    handle::Handle
    rows::Int
    magnitude::Matrix{Float64}
    angle::Matrix{Float64}
    iteration::Vector{Int32}
    status::Vector{Int32}                          # 0 converged, 1 iteration limit, 3 singular gain matrix
    objective::Vector{Float64}                     # se.objective = r' W r per realisation (equations.jl:689-698)
    pairs::Int                                     # correlated rectangular PMUs: rows of `woff` in setRealisations!
end

function GaussNewtonBatch(monitoring::Measurement, batch::Int; device::Int = 0)
    base = gaussNewton(monitoring, LU)
    m = base.method
    system = monitoring.system
    ac, br = system.model.ac, system.branch
    code, status, corr = typeCodes(monitoring)
    param = Matrix{Float64}(undef, 6, br.number)
    for k = 1:br.number
        param[:, k] .= (real(ac.admittance[k]), imag(ac.admittance[k]), br.parameter.conductance[k],
                        br.parameter.susceptance[k], br.parameter.turnsRatio[k], br.parameter.shiftAngle[k])
    end
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:jg_gn_create, lib), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
         Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Cint),
        h, system.bus.number, ac.nodalMatrix.colptr, ac.nodalMatrix.rowval, reim(ac.nodalMatrix.nzval),
        reim(ac.nodalMatrixTranspose.nzval), br.number, br.layout.from, br.layout.to, param,
        system.bus.layout.slack, length(code), code, status, m.index, length(corr), isempty(corr) ? Int64[0] : corr, batch, device))
    b = GaussNewtonBatch(monitoring, batch, Handle(h[], :gn), length(code), zeros(system.bus.number, batch), zeros(system.bus.number, batch),
        zeros(Int32, batch), zeros(Int32, batch), zeros(batch), length(corr))
    W = m.precision
    wdiag = [W[r, r] for r = 1:length(m.mean)]
    woff = Float64[W[r, r + 1] for r in corr]
    check(ccall((:jg_gn_set_measurement, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64),
        b.handle.ptr, m.mean, wdiag, isempty(woff) ? [0.0] : woff, 0, 0))
    check(ccall((:jg_gn_set_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), b.handle.ptr,
        base.voltage.magnitude, base.voltage.angle, 0))
    return b
end

"se.mean and the diagonal (+ pair terms `woff` [pairs, batch]) of se.precision per realisation: [rows, batch] each (acStateEstimation.jl:135-236)"
function setRealisations!(b::GaussNewtonBatch, mean::Matrix{Float64}, wdiag::Matrix{Float64}, woff::Matrix{Float64} = zeros(max(b.pairs, 1), b.batch))
    size(mean) == (b.rows, b.batch) && size(wdiag) == (b.rows, b.batch) || throw(DimensionMismatch("[rows, batch] means and precisions"))
    # (ADVICE r05) the pair terms of correlated rectangular PMUs travel per realisation: a short `woff` would be read past its end, a default of zeros would silently
    # drop the cross terms of the precision matrix
    b.pairs == 0 || size(woff) == (b.pairs, b.batch) || throw(DimensionMismatch("[correlated pairs, batch] off-diagonal precision terms: $(b.pairs) pair(s) in this model"))
    check(ccall((:jg_gn_set_measurement, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64),
        b.handle.ptr, mean, wdiag, woff, b.rows, size(woff, 1)))
end

"""
    setReadings!(b, row, kind, z1, v1, s1, z2, v2, s2);  drawNoise!(b, seed; scale = 1.0, first = 0)

Realisations drawn ON the device (jg_gn_set_readings / jg_gn_draw_noise): the raw readings per device once (first row 1-based, kind of acWLS value rule 0..5 --
include/jgrid.h --, mean / variance / status of the magnitude-type and of the angle-type quantity), then lane b of the batch becomes realisation `first + b` of `seed`:
what `add<Meter>!(...; noise = true)` draws (measurement/utility.jl:70-73) and acWLS makes of it (acStateEstimation.jl:135-236), without a byte over PCIe.
"""
setReadings!(b::GaussNewtonBatch, row::Vector{Int64}, kind::Vector{Int8}, z1::Vector{Float64}, v1::Vector{Float64}, s1::Vector{Int8},
             z2::Vector{Float64}, v2::Vector{Float64}, s2::Vector{Int8}) =
    check(ccall((:jg_gn_set_readings, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int8}, Ptr{Float64}, Ptr{Float64}, Ptr{Int8}, Ptr{Float64}, Ptr{Float64}, Ptr{Int8}),
        b.handle.ptr, length(row), row, kind, z1, v1, s1, z2, v2, s2))
drawNoise!(b::GaussNewtonBatch, seed::UInt64; scale::Float64 = 1.0, first::Int64 = 0) =
    check(ccall((:jg_gn_draw_noise, lib), Cint, (Ptr{Cvoid}, UInt64, Float64, Int64), b.handle.ptr, seed, scale, first))
"se.mean and diag(se.precision) of every realisation as the device holds them: [rows, batch] each (+ the pair terms [pairs, batch])"
function measurementDevice(b::GaussNewtonBatch, pairs::Int = 0)
    mean = Matrix{Float64}(undef, b.rows, b.batch); wdiag = similar(mean); woff = Matrix{Float64}(undef, max(pairs, 1), b.batch)
    check(ccall((:jg_gn_get_measurement, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.handle.ptr, mean, wdiag, woff))
    return mean, wdiag, woff
end

"stateEstimation!(analysis; iteration, tolerance) for every realisation of the batch (acStateEstimation.jl:1286-1329), then voltages and objectives"
function stateEstimation!(b::GaussNewtonBatch; iteration::Int64 = 40, tolerance::Float64 = 1e-8, fetch::Bool = true)
    check(ccall((:jg_gn_run, lib), Cint, (Ptr{Cvoid}, Int64, Float64, Ptr{Int32}, Ptr{Int32}), b.handle.ptr, iteration, tolerance, b.iteration, b.status))
    if fetch
        check(ccall((:jg_gn_get_voltage, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), b.handle.ptr, b.magnitude, b.angle))
        check(ccall((:jg_gn_get_objective, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, b.objective))
    end
    return nothing
end

"the batch's result record (magnitude | angle | iterations | status | objective per realisation, [2n + 3, batch]) into a DEVICE buffer of the caller"
packResults!(b::GaussNewtonBatch, record::Ptr{Float64}) =
    check(ccall((:jg_gn_pack_results_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, record))

"""
    monteCarloEstimation(monitoring, mean, wdiag, comm; iteration = 40, tolerance = 1e-8, record)

Noisy realisations (columns of `mean` / `wdiag`, [rows, realisations]) sharded over the ranks of `comm`: this rank estimates its contiguous block as one batch
(every rank the same count), then ONE all-gather hands every rank the record of all realisations: `record` = DEVICE memory for `world * batch` rows
of `2n + 3` doubles (magnitude | angle | iterations | status | objective).
"""
function monteCarloEstimation(monitoring::Measurement, mean::Matrix{Float64}, wdiag::Matrix{Float64}, comm::Comm; iteration::Int64 = 40,
                              tolerance::Float64 = 1e-8, record::Ptr{Float64})
    mine = shard(size(mean, 2), comm.rank, comm.world)
    b = GaussNewtonBatch(monitoring, length(mine); device = comm.device)
    setRealisations!(b, mean[:, mine], wdiag[:, mine])
    stateEstimation!(b; iteration, tolerance, fetch = false)
    check(ccall((:jg_gn_allgather_results, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, comm.ptr, record))
    return b
end

"drops the library's cached symbolic analyses (live analyses keep theirs): the next newtonRaphson(system, HIP) pays a full analysis again"
clearPlanCache() = ccall((:jg_plan_cache_clear, lib), Cvoid, ())

# ---- the rest of the ABI: sizes, maps, device-resident start points and records, the optional guard (include/jgrid.h) -------------------------
"number of HIP devices the library sees"
deviceCount() = Int(ccall((:jg_device_count, lib), Cint, ()))

"(dimJ, nnz(J), blocks of L + D + U, update terms, launches per factorisation, launches per backward sweep)"
function dims(analysis::HipAnyPowerFlow)
    d = Vector{Int64}(undef, 6)
    check(ccall((:jg_nr_dims, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), handle(analysis), d))
    return d
end
"(m, nnz(H), gain blocks, blocks of L + D + U, update terms, factor launches, backward launches, H slots)"
function dims(analysis::Union{HipStateEstimation, HipPmuStateEstimation})
    d = Vector{Int64}(undef, 8)
    check(ccall((:jg_gn_dims, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), handle(analysis), d))
    return d
end

"one step of iterative refinement behind every Newton step (what UMFPACK's solve does behind ldiv!, utility.jl:576-586); off by default"
setRefinement!(analysis::HipPowerFlow, on::Bool = true) =
    check(ccall((:jg_nr_set_refine, lib), Cint, (Ptr{Cvoid}, Cint), handle(analysis), on ? 1 : 0))

"pq, pvpq, pcount and the CSC pattern of the Jacobian as the DEVICE built them (bit-exact copies of newtonJacobian's, acPowerFlow.jl:89-175)"
function deviceMaps(analysis::HipPowerFlow)
    n, d = analysis.system.bus.number, dims(analysis)
    pq = Vector{Int64}(undef, n); pvpq = Vector{Int64}(undef, n); pcount = Vector{Int64}(undef, n)
    colptr = Vector{Int64}(undef, d[1] + 1); rowval = Vector{Int64}(undef, d[2])
    check(ccall((:jg_nr_get_maps, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        handle(analysis), pq, pvpq, pcount, colptr, rowval))
    return pq, pvpq, pcount, colptr, rowval
end
"se.type and the CSC pattern of H as the device built them (bit-exact copies of acWLS's, acStateEstimation.jl:77-259)"
function deviceMaps(analysis::HipStateEstimation)
    d = dims(analysis)
    type = Vector{Int8}(undef, d[1]); colptr = Vector{Int64}(undef, 2 * analysis.system.bus.number + 1); rowval = Vector{Int64}(undef, d[2])
    check(ccall((:jg_gn_get_maps, lib), Cint, (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int64}, Ptr{Int64}), handle(analysis), type, colptr, rowval))
    return type, colptr, rowval
end

"scenario s (1-based) of a batch: branch `label` out of service (0: back to the base grid) -- the four edits acNodalUpdate! makes, model.jl:93-101"
function setOutage!(b::NewtonRaphsonBatch, s::Int, label::Int64)
    ac, Y, lay = b.system.model.ac, b.system.model.ac.nodalMatrix, b.system.branch.layout
    position(r, c) = Y.colptr[c] + searchsortedfirst(view(Y.rowval, Y.colptr[c]:(Y.colptr[c + 1] - 1)), r) - 1
    ptr = zeros(Int64, 4); dy = zeros(Float64, 2, 4)
    if label != 0
        i, j = lay.from[label], lay.to[label]
        ptr .= (position(i, i), position(j, j), position(i, j), position(j, i))
        for (m, v) in enumerate((ac.nodalFromFrom[label], ac.nodalToTo[label], ac.nodalFromTo[label], ac.nodalToFrom[label]))
            dy[1, m], dy[2, m] = -real(v), -imag(v)
        end
    end
    check(ccall((:jg_nr_patch_ybus, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}), b.handle.ptr, s - 1, label == 0 ? 0 : 4, ptr, dy))
    b.outage[s] = label
    return nothing
end

"""
    fastPatch!(batch, scenario0, ptr, dbp, dbq)

Fast Newton-Raphson under batched outages (jg_nr_fast_patch_batch): scenarios `scenario0 + 1 : scenario0 + size(ptr, 2)` keep the shared B', B'' of
`jg_nr_fast_setup` plus the edits `dbp`, `dbq` ([k, count], k <= 4) at the stored Ybus pointers `ptr` ([k, count], 1-based, 0 = unused); the batch is
factorised once.  What `_updateBranch!(::AcPowerFlow{<:FastNewtonRaphson})` (branch.jl:477) does entry by entry for one scenario at a time.
"""
fastPatch!(b::NewtonRaphsonBatch, scenario0::Int, ptr::Matrix{Int64}, dbp::Matrix{Float64}, dbq::Matrix{Float64}) =
    check(ccall((:jg_nr_fast_patch_batch, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
        b.handle.ptr, scenario0, size(ptr, 2), size(ptr, 1), ptr, dbp, dbq))

"keeps the current voltages of every scenario inside HBM / brings them back (the start point of a Monte-Carlo or benchmark loop without a PCIe round trip)"
snapshotVoltage!(b::NewtonRaphsonBatch) = check(ccall((:jg_nr_snapshot_voltage, lib), Cint, (Ptr{Cvoid},), b.handle.ptr))
restoreVoltage!(b::NewtonRaphsonBatch) = check(ccall((:jg_nr_restore_voltage, lib), Cint, (Ptr{Cvoid},), b.handle.ptr))
snapshotVoltage!(analysis::HipStateEstimation) = check(ccall((:jg_gn_snapshot_voltage, lib), Cint, (Ptr{Cvoid},), handle(analysis)))
restoreVoltage!(analysis::HipStateEstimation) = check(ccall((:jg_gn_restore_voltage, lib), Cint, (Ptr{Cvoid},), handle(analysis)))

"method.iteration of every scenario, straight from the device"
function iterations(b::NewtonRaphsonBatch)
    check(ccall((:jg_nr_get_iteration, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}), b.handle.ptr, b.iteration))
    return b.iteration
end
function iterations(analysis::HipStateEstimation)
    it = Vector{Int32}(undef, 1)
    check(ccall((:jg_gn_get_iteration, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}), handle(analysis), it))
    return Int(it[1])
end

"""
    setBusType!(b, scenario0, type)
    busType(b)

Bus types per scenario (jg_nr_set_bus_type / jg_nr_get_bus_type): scenarios `scenario0 + 1 : scenario0 + size(type, 2)` take the columns of
`type` ([n, count] Int8: 1 PQ, 2 PV, 3 slack, one slack each); `setBusType!(b, scenario0, count)` returns them to the types the batch was built
with.  `busType` gives the types [n, batch] and the slack bus of every scenario.
"""
setBusType!(b::NewtonRaphsonBatch, scenario0::Int, type::Matrix{Int8}) =
    check(ccall((:jg_nr_set_bus_type, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Int8}), b.handle.ptr, scenario0, size(type, 2), type))
setBusType!(b::NewtonRaphsonBatch, scenario0::Int, count::Int) =
    check(ccall((:jg_nr_set_bus_type, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Int8}), b.handle.ptr, scenario0, count, C_NULL))
function busType(b::NewtonRaphsonBatch)
    type = Matrix{Int8}(undef, b.system.bus.number, b.batch)
    slack = Vector{Int64}(undef, b.batch)
    check(ccall((:jg_nr_get_bus_type, lib), Cint, (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int64}), b.handle.ptr, type, slack))
    return type, slack
end

"""
    reactiveLimit!(b; restart = true)

reactiveLimit! (acPowerFlow.jl:1081-1155) for every scenario of the batch on the device (jg_nr_set_generators once, then jg_nr_reactive_limit): the
scenarios with a violation take their new bus types and injections and, `restart`, start again from the system's initial point.  Returns the
violate matrix [ng, batch] (Int8); a scenario left without a slack reports status 5 from the next powerFlow! on.  `system` is not modified.
"""
const QLIM_TABLES = WeakKeyDict{NewtonRaphsonBatch, Any}()   # what jg_nr_set_generators last received per batch (sent again only when it changed)

function reactiveLimit!(b::NewtonRaphsonBatch; restart::Bool = true)
    system = b.system
    gen, bus = system.generator, system.bus
    key = (copy(gen.layout.bus), copy(gen.layout.status), copy(gen.output.active), copy(gen.capability.minReactive), copy(gen.capability.maxReactive),
           copy(gen.voltage.magnitude), copy(bus.voltage.magnitude), copy(bus.voltage.angle), copy(bus.demand.active), copy(bus.demand.reactive))
    get(QLIM_TABLES, b, nothing) == key || (QLIM_TABLES[b] = key; check(ccall((:jg_nr_set_generators, lib), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int8}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64),
        b.handle.ptr, gen.number, Vector{Int64}(gen.layout.bus), Vector{Int8}(gen.layout.status), gen.output.active, gen.capability.minReactive,
        gen.capability.maxReactive, gen.voltage.magnitude, bus.voltage.magnitude, bus.voltage.angle, bus.demand.active, bus.demand.reactive,
        system.base.power.value * system.base.power.prefix * 1e-6)))
    violate = Matrix{Int8}(undef, gen.number, b.batch)
    count = Vector{Int32}(undef, b.batch)
    check(ccall((:jg_nr_reactive_limit, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Int8}, Ptr{Int32}), b.handle.ptr, restart ? 1 : 0, violate, count))
    return violate
end

"adjustAngle! (acPowerFlow.jl:1196-1206) of every scenario on the device state: the angle of bus `slack` becomes the system's (jg_nr_adjust_angle)"
adjustAngle!(b::NewtonRaphsonBatch; slack::Int) =
    check(ccall((:jg_nr_adjust_angle, lib), Cint, (Ptr{Cvoid}, Int64, Float64), b.handle.ptr, slack, b.system.bus.voltage.angle[slack]))

"V and theta of every scenario into DEVICE buffers of the caller ([n, batch] each, e.g. AMDGPU.jl arrays: pass their pointers)"
voltageDevice!(b::NewtonRaphsonBatch, magnitude::Ptr{Float64}, angle::Ptr{Float64}) =
    check(ccall((:jg_nr_get_voltage_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), b.handle.ptr, magnitude, angle))
"the result record of the batch (V | theta | iterations | status per scenario, [2n + 2, batch]) into a DEVICE buffer of the caller: the operand of the one gather"
packResults!(b::NewtonRaphsonBatch, record::Ptr{Float64}) =
    check(ccall((:jg_nr_pack_results_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.handle.ptr, record))
"rows `rows` (0-based) of a record another batch owns <- lanes lane0 + 1 : lane0 + length(rows) of this pool (jg_nr_pack_rows_device)"
packRows!(pool::NewtonRaphsonBatch, record::Ptr{Float64}, lane0::Int, rows::Vector{Int32}) =
    check(ccall((:jg_nr_pack_rows_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Int32}), pool.handle.ptr, record, lane0, length(rows), rows))
"rows `rows` (0-based) of a screen-summary record ([10, .] doubles, screenSummary) another batch owns <- the summaries of lanes lane0 + 1 : lane0 + length(rows)
of this pool (jg_nr_screen_rows_device); the pool's branch table, ratings and outage labels must be set (screenSummary / setOutage! on the pool)"
screenRows!(pool::NewtonRaphsonBatch, record::Ptr{Float64}, lane0::Int, rows::Vector{Int32}) =
    check(ccall((:jg_nr_screen_rows_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Int32}), pool.handle.ptr, record, lane0, length(rows), rows))

"the collective for a record that is already packed: `count` doubles per rank from device pointer `send` into `recv` [count, world]"
allgatherDevice(comm::Comm, send::Ptr{Float64}, recv::Ptr{Float64}, count::Int) =
    check(ccall((:jg_comm_allgather_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), comm.ptr, send, recv, count))
commRank(comm::Comm) = Int(ccall((:jg_comm_rank, lib), Cint, (Ptr{Cvoid},), comm.ptr))
commWorld(comm::Comm) = Int(ccall((:jg_comm_world, lib), Cint, (Ptr{Cvoid},), comm.ptr))

"mean milliseconds of `reps` executions of one kernel group on the handle's stream (HIP events): 0 assembly, 1 factorisation, 2 backward sweep, 3 branch post-processing"
function timeKernel(analysis::HipAnyPowerFlow, kernel::Int, reps::Int = 10)
    ms = Ref(0.0)
    check(ccall((:jg_nr_time_kernel, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Float64}), handle(analysis), kernel, reps, ms))
    return ms[]
end
"... of a state estimation: 0 measurement rows, 1 gain + rhs gather, 2 factorisation, 3 backward sweep, 4 selected inverse"
function timeKernel(analysis::HipStateEstimation, kernel::Int, reps::Int = 10)
    ms = Ref(0.0)
    check(ccall((:jg_gn_time_kernel, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Float64}), handle(analysis), kernel, reps, ms))
    return ms[]
end

# ---- DC power flow and the batched DC N-1 screen (jgrid.h: jg_dc_*; csrc/jg_dc.hip) ------------------------------------------------------
# dcPowerFlow / solve! / power!(::DcPowerFlow) (src/powerFlow/dcPowerFlow.jl:42-134, src/postprocessing/dcAnalysis.jl:27-75) for `batch` scenarios of one
# grid on ONE factor of the base nodal matrix: an outage of a scenario (updateBranch!(analysis; label, status = 0)) is a rank-1 correction on that
# factor, never a refactorisation.  The C handle is an Int64 token.
"""
    DcPowerFlowBatch(system; batch = 1, device = 0)

Factorises system.model.dc.nodalMatrix (slack row and column removed, dcPowerFlow.jl:63-80) once on the device and uploads the branch table.
`solve!(b)` then gives `b.angle` [bus, batch] and `b.status` (0, or 3 where the outaged branch is a bridge: its angles are NaN).
"""
mutable struct DcPowerFlowBatch
    token::Int64
    system::PowerSystem
    batch::Int64
    angle::Matrix{Float64}
    status::Vector{Int32}
    rhs::Vector{Float64}                              # the base right-hand side the library holds (empty: none yet)
    injections::Vector{Tuple{Int64, Matrix{Float64}}}   # (lane0, [bus, count] right-hand sides) in the order they were set: a later one wins where lanes overlap
end
function DcPowerFlowBatch(system::PowerSystem; batch::Int64 = 1, device::Int64 = 0)
    if isempty(system.model.dc.nodalMatrix)
        dcModel!(system)
    end
    B = system.model.dc.nodalMatrix
    slack = system.bus.layout.slack
    token = Ref{Int64}(0)
    check(ccall((:jg_dc_create, lib), Cint, (Ref{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Float64, Int64, Cint),
        token, system.bus.number, B.colptr, B.rowval, B.nzval, slack, system.bus.voltage.angle[slack], batch, device))
    b = DcPowerFlowBatch(token[], system, batch, zeros(system.bus.number, batch), zeros(Int32, batch), Float64[], Tuple{Int64, Matrix{Float64}}[])
    finalizer(x -> (x.token != 0 && ccall((:jg_dc_destroy, lib), Cvoid, (Int64,), x.token); x.token = 0), b)
    br = system.branch
    check(ccall((:jg_dc_set_branches, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
        b.token, br.number, br.layout.from, br.layout.to, system.model.dc.admittance, br.parameter.shiftAngle))
    return b
end
"{n, batch, ld, branches, factor entries, factorisation levels, forward levels, backward levels, launches of a sweep pair, padded sweep terms}"
function dims(b::DcPowerFlowBatch)
    d = zeros(Int64, 10)
    check(ccall((:jg_dc_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, d))
    return d
end
"scenario `lane0 + s` (0-based lanes) loses branch `branches[s]` (index, 0 = no outage)"
setOutages!(b::DcPowerFlowBatch, branches::Vector{Int64}; lane0::Int64 = 0) =
    check(ccall((:jg_dc_set_outages, lib), Cint, (Int64, Int64, Int64, Ptr{Int64}), b.token, lane0, length(branches), branches))
baseRhs(b::DcPowerFlowBatch) = b.system.bus.supply.active .- b.system.bus.demand.active .- b.system.bus.shunt.conductance .- b.system.model.dc.shiftPower
# jg_dc_set_rhs drops the per-scenario injections the library holds (jgrid.h), so the base right-hand side goes up only when it CHANGED and the
# injections kept in b.injections follow it again (what dcpowerflow.py: solve_ / _upload_injections do)
function uploadRhs!(b::DcPowerFlowBatch)
    rhs = baseRhs(b)
    if rhs != b.rhs
        check(ccall((:jg_dc_set_rhs, lib), Cint, (Int64, Ptr{Float64}), b.token, rhs))
        b.rhs = rhs
        for (lane0, own) in b.injections
            check(ccall((:jg_dc_set_injections, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, lane0, size(own, 2), own))
        end
    end
    return nothing
end
"""
    setInjections!(b, rhs; lane0 = 0)

Lanes lane0 .. lane0 + size(rhs, 2) - 1 (0-based) get right-hand sides of their own: a [bus, count] matrix of supply - demand - shunt conductance -
shiftPower per scenario.  They hold for every later `solve!` of the batch, also after the system's own right-hand side changed.
"""
function setInjections!(b::DcPowerFlowBatch, rhs::Matrix{Float64}; lane0::Int64 = 0)
    push!(b.injections, (lane0, copy(rhs)))
    uploadRhs!(b)                                     # the base first (the library asks for it), with every kept injection if it changed
    check(ccall((:jg_dc_set_injections, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, lane0, size(rhs, 2), rhs))
    return nothing
end
"solve!(analysis) for every scenario (dcPowerFlow.jl:63-101)"
function JuliaGrid.solve!(b::DcPowerFlowBatch)
    uploadRhs!(b)
    check(ccall((:jg_dc_solve, lib), Cint, (Int64,), b.token))
    check(ccall((:jg_dc_get_angle, lib), Cint, (Int64, Ptr{Float64}, Ptr{Int32}), b.token, b.angle, b.status))
    return nothing
end
"active power at the from-bus end of every branch, [branch, batch] (dcAnalysis.jl:41-48); to = -from; 0 on a lane's outaged branch"
function fromPower(b::DcPowerFlowBatch)
    from = Matrix{Float64}(undef, b.system.branch.number, b.batch)
    check(ccall((:jg_dc_get_flows, lib), Cint, (Int64, Ptr{Float64}), b.token, from))
    return from
end
"""
    screenSummary(b::DcPowerFlowBatch; rating = nothing, record = nothing) -> Matrix [5, batch]

Per scenario: worst |from| / rating and its branch (0: none rated), largest |from| and its branch, status.  `record`: a DEVICE pointer for
`5 * batch` doubles instead (the operand of `allgatherDevice`).
"""
function screenSummary(b::DcPowerFlowBatch; rating::Union{Nothing, Vector{Float64}} = nothing, record::Union{Nothing, Ptr{Float64}} = nothing)
    if rating === nothing
        check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, C_NULL))
    else
        check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    end
    if record !== nothing
        check(ccall((:jg_dc_screen_device, lib), Cint, (Int64, Ptr{Float64}), b.token, record))
        return nothing
    end
    rec = Matrix{Float64}(undef, 5, b.batch)
    check(ccall((:jg_dc_screen, lib), Cint, (Int64, Ptr{Float64}), b.token, rec))
    return rec
end
"angle | status per scenario, `(bus + 1) * batch` doubles, into DEVICE memory of the caller (the operand of `allgatherDevice`)"
packResults!(b::DcPowerFlowBatch, dst::Ptr{Float64}) = check(ccall((:jg_dc_pack_results_device, lib), Cint, (Int64, Ptr{Float64}), b.token, dst))
"(device address of the batch-minor angles, their leading dimension, device address of the Int32 status)"
function angleDevice(b::DcPowerFlowBatch)
    info = zeros(Int64, 3)
    check(ccall((:jg_dc_angle_device, lib), Cint, (Int64, Ptr{Int64}), b.token, info))
    return info
end
"milliseconds of `reps` runs (HIP events): 0 the whole chain of a batch, 1 the sweep pair, 2 the combine, 3 flows + summary"
function timeKernel(b::DcPowerFlowBatch, kernel::Int, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dc_time_kernel, lib), Cint, (Int64, Cint, Cint, Ptr{Float64}), b.token, kernel, reps, ms))
    return ms
end
"scenario `lane0 + s` (0-based lanes) loses branches `first[s]` AND `second[s]` (indices; `second[s] = 0`: a single outage)"
setOutagePairs!(b::DcPowerFlowBatch, first::Vector{Int64}, second::Vector{Int64}; lane0::Int64 = 0) =
    check(ccall((:jg_dc_set_outage_pairs, lib), Cint, (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}), b.token, lane0, length(first), first, second))
"""
    setIslandMode!(b, mode)

`mode = 1`: lanes set AFTERWARDS by `setOutages!` whose branch is a bridge are solved on the side of the bridge that holds the slack (status 4, NaN angles on
the buses that leave, flows 0 on the branches that touch them) instead of being skipped with status 3; `mode = 0` is the default (jgrid.h: jg_dc_set_island_mode).
"""
setIslandMode!(b::DcPowerFlowBatch, mode::Integer) = check(ccall((:jg_dc_set_island_mode, lib), Cint, (Int64, Cint), b.token, mode))
"what the lanes of a solved batch shed, `[4, batch]`: buses, the right-hand side summed over them, the bridge's end `m` on the slack's side, the flow that left `m`"
function islands(b::DcPowerFlowBatch)
    rec = zeros(Float64, 4, dims(b)[2])
    check(ccall((:jg_dc_get_islands, lib), Cint, (Int64, Ptr{Float64}), b.token, rec))
    return rec
end
"host only: `(preorder, lo, hi, side)` -- the buses that leave with branch `k` are those with `lo[k] <= preorder <= hi[k]` (`lo > hi`: no bridge; jgrid.h: jg_dc_island_table)"
function islandTable(system::PowerSystem)
    br = system.branch
    pre = zeros(Int32, system.bus.number)
    lo = zeros(Int32, br.number); hi = zeros(Int32, br.number); side = zeros(Int32, br.number)
    check(ccall((:jg_dc_island_table, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                system.bus.number, br.number, br.layout.from, br.layout.to, Float64.(br.layout.status .== 1), system.bus.layout.slack, pre, lo, hi, side))
    return pre, lo, hi, side
end
"""
    pairScreenBuild!(b, candidates; monitored = nothing, budget = 0) -> info [8]

The DC N-2 screen (jgrid.h: jg_dc_pair_*): one sweep pair per candidate branch (indices, in service, ascending) fills the outage sensitivities of the
monitored branches (default: every branch in service).  `budget`: bytes they may take (0: 0.8 of the free device memory); an error names the sizes.
"""
function pairScreenBuild!(b::DcPowerFlowBatch, candidates::Vector{Int64}; monitored::Union{Nothing, Vector{Int64}} = nothing, budget::Int64 = 0)
    uploadRhs!(b)
    info = zeros(Float64, 8)
    if monitored === nothing
        check(ccall((:jg_dc_pair_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}),
            b.token, length(candidates), candidates, 0, C_NULL, budget, info))
    else
        check(ccall((:jg_dc_pair_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}),
            b.token, length(candidates), candidates, length(monitored), monitored, budget, info))
    end
    return info
end
"""
    pairScreen(b, k0, k1, candidates; rating, threshold = 1.0, capacity = 2^20, islandCapacity = 2^16) -> (records [5, m], islanding [2, i], totals [6], worst)

All pairs (k, l > k) whose first branch is candidate position k0 .. k1 - 1 (0-based): the records of the pairs above `threshold` sorted by (k, l) (branch k,
branch l, worst branch, worst |from| / rating, overloaded branches), the islanding pairs, the totals (pairs, violating, islanding, records kept, islanding
pairs kept, overflow flags) and the worst loading per candidate.
"""
function pairScreen(b::DcPowerFlowBatch, k0::Int64, k1::Int64, candidates::Vector{Int64}; rating::Vector{Float64}, threshold::Float64 = 1.0,
                    capacity::Int64 = 2^20, islandCapacity::Int64 = 2^16)
    check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    records = Matrix{Float64}(undef, 5, capacity)
    islanding = Matrix{Int64}(undef, 2, islandCapacity)
    totals = zeros(Int64, 6)
    worst = zeros(Float64, length(candidates))
    check(ccall((:jg_dc_pair_screen, lib), Cint, (Int64, Int64, Int64, Float64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
                                                  Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
        b.token, k0, k1, threshold, capacity, records, islandCapacity, islanding, totals, worst, C_NULL, C_NULL, C_NULL, C_NULL))
    return records[:, 1:totals[4]], islanding[:, 1:totals[5]], totals, worst
end
"milliseconds of `reps` runs on candidate rows k0 .. k1 - 1 (HIP events): 0 the pair screen kernel, 1 its row / column summaries"
function pairTimeKernel(b::DcPowerFlowBatch, kernel::Int, k0::Int64, k1::Int64, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dc_pair_time_kernel, lib), Cint, (Int64, Cint, Int64, Int64, Cint, Ptr{Float64}), b.token, kernel, k0, k1, reps, ms))
    return ms
end
"frees the sensitivities a pair screen keeps on the device"
pairScreenRelease!(b::DcPowerFlowBatch) = check(ccall((:jg_dc_pair_release, lib), Cint, (Int64,), b.token))
"""
    groupScreenBuild!(b, groups; monitored = nothing, budget = 0) -> info [8]

The DC common-mode screen (jgrid.h: jg_dc_group_*): `groups` is a vector of vectors of 1 to 8 branch indices (in service, none twice within a group), each
group one case.  The candidates of the kept outage sensitivities are the sorted union of all members; `monitored` and `budget` as `pairScreenBuild!`.
"""
function groupScreenBuild!(b::DcPowerFlowBatch, groups::Vector{Vector{Int64}}; monitored::Union{Nothing, Vector{Int64}} = nothing, budget::Int64 = 0)
    uploadRhs!(b)
    info = zeros(Float64, 8)
    offsets = Int64[0; cumsum(length.(groups))]
    members = reduce(vcat, groups; init = Int64[])
    if monitored === nothing
        check(ccall((:jg_dc_group_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}),
            b.token, length(groups), offsets, members, 0, C_NULL, budget, info))
    else
        check(ccall((:jg_dc_group_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}),
            b.token, length(groups), offsets, members, length(monitored), monitored, budget, info))
    end
    return info
end
"dims [6] of the group screen built last: groups, their leading dimension, candidates, rows of Phi, monitored branches, members of the largest group"
function groupScreenDims(b::DcPowerFlowBatch)
    dims = zeros(Int64, 6)
    check(ccall((:jg_dc_group_get_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, dims))
    return dims
end
"the candidates of the group screen built last: the union of the members, ascending"
function groupScreenCandidates(b::DcPowerFlowBatch)
    labels = zeros(Int64, groupScreenDims(b)[3])
    check(ccall((:jg_dc_group_get_candidates, lib), Cint, (Int64, Ptr{Int64}), b.token, labels))
    return labels
end
"the base-case flows of the monitored branches of the group screen built last, ascending by branch"
function groupScreenBase(b::DcPowerFlowBatch)
    flow = zeros(Float64, groupScreenDims(b)[5])
    check(ccall((:jg_dc_group_get_base, lib), Cint, (Int64, Ptr{Float64}), b.token, flow))
    return flow
end
"""
    groupScreen(b, g0, g1; rating, threshold = 1.0, capacity = 2^20, dense = false) -> (status, worst, worstBranch, count, records [4, m], islanding, totals [6], flows, ms)

The groups g0 .. g1 - 1 (0-based): per group the status (3: it islands a part of the grid), the worst |from| / rating over the monitored branches that stay,
its branch and the number of branches above `threshold`; the violating branches sorted by (group, branch) (group, branch, flow, loading); the islanding
groups; the totals; with `dense` the flows [monitored, g1 - g0] (0 on the members, NaN for status 3); the milliseconds of the solves and the screen kernel.
"""
function groupScreen(b::DcPowerFlowBatch, g0::Int64, g1::Int64; rating::Vector{Float64}, threshold::Float64 = 1.0, capacity::Int64 = 2^20, dense::Bool = false)
    check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    rb = g1 - g0
    records = Matrix{Float64}(undef, 4, capacity)
    islanding = zeros(Int64, rb)
    totals = zeros(Int64, 6)
    status = zeros(Int32, rb); worst = zeros(Float64, rb); branch = zeros(Int32, rb); count = zeros(Int32, rb)
    flows = dense ? zeros(Float64, groupScreenDims(b)[5], rb) : zeros(Float64, 0, 0)
    ms = zeros(Float64, 1)
    check(ccall((:jg_dc_group_screen, lib), Cint, (Int64, Int64, Int64, Float64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
                                                   Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
        b.token, g0, g1, threshold, capacity, records, rb, islanding, totals, status, worst, branch, count, dense ? pointer(flows) : Ptr{Float64}(C_NULL), ms))
    return status, worst, branch, count, records[:, 1:totals[4]], islanding[1:totals[5]], totals, flows, ms[1]
end
"milliseconds of `reps` runs on the groups g0 .. g1 - 1 (HIP events): 0 the group screen kernel, 1 the k x k solves"
function groupTimeKernel(b::DcPowerFlowBatch, kernel::Int, g0::Int64, g1::Int64, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dc_group_time_kernel, lib), Cint, (Int64, Cint, Int64, Int64, Cint, Ptr{Float64}), b.token, kernel, g0, g1, reps, ms))
    return ms
end
"frees what a group screen keeps on the device"
groupScreenRelease!(b::DcPowerFlowBatch) = check(ccall((:jg_dc_group_release, lib), Cint, (Int64,), b.token))
"""
    cascadeScreenBuild!(b, events; monitored = nothing, budget = 0) -> info [8]

The DC cascading-outage screen (jgrid.h: jg_dc_cascade_*): `events` is a vector of vectors of 1 to 8 branch indices (in service, none twice within an
event), each the initiating outage of one cascade.  `monitored` are the branches that can trip and that are reported (nothing: every branch in service).
The candidates of the kept outage sensitivities are the sorted union of all members and the monitored branches in service; they cannot be blocked, a
build that does not fit `budget` is refused with the bytes needed and available.
"""
function cascadeScreenBuild!(b::DcPowerFlowBatch, events::Vector{Vector{Int64}}; monitored::Union{Nothing, Vector{Int64}} = nothing, budget::Int64 = 0)
    uploadRhs!(b)
    info = zeros(Float64, 8)
    offsets = Int64[0; cumsum(length.(events))]
    members = reduce(vcat, events; init = Int64[])
    if monitored === nothing
        check(ccall((:jg_dc_cascade_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}),
            b.token, length(events), offsets, members, 0, C_NULL, budget, info))
    else
        check(ccall((:jg_dc_cascade_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}),
            b.token, length(events), offsets, members, length(monitored), monitored, budget, info))
    end
    return info
end
"dims [6] of the cascade screen built last: events, their leading dimension, candidates, rows of Phi, monitored branches, members of the largest event"
function cascadeScreenDims(b::DcPowerFlowBatch)
    dims = zeros(Int64, 6)
    check(ccall((:jg_dc_cascade_get_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, dims))
    return dims
end
"the candidates of the cascade screen built last: the union of the initiating members and the monitored branches in service, ascending"
function cascadeScreenCandidates(b::DcPowerFlowBatch)
    labels = zeros(Int64, cascadeScreenDims(b)[3])
    check(ccall((:jg_dc_cascade_get_candidates, lib), Cint, (Int64, Ptr{Int64}), b.token, labels))
    return labels
end
"the base-case flows of the monitored branches of the cascade screen built last, ascending by branch"
function cascadeScreenBase(b::DcPowerFlowBatch)
    flow = zeros(Float64, cascadeScreenDims(b)[5])
    check(ccall((:jg_dc_cascade_get_base, lib), Cint, (Int64, Ptr{Float64}), b.token, flow))
    return flow
end
"""
    cascadeScreen(b, c0, c1; rating, trip = 1.0, rule = 0, most = 8, dense = false)
        -> (status, stages, size, tripped [most, m], stage [most, m], loading [most, m], worst, worstBranch, pending, flows, ms)

The cascades c0 .. c1 - 1 (0-based), each run to its end in one kernel launch: a monitored rated branch trips when |from| / rating > trip; rule 0: every
overloaded branch leaves at once, rule 1: only the most loaded one.  Per cascade the status (0: stable, 3: the set islands a part of the grid, 5: truncated,
the next stage would exceed `most`), the stages of trips applied, the branches out at the end, the branches in the order they left with the stage and the
loading that tripped each (0 / -1 / NaN on unused slots, stage 0 and NaN on the initiating members), the worst loading of the final state and its branch,
the overloaded branches of a truncated cascade; with `dense` the final flows [monitored, c1 - c0]; the milliseconds of the kernel.
"""
function cascadeScreen(b::DcPowerFlowBatch, c0::Int64, c1::Int64; rating::Vector{Float64}, trip::Float64 = 1.0, rule::Int = 0, most::Int = 8, dense::Bool = false)
    check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    rb = c1 - c0
    status = zeros(Int32, rb); stages = zeros(Int32, rb); size = zeros(Int32, rb); pending = zeros(Int32, rb)
    tripped = zeros(Int64, most, rb); stage = zeros(Int32, most, rb); loading = zeros(Float64, most, rb)
    worst = zeros(Float64, rb); branch = zeros(Int32, rb)
    flows = dense ? zeros(Float64, cascadeScreenDims(b)[5], rb) : zeros(Float64, 0, 0)
    ms = zeros(Float64, 1)
    check(ccall((:jg_dc_cascade_run, lib), Cint, (Int64, Int64, Int64, Float64, Cint, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
                                                  Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
        b.token, c0, c1, trip, rule, most, status, stages, size, tripped, stage, loading, worst, branch, pending, dense ? pointer(flows) : Ptr{Float64}(C_NULL), ms))
    return status, stages, size, tripped, stage, loading, worst, branch, pending, flows, ms[1]
end
"milliseconds of `reps` runs on the cascades c0 .. c1 - 1 with the trip and most of the last run (HIP events): 0 rule 0 (all), 1 rule 1 (worst)"
function cascadeTimeKernel(b::DcPowerFlowBatch, kernel::Int, c0::Int64, c1::Int64, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dc_cascade_time_kernel, lib), Cint, (Int64, Cint, Int64, Int64, Cint, Ptr{Float64}), b.token, kernel, c0, c1, reps, ms))
    return ms
end
"frees what a cascade screen keeps on the device"
cascadeScreenRelease!(b::DcPowerFlowBatch) = check(ccall((:jg_dc_cascade_release, lib), Cint, (Int64,), b.token))
"""
    chanceScreenBuild!(b, factors, candidates; monitored = nothing, injection = nothing, budget = 0) -> info [12]

The DC probabilistic N-1 screen under Gaussian injection uncertainty (jgrid.h: jg_dc_chance_*): `factors` is `[buses, r]` with 1 <= r <= 32, the injections
are p0 + factors * xi with xi ~ N(0, I); one sweep pair per factor and one per candidate branch (indices, in service, ascending), no sample.  `injection`
is the right-hand side of p0 `[buses]` as `setInjections!` takes it (default: the base case of `b`); `monitored` and `budget` as `pairScreenBuild!`.
"""
function chanceScreenBuild!(b::DcPowerFlowBatch, factors::Matrix{Float64}, candidates::Vector{Int64}; monitored::Union{Nothing, Vector{Int64}} = nothing,
                            injection::Union{Nothing, Vector{Float64}} = nothing, budget::Int64 = 0)
    uploadRhs!(b)
    info = zeros(Float64, 12)
    mon = monitored === nothing ? Int64[] : monitored
    check(ccall((:jg_dc_chance_build, lib), Cint, (Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64}),
        b.token, size(factors, 2), factors, length(candidates), candidates, length(mon), monitored === nothing ? Ptr{Int64}(C_NULL) : pointer(mon),
        injection === nothing ? Ptr{Float64}(C_NULL) : pointer(injection), budget, info))
    return info
end
"dims [6] of the chance screen built last: candidates, their leading dimension, rows of Phi, monitored branches, factors, leading dimension of S"
function chanceScreenDims(b::DcPowerFlowBatch)
    dims = zeros(Int64, 6)
    check(ccall((:jg_dc_chance_get_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, dims))
    return dims
end
"the base case of the chance screen built last, no outage: (mean, std, probability) per monitored branch, ascending by branch"
function chanceScreenBase(b::DcPowerFlowBatch; rating::Vector{Float64})
    check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    nm = chanceScreenDims(b)[4]
    mean = zeros(Float64, nm); std = zeros(Float64, nm); probability = zeros(Float64, nm)
    check(ccall((:jg_dc_chance_get_base, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.token, mean, std, probability))
    return mean, std, probability
end
"""
    chanceScreen(b, k0, k1; rating, probability = 0.05, capacity = 2^20, dense = false) -> (status, worst, worstBranch, count, records [5, m], totals [5], mean, std, p)

The candidates k0 .. k1 - 1 (0-based positions): per candidate the status (3: a bridge), the largest probability that a monitored branch exceeds its rating,
that branch and the number of branches with P >= `probability`; the records (k, m, mean, std, P) sorted by (k, m); the totals; with `dense` the mean, the
standard deviation and the probability [monitored, k1 - k0] (NaN for status 3).
"""
function chanceScreen(b::DcPowerFlowBatch, k0::Int64, k1::Int64; rating::Vector{Float64}, probability::Float64 = 0.05, capacity::Int64 = 2^20, dense::Bool = false)
    check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    rb = k1 - k0
    records = Matrix{Float64}(undef, 5, capacity)
    totals = zeros(Int64, 5)
    status = zeros(Int32, rb); worst = zeros(Float64, rb); branch = zeros(Int32, rb); count = zeros(Int32, rb)
    nm = dense ? chanceScreenDims(b)[4] : 0
    mean = zeros(Float64, nm, dense ? rb : 0); std = zeros(Float64, nm, dense ? rb : 0); p = zeros(Float64, nm, dense ? rb : 0)
    none = Ptr{Float64}(C_NULL)
    check(ccall((:jg_dc_chance_screen, lib), Cint, (Int64, Int64, Int64, Float64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32},
                                                    Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.token, k0, k1, probability, capacity, records, totals, worst, branch, count, status, dense ? pointer(mean) : none, dense ? pointer(std) : none,
        dense ? pointer(p) : none))
    return status, worst, branch, count, records[:, 1:totals[4]], totals, mean, std, p
end
"milliseconds of `reps` runs on the candidates k0 .. k1 - 1 (HIP events): 0 the chance screen kernel, 1 the base-case kernel"
function chanceTimeKernel(b::DcPowerFlowBatch, kernel::Int, k0::Int64, k1::Int64, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dc_chance_time_kernel, lib), Cint, (Int64, Cint, Int64, Int64, Cint, Ptr{Float64}), b.token, kernel, k0, k1, reps, ms))
    return ms
end
"frees what a chance screen keeps on the device"
chanceScreenRelease!(b::DcPowerFlowBatch) = check(ccall((:jg_dc_chance_release, lib), Cint, (Int64,), b.token))
"""
    seriesScreenBuild!(b, candidates, rhs; monitored = nothing, budget = 0) -> info [12]

The DC N-1 screen over a series of injection profiles (jgrid.h: jg_dc_series_*): `rhs` is `[buses, T]`, one right-hand side per profile as
`setInjections!` takes them (net injection - shunt conductance - shiftPower).  One sweep pair per candidate branch (indices, in service, ascending; one is
allowed) and one per profile; `budget`: bytes the sensitivities and the profiles' base flows may take (0: 0.8 of the free device memory).
"""
function seriesScreenBuild!(b::DcPowerFlowBatch, candidates::Vector{Int64}, rhs::Matrix{Float64}; monitored::Union{Nothing, Vector{Int64}} = nothing, budget::Int64 = 0)
    size(rhs, 1) == dims(b)[1] || throw(DimensionMismatch("[buses, profiles] right-hand sides"))
    uploadRhs!(b)
    info = zeros(Float64, 12)
    if monitored === nothing
        check(ccall((:jg_dc_series_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}),
            b.token, length(candidates), candidates, 0, C_NULL, size(rhs, 2), rhs, budget, info))
    else
        check(ccall((:jg_dc_series_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}),
            b.token, length(candidates), candidates, length(monitored), monitored, size(rhs, 2), rhs, budget, info))
    end
    return info
end
"""
    seriesScreen(b, k0, k1, candidates, profiles; rating, threshold = 1.0, capacity = 2^20) -> (records [5, m], islanding, totals [5], worst, worstProfile, violatingProfile, base [3, T])

All cases (k, t) of the candidate positions k0 .. k1 - 1 (0-based) and every profile: the records of the cases above `threshold` sorted by (k, t) (branch k,
profile t (0-based), worst branch, worst |from| / rating, overloaded branches), the bridge candidates of the block, the totals (cases, violating, bridges,
records kept, overflow flag), the worst loading per candidate and per profile, the violating candidates per profile and the profiles' base case.
"""
function seriesScreen(b::DcPowerFlowBatch, k0::Int64, k1::Int64, candidates::Vector{Int64}, profiles::Int64; rating::Vector{Float64}, threshold::Float64 = 1.0,
                      capacity::Int64 = 2^20)
    check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    records = Matrix{Float64}(undef, 5, capacity)
    islanding = zeros(Int64, max(k1 - k0, 1))
    totals = zeros(Int64, 5)
    worst = zeros(Float64, length(candidates))
    worstProfile = zeros(Float64, profiles); violatingProfile = zeros(Int64, profiles); base = zeros(Float64, 3, profiles)
    check(ccall((:jg_dc_series_screen, lib), Cint, (Int64, Int64, Int64, Float64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64},
                                                    Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
        b.token, k0, k1, threshold, capacity, records, islanding, totals, worst, worstProfile, violatingProfile, base, C_NULL, C_NULL, C_NULL))
    return records[:, 1:totals[4]], islanding[1:totals[3]], totals, worst, worstProfile, violatingProfile, base
end
"milliseconds of `reps` runs on candidate rows k0 .. k1 - 1 (HIP events): 0 the series screen kernel, 1 its row / column summaries"
function seriesTimeKernel(b::DcPowerFlowBatch, kernel::Int, k0::Int64, k1::Int64, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dc_series_time_kernel, lib), Cint, (Int64, Cint, Int64, Int64, Cint, Ptr{Float64}), b.token, kernel, k0, k1, reps, ms))
    return ms
end
"frees the sensitivities and base flows a series screen keeps on the device"
seriesScreenRelease!(b::DcPowerFlowBatch) = check(ccall((:jg_dc_series_release, lib), Cint, (Int64,), b.token))
"island mode of the NEXT `seriesScreenBuild!`: 0 a bridge candidate is skipped (status 3), 1 it is screened on the slack's island (jgrid.h)"
seriesScreenIslandMode!(b::DcPowerFlowBatch, mode::Int) = check(ccall((:jg_dc_series_set_island_mode, lib), Cint, (Int64, Cint), b.token, mode))
"island mode of the NEXT `pairScreenBuild!`: 0 a pair with a bridge is singular (status 3), 1 its bridges are shed and it is screened on the slack's island (jgrid.h)"
pairScreenIslandMode!(b::DcPowerFlowBatch, mode::Int) = check(ccall((:jg_dc_pair_set_island_mode, lib), Cint, (Int64, Cint), b.token, mode))
"""
    pairScreenShed(b, k0, k1) -> (branches, buses, m, side, flow [bridges])

The bridge candidates among the positions k0 .. k1 - 1 (0-based) of a pair screen built in island mode 1: the branch, the number of buses that leave, the
bridge's end on the slack's side, which end that is (+1 from, -1 to), and the flow that left that end over the bridge in the base case.
"""
function pairScreenShed(b::DcPowerFlowBatch, k0::Int64, k1::Int64)
    count = zeros(Int64, 1)
    branches = zeros(Int64, max(k1 - k0, 1)); buses = zeros(Int64, max(k1 - k0, 1)); m = zeros(Int64, max(k1 - k0, 1)); side = zeros(Int64, max(k1 - k0, 1))
    check(ccall((:jg_dc_pair_get_shed_table, lib), Cint, (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        b.token, k0, k1, count, branches, buses, m, side))
    c = count[1]
    flow = zeros(Float64, max(c, 1))
    c > 0 && check(ccall((:jg_dc_pair_get_shed, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, k0, k1, flow))
    return branches[1:c], buses[1:c], m[1:c], side[1:c], flow[1:c]
end
"""
    seriesScreenShed(b, k0, k1, profiles) -> (branches, buses, m, side, flow [T, bridges])

The bridge candidates among the positions k0 .. k1 - 1 (0-based) of a series screen built in island mode 1: the branch, the number of buses that leave, the
bridge's end on the slack's side, which end that is (+1 from, -1 to), and the flow that left that end over the bridge before the outage, per profile.
"""
function seriesScreenShed(b::DcPowerFlowBatch, k0::Int64, k1::Int64, profiles::Int64)
    count = zeros(Int64, 1)
    branches = zeros(Int64, max(k1 - k0, 1)); buses = zeros(Int64, max(k1 - k0, 1)); m = zeros(Int64, max(k1 - k0, 1)); side = zeros(Int64, max(k1 - k0, 1))
    check(ccall((:jg_dc_series_get_shed_table, lib), Cint, (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        b.token, k0, k1, count, branches, buses, m, side))
    c = count[1]
    flow = zeros(Float64, profiles, max(c, 1))
    c > 0 && check(ccall((:jg_dc_series_get_shed, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, k0, k1, flow))
    return branches[1:c], buses[1:c], m[1:c], side[1:c], flow[:, 1:c]
end
"""
    transferScreenBuild!(b, candidates, directions; baseRhs = nothing, monitored = nothing, budget = 0) -> info [12]

The DC transfer-capability screen (jgrid.h: jg_dc_transfer_*): `directions` is `[buses, T]`, the net active injection per unit of transfer of every
direction (the slack takes what a direction does not balance).  `baseRhs`: the right-hand side of a base profile as `uploadRhs!` sets it (default: the
system's own).  One sweep pair per candidate branch (indices, in service, ascending; one is allowed) and one per direction; `budget`: bytes the outage and
the transfer sensitivities may take (0: 0.8 of the free device memory).
"""
function transferScreenBuild!(b::DcPowerFlowBatch, candidates::Vector{Int64}, directions::Matrix{Float64}; baseRhs::Union{Nothing, Vector{Float64}} = nothing,
                              monitored::Union{Nothing, Vector{Int64}} = nothing, budget::Int64 = 0)
    size(directions, 1) == dims(b)[1] || throw(DimensionMismatch("[buses, transfers] directions"))
    baseRhs === nothing || length(baseRhs) == dims(b)[1] || throw(DimensionMismatch("[buses] base right-hand side"))
    uploadRhs!(b)
    info = zeros(Float64, 12)
    mon = monitored === nothing ? Int64[] : monitored
    check(ccall((:jg_dc_transfer_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}),
        b.token, length(candidates), candidates, length(mon), monitored === nothing ? C_NULL : mon, size(directions, 2), directions,
        baseRhs === nothing ? C_NULL : baseRhs, budget, info))
    return info
end
"""
    transferScreen(b, k0, k1, candidates, transfers; rating, cutoff = 1e-6, amount = nothing, capacity = 2^20)
        -> (records [5, m], islanding, totals [5], worst, capability, limitingOutage, limitingBranch, base [3, T])

All cases (k, t) of the candidate positions k0 .. k1 - 1 (0-based) and every transfer: the capability per transfer over the block's outages with the outage
and the branch that give it (merge with `base[1, :]`, the base case, for the answer), the least capability per candidate, the bridge candidates of the
block, and with `amount` (one value per transfer) the records of the cases below it sorted by (k, t) (branch k, transfer t (0-based), limiting branch,
capability, flow sensitivity of the limiting branch) with the totals (cases, below their amount, bridges, records kept, overflow flag).
"""
function transferScreen(b::DcPowerFlowBatch, k0::Int64, k1::Int64, candidates::Vector{Int64}, transfers::Int64; rating::Vector{Float64}, cutoff::Float64 = 1e-6,
                        amount::Union{Nothing, Vector{Float64}} = nothing, capacity::Int64 = 2^20)
    check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    amount === nothing || length(amount) == transfers || throw(DimensionMismatch("one amount per transfer"))
    capacity = amount === nothing ? 0 : capacity
    records = Matrix{Float64}(undef, 5, max(capacity, 1))
    islanding = zeros(Int64, max(k1 - k0, 1))
    totals = zeros(Int64, 5)
    worst = fill(Inf, length(candidates))
    capability = fill(Inf, transfers); limitingOutage = zeros(Int64, transfers); limitingBranch = zeros(Int64, transfers); base = zeros(Float64, 3, transfers)
    check(ccall((:jg_dc_transfer_screen, lib), Cint, (Int64, Int64, Int64, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
                                                      Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        b.token, k0, k1, cutoff, amount === nothing ? C_NULL : amount, capacity, records, islanding, totals, worst, capability, limitingOutage, limitingBranch,
        base, C_NULL, C_NULL))
    return records[:, 1:totals[4]], islanding[1:totals[3]], totals, worst, capability, limitingOutage, limitingBranch, base
end
"milliseconds of `reps` runs on candidate rows k0 .. k1 - 1 (HIP events): 0 the transfer screen kernel, 1 its row / column summaries"
function transferTimeKernel(b::DcPowerFlowBatch, kernel::Int, k0::Int64, k1::Int64, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dc_transfer_time_kernel, lib), Cint, (Int64, Cint, Int64, Int64, Cint, Ptr{Float64}), b.token, kernel, k0, k1, reps, ms))
    return ms
end
"frees the sensitivities a transfer screen keeps on the device"
transferScreenRelease!(b::DcPowerFlowBatch) = check(ccall((:jg_dc_transfer_release, lib), Cint, (Int64,), b.token))
"island mode of the NEXT `transferScreenBuild!`: 0 a bridge candidate is skipped (status 3), 1 it is screened on the slack's island (jgrid.h)"
transferScreenIslandMode!(b::DcPowerFlowBatch, mode::Int) = check(ccall((:jg_dc_transfer_set_island_mode, lib), Cint, (Int64, Cint), b.token, mode))
"""
    transferScreenShed(b, k0, k1, transfers) -> (branches, buses, m, side, flow [bridges], transfer [T, bridges])

The bridge candidates among the positions k0 .. k1 - 1 (0-based) of a transfer screen built in island mode 1, as `seriesScreenShed`: the flow that left the
bridge's end on the slack's side at zero transfer, and per unit of each transfer (not 0: the direction is partly shed with the bridge).
"""
function transferScreenShed(b::DcPowerFlowBatch, k0::Int64, k1::Int64, transfers::Int64)
    count = zeros(Int64, 1)
    branches = zeros(Int64, max(k1 - k0, 1)); buses = zeros(Int64, max(k1 - k0, 1)); m = zeros(Int64, max(k1 - k0, 1)); side = zeros(Int64, max(k1 - k0, 1))
    check(ccall((:jg_dc_transfer_get_shed_table, lib), Cint, (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        b.token, k0, k1, count, branches, buses, m, side))
    c = count[1]
    flow = zeros(Float64, max(c, 1)); per = zeros(Float64, transfers, max(c, 1))
    c > 0 && check(ccall((:jg_dc_transfer_get_shed, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}), b.token, k0, k1, flow, per))
    return branches[1:c], buses[1:c], m[1:c], side[1:c], flow[1:c], per[:, 1:c]
end
"""
    generatorScreenBuild!(b, candidates, buses, colptr, rowidx, values; monitored = nothing, budget = 0) -> info [16]

The DC generator-outage screen (jgrid.h: jg_dc_generator_*): G-1 and generator x branch cases, the loop `updateGenerator!(system, analysis; label = g,
status = 0)`, `solve!`, `power!` around `updateBranch!(...; label = k, status = 0)` per branch.  `buses` are the distinct generator buses (indices, strictly
ascending, the slack aside); `colptr` (from 0), `rowidx` (0-based positions in `buses`) and `values` are the sparse matrix A in CSC, one column per outage:
`-Pg` at the unit's bus (the slack then picks the loss up, the reference's semantics) and whatever other units add at theirs.  One sweep pair per candidate
branch and one per generator bus, never per generator.  The loss of the slack bus's last unit is the caller's to refuse, as `updateGenerator!` does.
"""
function generatorScreenBuild!(b::DcPowerFlowBatch, candidates::Vector{Int64}, buses::Vector{Int64}, colptr::Vector{Int64}, rowidx::Vector{Int64},
                               values::Vector{Float64}; monitored::Union{Nothing, Vector{Int64}} = nothing, budget::Int64 = 0)
    length(colptr) >= 2 || throw(DimensionMismatch("colptr has one entry per generator outage and one more"))
    uploadRhs!(b)
    info = zeros(Float64, 16)
    mon = monitored === nothing ? Int64[] : monitored
    check(ccall((:jg_dc_generator_build, lib), Cint, (Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
                                                      Ptr{Float64}, Int64, Ptr{Float64}),
        b.token, length(candidates), candidates, length(mon), monitored === nothing ? C_NULL : mon, length(colptr) - 1, length(buses), buses, colptr,
        rowidx, values, budget, info))
    return info
end
"""
    generatorScreen(b, k0, k1, candidates, generators; rating, threshold = 1.0, capacity = 2^20) -> (records [5, m], islanding, totals [5], worst, worstGenerator, violatingGenerator, base [3, G])

All cases (k, g) of the candidate positions k0 .. k1 - 1 (0-based) and every generator outage, and with k0 = 0 the G-1 cases as row 0: the records of the
cases above `threshold` sorted by (k, g) (branch k, 0 for a G-1 case; generator column g (0-based); worst branch; worst |from| / rating; overloaded
branches), the bridge candidates of the block, the totals, the worst loading per candidate and per generator, the violating candidates per generator and
the G-1 cases.
"""
function generatorScreen(b::DcPowerFlowBatch, k0::Int64, k1::Int64, candidates::Vector{Int64}, generators::Int64; rating::Vector{Float64},
                         threshold::Float64 = 1.0, capacity::Int64 = 2^20)
    check(ccall((:jg_dc_set_rating, lib), Cint, (Int64, Ptr{Float64}), b.token, rating))
    records = Matrix{Float64}(undef, 5, capacity)
    islanding = zeros(Int64, max(k1 - k0, 1))
    totals = zeros(Int64, 5)
    worst = zeros(Float64, length(candidates))
    worstGenerator = zeros(Float64, generators); violatingGenerator = zeros(Int64, generators); base = zeros(Float64, 3, generators)
    check(ccall((:jg_dc_generator_screen, lib), Cint, (Int64, Int64, Int64, Float64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64},
                                                       Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
        b.token, k0, k1, threshold, capacity, records, islanding, totals, worst, worstGenerator, violatingGenerator, base, C_NULL, C_NULL, C_NULL))
    return records[:, 1:totals[4]], islanding[1:totals[3]], totals, worst, worstGenerator, violatingGenerator, base
end
"the from-end flows of every G-1 case, `[generators, rows]` on the rows of the build (monitored and candidate branches, ascending)"
function generatorScreenFlows(b::DcPowerFlowBatch, rows::Int64, generators::Int64)
    flows = zeros(Float64, generators, rows)
    check(ccall((:jg_dc_generator_get_flows, lib), Cint, (Int64, Ptr{Float64}), b.token, flows))
    return flows
end
"milliseconds of `reps` runs (HIP events): 0 the screen kernel and 1 its summaries on candidate rows k0 .. k1 - 1, 2 the kernel that forms the G-1 flows"
function generatorTimeKernel(b::DcPowerFlowBatch, kernel::Int, k0::Int64, k1::Int64, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dc_generator_time_kernel, lib), Cint, (Int64, Cint, Int64, Int64, Cint, Ptr{Float64}), b.token, kernel, k0, k1, reps, ms))
    return ms
end
"frees what a generator screen keeps on the device"
generatorScreenRelease!(b::DcPowerFlowBatch) = check(ccall((:jg_dc_generator_release, lib), Cint, (Int64,), b.token))
"island mode of the NEXT `generatorScreenBuild!`: 0 a bridge candidate is skipped (status 3), 1 it is screened on the slack's island (jgrid.h)"
generatorScreenIslandMode!(b::DcPowerFlowBatch, mode::Int) = check(ccall((:jg_dc_generator_set_island_mode, lib), Cint, (Int64, Cint), b.token, mode))
"""
    generatorScreenShed(b, k0, k1, generators) -> (branches, buses, m, side, flow [G, bridges])

The bridge candidates among the positions k0 .. k1 - 1 (0-based) of a generator screen built in island mode 1, as `seriesScreenShed`: the flow that left
the bridge's end on the slack's side before the branch outage, per generator outage.
"""
function generatorScreenShed(b::DcPowerFlowBatch, k0::Int64, k1::Int64, generators::Int64)
    count = zeros(Int64, 1)
    branches = zeros(Int64, max(k1 - k0, 1)); buses = zeros(Int64, max(k1 - k0, 1)); m = zeros(Int64, max(k1 - k0, 1)); side = zeros(Int64, max(k1 - k0, 1))
    check(ccall((:jg_dc_generator_get_shed_table, lib), Cint, (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        b.token, k0, k1, count, branches, buses, m, side))
    c = count[1]
    flow = zeros(Float64, generators, max(c, 1))
    c > 0 && check(ccall((:jg_dc_generator_get_shed, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, k0, k1, flow))
    return branches[1:c], buses[1:c], m[1:c], side[1:c], flow[:, 1:c]
end

# ---- DC state estimation with batched bad-data removal (jgrid.h: jg_dcse_*; csrc/jg_dcse.hip) ------------------------------------------------
# dcStateEstimation / solve! / power! / residualTest! / chiTest (src/stateEstimation/dcStateEstimation.jl:42-151, 342-434, badData.jl:48-117, 963-977) for
# `batch` realisations of one measurement set on ONE factor of the gain matrix.  The C handle is an Int64 token.
"""
    DcStateEstimationBatch

What `dcStateEstimation(monitoring, HIP; batch)` returns: `se` is the reference's WLS model (coefficient, mean, precision, index, built by the reference's
own `dcStateEstimationWls`), `readings` [row, batch] the lanes' means, `angle` [bus, batch], `status` and `objective` per lane after `solve!`.
"""
mutable struct DcStateEstimationBatch
    token::Int64
    system::PowerSystem
    monitoring::Measurement
    se::Any
    correct::Int64
    batch::Int64
    readings::Matrix{Float64}
    angle::Matrix{Float64}
    status::Vector{Int32}
    objective::Vector{Float64}
    from::Matrix{Float64}
    rowStatus::Vector{Int32}
    stale::Bool
end
"rows of se.coefficient as 0-based row pointers, 1-based ascending columns and values with every status taken as 1"
function dcseRows(system::PowerSystem, monitoring::Measurement, coefficient)
    dc = system.model.dc
    Ht = sparse(transpose(coefficient))
    rowptr = Ht.colptr .- 1
    col = copy(Ht.rowval)
    val = copy(Ht.nzval)
    watt = monitoring.wattmeter
    for i = 1:watt.number                                 # out-of-service rows hold stored zeros: their values with status 1 come from the model
        k = watt.layout.index[i]
        for p in Ht.colptr[i]:(Ht.colptr[i + 1] - 1)
            if watt.layout.bus[i]
                val[p] = dc.nodalMatrix[col[p], k]
            else
                a = watt.layout.from[i] ? dc.admittance[k] : -dc.admittance[k]
                val[p] = col[p] == system.branch.layout.from[k] ? a : -a
            end
        end
    end
    for p in Ht.colptr[watt.number + 1]:(Ht.colptr[end] - 1)
        val[p] = 1.0
    end
    return rowptr, col, val
end
function dcseRowStatus(monitoring::Measurement, index, number::Int64)
    status = ones(Int32, number)
    status[1:monitoring.wattmeter.number] .= monitoring.wattmeter.active.status
    for (i, row) in index
        status[row] = monitoring.pmu.angle.status[i]
    end
    return status
end
function JuliaGrid.dcStateEstimation(monitoring::Measurement, ::Type{T}; batch::Int64 = 1, device::Int64 = 0) where T <: Union{HIP, HIPOrthogonal}
    system = monitoring.system
    coefficient, mean, precision, power, index, number, inservice = JuliaGrid.dcStateEstimationWls(system, monitoring)
    se = (coefficient = coefficient, mean = mean, precision = precision, index = index, number = number, inservice = inservice)
    rowptr, col, val = dcseRows(system, monitoring, coefficient)
    status = dcseRowStatus(monitoring, index, number)
    slack = system.bus.layout.slack
    token = Ref{Int64}(0)
    check(ccall((:jg_dcse_create, lib), Cint, (Ref{Int64}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Int64, Float64, Int64, Cint),
        token, system.bus.number, number, rowptr, col, val, precision.nzval, status, slack, system.bus.voltage.angle[slack], batch, device))
    b = DcStateEstimationBatch(token[], system, monitoring, se, T === HIPOrthogonal ? 1 : 0, batch, repeat(mean, 1, batch), zeros(system.bus.number, batch),
        zeros(Int32, batch), zeros(batch), zeros(system.branch.number, batch), status, true)
    finalizer(x -> (x.token != 0 && ccall((:jg_dcse_destroy, lib), Cvoid, (Int64,), x.token); x.token = 0), b)
    br = system.branch
    check(ccall((:jg_dcse_set_branches, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
        b.token, br.number, br.layout.from, br.layout.to, system.model.dc.admittance, br.parameter.shiftAngle))
    return b
end
"{n, m, batch, ld, entries of G, factor entries, factorisation levels, forward levels, backward levels, sweep launches, sweep terms, refactorisations, Omega runs, largest |S|}"
function dims(b::DcStateEstimationBatch)
    d = zeros(Int64, 14)
    check(ccall((:jg_dcse_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, d))
    return d
end
"the means of lanes lane0 .. (0-based), a [row, count] matrix in the order of se.mean"
function setReadings!(b::DcStateEstimationBatch, z::Matrix{Float64}; lane0::Int64 = 0)
    b.readings[:, (lane0 + 1):(lane0 + size(z, 2))] .= z
    check(ccall((:jg_dcse_set_readings, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, lane0, size(z, 2), z))
    return nothing
end
"solve!(analysis) for every lane (dcStateEstimation.jl:342-434); lanes with removed rows are compensated on the shared factor"
function JuliaGrid.solve!(b::DcStateEstimationBatch)
    if b.stale
        check(ccall((:jg_dcse_set_readings, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, 0, b.batch, b.readings))
        b.stale = false
    end
    check(ccall((:jg_dcse_solve, lib), Cint, (Int64, Cint), b.token, b.correct))
    check(ccall((:jg_dcse_get_angle, lib), Cint, (Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), b.token, b.angle, b.status, b.objective))
    return nothing
end
"power!(analysis) branch part (dcAnalysis.jl:353-374): from [branch, batch]; to = -from"
function JuliaGrid.power!(b::DcStateEstimationBatch)
    check(ccall((:jg_dcse_get_flows, lib), Cint, (Int64, Ptr{Float64}), b.token, b.from))
    return nothing
end
"""
    residualTest!(b::DcStateEstimationBatch; threshold = 3.0) -> (detect, maxNormalizedResidual, index)

Per lane (badData.jl:48-117).  A lane of a batch whose maximum exceeds the threshold drops that row by compensation; a handle of batch 1 follows the
reference: the row's status becomes 0 and the gain is re-assembled and refactorised.
"""
function JuliaGrid.residualTest!(b::DcStateEstimationBatch; threshold::Float64 = 3.0)
    mx = zeros(b.batch)
    idx = zeros(Int32, b.batch)
    check(ccall((:jg_dcse_residual_test, lib), Cint, (Int64, Float64, Cint, Ptr{Float64}, Ptr{Int32}), b.token, threshold, b.batch == 1 ? 0 : 1, mx, idx))
    if b.batch == 1 && mx[1] > threshold && idx[1] > 0
        b.rowStatus[idx[1]] = 0
        b.readings[idx[1], 1] = 0.0
        b.stale = true
        check(ccall((:jg_dcse_set_weights, lib), Cint, (Int64, Ptr{Float64}, Ptr{Int32}), b.token, b.se.precision.nzval, b.rowStatus))
    end
    return (detect = mx .> threshold, maxNormalizedResidual = mx, index = idx)
end
"every normalised residual of the current estimate, [row, batch]"
function normalizedResiduals(b::DcStateEstimationBatch)
    r = Matrix{Float64}(undef, b.se.number, b.batch)
    check(ccall((:jg_dcse_get_normalized_residual, lib), Cint, (Int64, Ptr{Float64}), b.token, r))
    return r
end
"lane s drops row rows[s] of se.mean (0: none) by compensation, whatever its residual"
removeRows!(b::DcStateEstimationBatch, rows::Vector{Int32}) = check(ccall((:jg_dcse_remove_rows, lib), Cint, (Int64, Ptr{Int32}), b.token, rows))
"(rows [largest |S|, batch] (0: none), count [batch]) of the measurements the lanes have removed"
function removedRows(b::DcStateEstimationBatch)
    rows = zeros(Int32, dims(b)[14], b.batch)
    count = zeros(Int32, b.batch)
    check(ccall((:jg_dcse_get_removed, lib), Cint, (Int64, Ptr{Int32}, Ptr{Int32}), b.token, rows, count))
    return rows, count
end
"chiTest(analysis; confidence) per lane (badData.jl:963-977): (detect, threshold, objective)"
function chiTest(b::DcStateEstimationBatch; confidence::Float64 = 0.95)
    _, gone = removedRows(b)
    df = sum(b.rowStatus) .- gone .- b.system.bus.number .+ 1
    chi = [JuliaGrid.quantile(JuliaGrid.Chisq(d), confidence) for d in df]
    return (detect = b.objective .>= chi, threshold = chi, objective = b.objective)
end
"the analysis follows a changed status or variance: re-assembly and ONE numeric refactorisation (powermeter.jl:704-757, pmu.jl:877-899)"
function refreshWeights!(b::DcStateEstimationBatch)
    b.rowStatus = dcseRowStatus(b.monitoring, b.se.index, b.se.number)
    precision = 1.0 ./ vcat(b.monitoring.wattmeter.active.variance, [b.monitoring.pmu.angle.variance[i] for (i, row) in b.se.index])
    check(ccall((:jg_dcse_set_weights, lib), Cint, (Int64, Ptr{Float64}, Ptr{Int32}), b.token, precision, b.rowStatus))
    return nothing
end
"updateWattmeter!(analysis; label, active, variance, status): a reading moves the row's mean in every lane; a status or variance refactorises once"
function JuliaGrid.updateWattmeter!(b::DcStateEstimationBatch; label, active = nothing, variance = nothing, status = nothing)
    updateWattmeter!(b.monitoring; label = label, (k => v for (k, v) in pairs((active = active, variance = variance, status = status)) if v !== nothing)...)
    refreshRow!(b)
    (variance !== nothing || status !== nothing) && refreshWeights!(b)
    return nothing
end
"updatePmu!(analysis; label, angle, varianceAngle, statusAngle)"
function JuliaGrid.updatePmu!(b::DcStateEstimationBatch; label, angle = nothing, varianceAngle = nothing, statusAngle = nothing)
    updatePmu!(b.monitoring; label = label, (k => v for (k, v) in pairs((angle = angle, varianceAngle = varianceAngle, statusAngle = statusAngle)) if v !== nothing)...)
    refreshRow!(b)
    (varianceAngle !== nothing || statusAngle !== nothing) && refreshWeights!(b)
    return nothing
end
"se.mean follows the Measurement container; every lane restarts from it"
function refreshRow!(b::DcStateEstimationBatch)
    mean = JuliaGrid.dcStateEstimationWls(b.system, b.monitoring)[2]
    b.readings .= mean
    b.stale = true
    return nothing
end
"milliseconds of `reps` runs (HIP events): 0 the chain of a batch, 1 right-hand side, 2 sweep pair, 3 residual pass, 4 normalised pass, 5 Omega diagonal + pass"
function timeKernel(b::DcStateEstimationBatch, kernel::Int, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dcse_time_kernel, lib), Cint, (Int64, Cint, Cint, Ptr{Float64}), b.token, kernel, reps, ms))
    return ms
end
"""
    criticalScreen(b::DcStateEstimationBatch; correlation = nothing, capacity = 65536)

The critical measurements and critical pairs of the full measurement set (jgrid.h: jg_dcse_critical_screen): `critical` rows, `pairs` [3, k] = (i, j, gamma)
sorted by (i, j) with gamma = +-1 for the critical pairs and only for them, the exact totals, per row the `partner` of the largest |gamma| (0: none) with
its `partnerCorrelation`, and the `variance` Omega_ii.  The lanes must not have removed rows.
"""
function criticalScreen(b::DcStateEstimationBatch; correlation::Union{Nothing, Float64} = nothing, capacity::Int64 = 65536)
    m = b.se.number
    records = zeros(Float64, 3, max(capacity, 1))
    totals = zeros(Int64, 3)
    single = zeros(Int32, m)
    partner = zeros(Int32, m)
    gamma = zeros(Float64, m)
    variance = zeros(Float64, m)
    check(ccall((:jg_dcse_critical_screen, lib), Cint, (Int64, Float64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                b.token, correlation === nothing ? -1.0 : correlation, capacity, records, totals, single, partner, gamma))
    check(ccall((:jg_dcse_get_variance, lib), Cint, (Int64, Ptr{Float64}), b.token, variance))
    kept = min(totals[2] + totals[3], capacity)
    return (critical = findall(single .== 1), pairs = records[:, 1:kept], totalSingles = totals[1], totalPairs = totals[2], totalCorrelated = totals[3],
            partner = partner, partnerCorrelation = gamma, variance = variance)
end
"milliseconds of `reps` runs (HIP events) of the screen's cross pass over all rows against the first block of 512 columns"
function criticalTimeKernel(b::DcStateEstimationBatch, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dcse_critical_time_kernel, lib), Cint, (Int64, Cint, Ptr{Float64}), b.token, reps, ms))
    return ms
end
"""
    topologyCandidates!(b::DcStateEstimationBatch, branch, ptr, row, sign)

The candidate branches of the status tests and their meter columns m_k (jgrid.h: jg_dcse_topology_set): `branch` 1-based, `ptr` 0-based offsets
[count + 1], `row` 1-based rows of the set ascending in a column, `sign` +-1 (+1 from-end wattmeters of k and injection wattmeters on from(k), -1 the
to-end side).  Rows out of service are masked by the library.
"""
function topologyCandidates!(b::DcStateEstimationBatch, branch::Vector{Int64}, ptr::Vector{Int64}, row::Vector{Int64}, sign::Vector{Int32})
    check(ccall((:jg_dcse_topology_set, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}),
                b.token, length(branch), branch, ptr, row, sign))
    return length(branch)
end
"the denominators D_k, the norms m_k' W m_k and the status (0 testable, 1 critical branch, 2 unseen) of the `count` candidates, and how often they were formed"
function topologyDenominators(b::DcStateEstimationBatch, count::Int64)
    D = zeros(Float64, count)
    norm = zeros(Float64, count)
    status = zeros(Int32, count)
    runs = zeros(Int64, 1)
    check(ccall((:jg_dcse_topology_denominators, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}), b.token, D, norm, status, runs))
    return (denominator = D, norm = norm, status = status, runs = runs[1])
end
"""
    topologyScreen(b::DcStateEstimationBatch; threshold = 3.0, capacity = 65536, dense = 0)

The status test of every candidate in every lane of a solved batch whose lanes removed nothing (jgrid.h: jg_dcse_topology_screen): `records` [4, k] =
(lane, candidate, t, phi) sorted by (lane, candidate) with the exact `total`, per lane the `best` candidate (0: none is testable) with its `statistic`
and `flowError`, the `count` at or above the threshold, and with `dense` = the number of candidates every statistic [lane, candidate].
"""
function topologyScreen(b::DcStateEstimationBatch; threshold::Float64 = 3.0, capacity::Int64 = 65536, dense::Int64 = 0)
    lanes = b.batch
    records = zeros(Float64, 4, max(capacity, 1))
    totals = zeros(Int64, 2)
    best = zeros(Int32, lanes)
    statistic = zeros(Float64, lanes)
    flowError = zeros(Float64, lanes)
    count = zeros(Int32, lanes)
    all = zeros(Float64, lanes, dense)
    check(ccall((:jg_dcse_topology_screen, lib), Cint,
                (Int64, Float64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                b.token, threshold, capacity, records, totals, best, statistic, flowError, count, dense > 0 ? pointer(all) : Ptr{Float64}(C_NULL)))
    kept = min(totals[1], capacity)
    return (records = records[:, 1:kept], total = totals[1], lanesWithRecords = totals[2], best = best, statistic = statistic, flowError = flowError,
            count = count, statisticAll = all)
end
"the angles [bus, lane] of the lanes corrected for `candidate[lane]` (0: the lane's estimate as it is); the batch's own estimate is left untouched"
function topologyCorrect(b::DcStateEstimationBatch, candidate::Vector{Int32})
    angle = zeros(Float64, size(b.angle, 1), b.batch)
    check(ccall((:jg_dcse_topology_correct, lib), Cint, (Int64, Ptr{Int32}, Ptr{Float64}), b.token, candidate, angle))
    return angle
end
"milliseconds of `reps` runs (HIP events): 0 all denominators, 1 right-hand sides, 2 sweep pair, 3 denominator kernel, 4 statistic pass, 5 correction"
function topologyTimeKernel(b::DcStateEstimationBatch, kernel::Int, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dcse_topology_time, lib), Cint, (Int64, Cint, Cint, Ptr{Float64}), b.token, kernel, reps, ms))
    return ms
end

# ---- batched DC optimal power flow: ADMM on one shared factor (jgrid.h: jg_dcopf_*; csrc/jg_dcopf.hip) -------------------------------------------
# The QP level of dcOptimalPowerFlow / solve! (src/optimalPowerFlow/dcOptimalPowerFlow.jl:44-198, 298-370): min 1/2 x'Px + q'x, l <= Ax <= u with P (its
# diagonal), q and A (CSR, 0-based rowptr, 1-based ascending columns) shared by `batch` lanes and the bounds each lane's own.  The model rows of a
# PowerSystem are stated by the Python package (dcoptimalpowerflow.modelRows); per-lane arrays are [rows or variables, lane].
mutable struct DcOptimalPowerFlowBatch
    token::Int64
    variables::Int64
    rows::Int64
    batch::Int64
end
function dcOptimalPowerFlowBatch(P::Vector{Float64}, q::Vector{Float64}, rowptr::Vector{Int64}, col::Vector{Int64}, val::Vector{Float64}, equality::Vector{Int32};
                                 batch::Int64 = 1, rho::Float64 = 0.1, sigma::Float64 = 1e-6, alpha::Float64 = 1.6, device::Int64 = 0)
    token = Ref{Int64}(0)
    check(ccall((:jg_dcopf_create, lib), Cint,
                (Ref{Int64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int64, Float64, Float64, Float64, Cint),
                token, length(P), length(equality), P, q, rowptr, col, val, equality, batch, rho, sigma, alpha, device))
    b = DcOptimalPowerFlowBatch(token[], length(P), length(equality), batch)
    finalizer(x -> (x.token != 0 && ccall((:jg_dcopf_destroy, lib), Cvoid, (Int64,), x.token); x.token = 0), b)
    return b
end
"no device: K = P + sigma I + A' rho A dense from the library's term lists, the objective's scale, the rows' scales"
function opfHostModel(P::Vector{Float64}, q::Vector{Float64}, rowptr::Vector{Int64}, col::Vector{Int64}, val::Vector{Float64}, equality::Vector{Int32},
                      rho::Float64, sigma::Float64)
    n, m = length(P), length(equality)
    K = zeros(Float64, n, n)
    scale = zeros(Float64, 1)
    E = zeros(Float64, m)
    check(ccall((:jg_dcopf_host_model, lib), Cint,
                (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                n, m, P, q, rowptr, col, val, equality, rho, sigma, K, scale, E))
    return K, scale[1], E
end
"{variables, rows, batch, ld, entries of K, factor entries, factorisation levels, refactorisations, 1 if K is singular but for sigma}"
function dims(b::DcOptimalPowerFlowBatch)
    d = zeros(Int64, 9)
    check(ccall((:jg_dcopf_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, d))
    return d
end
function opfRho(b::DcOptimalPowerFlowBatch)
    r = zeros(Float64, 1)
    check(ccall((:jg_dcopf_get_rho, lib), Cint, (Int64, Ptr{Float64}), b.token, r))
    return r[1]
end
"l, u [rows, lane]; a bound at or beyond 1e20 (or infinite) is none"
function setBounds!(b::DcOptimalPowerFlowBatch, l::Matrix{Float64}, u::Matrix{Float64})
    size(l) == size(u) == (b.rows, b.batch) || throw(DimensionMismatch("bounds are [rows, lane]"))
    check(ccall((:jg_dcopf_set_bounds, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}), b.token, l, u))
end
"warm start: x [variables, lane], y [rows, lane] as `opfSolution` returns them"
function setStart!(b::DcOptimalPowerFlowBatch, x::Matrix{Float64}, y::Matrix{Float64})
    size(x) == (b.variables, b.batch) && size(y) == (b.rows, b.batch) || throw(DimensionMismatch("x is [variables, lane], y [rows, lane]"))
    check(ccall((:jg_dcopf_set_start, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}), b.token, x, y))
end
"iterations and status per lane (0 solved, 2 primal infeasible, 5 iteration limit, 3 singular), the refactorisations so far"
function JuliaGrid.solve!(b::DcOptimalPowerFlowBatch; tolerance::Float64 = 1e-9, iteration::Int64 = 100000, check_every::Int64 = 25, adapt_every::Int64 = 200)
    iterations = zeros(Int32, b.batch)
    status = zeros(Int32, b.batch)
    refactorisations = zeros(Int64, 1)
    check(ccall((:jg_dcopf_run, lib), Cint, (Int64, Float64, Int64, Int64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                b.token, tolerance, iteration, check_every, adapt_every, iterations, status, refactorisations))
    return (iterations = iterations, status = status, refactorisations = refactorisations[1])
end
"x [variables, lane], y, z [rows, lane] and the objective [lane] of the unscaled problem"
function opfSolution(b::DcOptimalPowerFlowBatch)
    x = zeros(Float64, b.variables, b.batch)
    y = zeros(Float64, b.rows, b.batch)
    z = zeros(Float64, b.rows, b.batch)
    objective = zeros(Float64, b.batch)
    check(ccall((:jg_dcopf_get, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.token, x, y, z, objective))
    return (x = x, y = y, z = z, objective = objective)
end
"one branch out per lane on the shared factor: the variables of its buses, their balance rows (1-based), its admittance, state 0 none / 1 outage / 3 bridge
(the lane is not run: status 3); the caller frees the branch's own rows through the bounds.  `clearBranchOutages!` clears the set"
function setBranchOutages!(b::DcOptimalPowerFlowBatch, fromVariable::Vector{Int64}, toVariable::Vector{Int64}, fromRow::Vector{Int64}, toRow::Vector{Int64},
                           admittance::Vector{Float64}, state::Vector{Int32})
    all(length(v) == b.batch for v in (fromVariable, toVariable, fromRow, toRow, admittance, state)) || throw(DimensionMismatch("one entry per lane"))
    check(ccall((:jg_dcopf_set_branch_outages, lib), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
                b.token, fromVariable, toVariable, fromRow, toRow, admittance, state))
end
function clearBranchOutages!(b::DcOptimalPowerFlowBatch)
    check(ccall((:jg_dcopf_set_branch_outages, lib), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
                b.token, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
end
"milliseconds of `reps` runs (HIP events): 0 one iteration, 1 right-hand side, 2 sweep pair, 3 projection step, 4 residual pass and verdict, 5 assembly and
refactorisation, 6 the outaged lanes' correction, 7 the build of their W (6, 7: with a set of outages)"
function opfTimeKernel(b::DcOptimalPowerFlowBatch, kernel::Int, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dcopf_time, lib), Cint, (Int64, Cint, Cint, Ptr{Float64}), b.token, kernel, reps, ms))
    return ms
end

# ---- batched DC least-absolute-value state estimation (jgrid.h: jg_dclav_*; csrc/jg_dclav.hip) --------------------------------------------------
# dcLavStateEstimation / solve! (src/stateEstimation/dcStateEstimation.jl:201-313, src/backend/expressions.jl:381-421) for `batch` realisations of one
# measurement set: the reference hands the LP to a JuMP optimizer; here every lane runs a primal-dual interior-point method on a lane-valued factor of
# the gain H' Q H.  The rows are those of the WLS model (dcseRows / dcseRowStatus above).  The C handle is an Int64 token.
"""
    DcLavStateEstimationBatch

What `dcLavStateEstimation(monitoring, HIP; batch)` returns: `se` holds the rows of the reference's WLS model (coefficient, mean, index), `readings`
[row, batch] the lanes' means, and after `solve!` `angle` [bus, batch], `status` (0 solved, 5 iteration limit, 1 unobservable, 3 a bad pivot in the lane),
`objective`, `iterations`, `residual`, `dual` [row, batch] and `gap` per lane.
"""
mutable struct DcLavStateEstimationBatch
    token::Int64
    system::PowerSystem
    monitoring::Measurement
    se::Any
    batch::Int64
    iteration::Int64
    tolerance::Float64
    readings::Matrix{Float64}
    angle::Matrix{Float64}
    status::Vector{Int32}
    objective::Vector{Float64}
    iterations::Vector{Int32}
    residual::Matrix{Float64}
    dual::Matrix{Float64}
    gap::Vector{Float64}
    from::Matrix{Float64}
    rowStatus::Vector{Int32}
    stale::Bool
end
function JuliaGrid.dcLavStateEstimation(monitoring::Measurement, ::Type{HIP}; batch::Int64 = 1, iteration::Int64 = 50, tolerance::Float64 = 1e-8, device::Int64 = 0)
    system = monitoring.system
    coefficient, mean, precision, power, index, number, inservice = JuliaGrid.dcStateEstimationWls(system, monitoring)
    se = (coefficient = coefficient, mean = mean, index = index, number = number, inservice = inservice)
    rowptr, col, val = dcseRows(system, monitoring, coefficient)
    status = dcseRowStatus(monitoring, index, number)
    slack = system.bus.layout.slack
    token = Ref{Int64}(0)
    check(ccall((:jg_dclav_create, lib), Cint, (Ref{Int64}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int64, Float64, Int64, Cint),
        token, system.bus.number, number, rowptr, col, val, status, slack, system.bus.voltage.angle[slack], batch, device))
    b = DcLavStateEstimationBatch(token[], system, monitoring, se, batch, iteration, tolerance, repeat(mean, 1, batch), zeros(system.bus.number, batch),
        zeros(Int32, batch), zeros(batch), zeros(Int32, batch), zeros(number, batch), zeros(number, batch), zeros(batch), zeros(system.branch.number, batch), status, true)
    finalizer(x -> (x.token != 0 && ccall((:jg_dclav_destroy, lib), Cvoid, (Int64,), x.token); x.token = 0), b)
    br = system.branch
    check(ccall((:jg_dclav_set_branches, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
        b.token, br.number, br.layout.from, br.layout.to, system.model.dc.admittance, br.parameter.shiftAngle))
    return b
end
"{n, m, batch, ld, entries of G, factor entries, factorisation levels, forward levels, backward levels, sweep launches, bytes per lane, in-service rows, factorisations, iterations of the last solve}"
function dims(b::DcLavStateEstimationBatch)
    d = zeros(Int64, 14)
    check(ccall((:jg_dclav_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, d))
    return d
end
"the means of lanes lane0 .. (0-based), a [row, count] matrix in the order of se.mean"
function setReadings!(b::DcLavStateEstimationBatch, z::Matrix{Float64}; lane0::Int64 = 0)
    b.readings[:, (lane0 + 1):(lane0 + size(z, 2))] .= z
    check(ccall((:jg_dclav_set_readings, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, lane0, size(z, 2), z))
    return nothing
end
"the status of every row (0 / 1): the next solve! starts anew on the changed set, nothing symbolic is redone"
function setRowStatus!(b::DcLavStateEstimationBatch, status::Vector{Int32})
    check(ccall((:jg_dclav_set_status, lib), Cint, (Int64, Ptr{Int32}), b.token, status))
    b.rowStatus .= status
    return nothing
end
"setInitialPoint!: `angle` [bus, batch] replaces the unit-weight least-squares estimate in the start of the NEXT solve!"
function JuliaGrid.setInitialPoint!(b::DcLavStateEstimationBatch, angle::Matrix{Float64})
    check(ccall((:jg_dclav_set_initial, lib), Cint, (Int64, Ptr{Float64}), b.token, angle))
    return nothing
end
"solve!(analysis) for every lane; every call starts anew (interior-point iterations are not warm-started)"
function JuliaGrid.solve!(b::DcLavStateEstimationBatch)
    if b.stale
        check(ccall((:jg_dclav_set_readings, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, 0, b.batch, b.readings))
        b.stale = false
    end
    check(ccall((:jg_dclav_solve, lib), Cint, (Int64, Cint, Float64), b.token, b.iteration, b.tolerance))
    check(ccall((:jg_dclav_get_angle, lib), Cint, (Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}), b.token, b.angle, b.status, b.objective, b.iterations))
    check(ccall((:jg_dclav_get_residual, lib), Cint, (Int64, Ptr{Float64}), b.token, b.residual))
    check(ccall((:jg_dclav_get_dual, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}), b.token, b.dual, b.gap))
    return nothing
end
"power!(analysis) branch part (dcAnalysis.jl:353-374): from [branch, batch]; to = -from"
function JuliaGrid.power!(b::DcLavStateEstimationBatch)
    check(ccall((:jg_dclav_get_flows, lib), Cint, (Int64, Ptr{Float64}), b.token, b.from))
    return nothing
end
"the lane-valued factor alone: `q` [row, batch] the lanes' weights, `rhs` [bus, batch] -> (H' Q H)^-1 rhs [bus, batch] and the lanes' bad-pivot flags"
function lavFactorSolve(b::DcLavStateEstimationBatch, q::Matrix{Float64}, rhs::Matrix{Float64})
    x = zeros(Float64, size(rhs))
    bad = zeros(Int32, b.batch)
    check(ccall((:jg_dclav_factor_solve, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), b.token, q, rhs, x, bad))
    return x, bad
end
"milliseconds of `reps` runs (HIP events): 0 a whole iteration but its update, 1 assembly, 2 factorisation, 3 one sweep pair, 4 the row, column and step passes"
function lavTimeKernel(b::DcLavStateEstimationBatch, kernel::Int, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dclav_time_kernel, lib), Cint, (Int64, Cint, Cint, Ptr{Float64}), b.token, kernel, reps, ms))
    return ms
end
export DcLavStateEstimationBatch, setRowStatus!, lavFactorSolve, lavTimeKernel

# ---- batched PMU least-absolute-value state estimation (jgrid.h: jg_pmulav_*; csrc/jg_pmulav.hip) ------------------------------------------------
# pmuLavStateEstimation / solve! (src/stateEstimation/pmuStateEstimation.jl:223-338, 474-512) for `batch` realisations of one PMU set: the iteration of
# the DC LAV batch without a fixed state, on the coefficient matrix of the reference's WLS model.  Readings are polar.  The C handle is an Int64 token.
"""
    PmuLavStateEstimationBatch

What `pmuLavStateEstimation(monitoring, HIP; batch)` returns: `magnitudeReading`, `angleReading` [pmu, batch] the lanes' phasors, and after `solve!`
`magnitude`, `angle` [bus, batch], `status` (0 solved, 5 iteration limit, 1 a state no in-service row touches, 3 a bad pivot in the lane), `objective`,
`iterations`, `residual`, `dual` [2 pmu, batch] and `gap` per lane.
"""
mutable struct PmuLavStateEstimationBatch
    token::Int64
    system::PowerSystem
    monitoring::Measurement
    batch::Int64
    iteration::Int64
    tolerance::Float64
    magnitudeReading::Matrix{Float64}
    angleReading::Matrix{Float64}
    magnitude::Matrix{Float64}
    angle::Matrix{Float64}
    status::Vector{Int32}
    objective::Vector{Float64}
    iterations::Vector{Int32}
    residual::Matrix{Float64}
    dual::Matrix{Float64}
    gap::Vector{Float64}
    stale::Bool
    branches::Bool
end
"the status of every PMU as the LAV model reads it: in the model only with both channels in service (pmuStateEstimation.jl:277, 304-306)"
pmuLavStatus(monitoring::Measurement) = Int32.(monitoring.pmu.magnitude.status .* monitoring.pmu.angle.status)
function JuliaGrid.pmuLavStateEstimation(monitoring::Measurement, ::Type{HIP}; batch::Int64 = 1, iteration::Int64 = 50, tolerance::Float64 = 1e-8, device::Int64 = 0)
    system = monitoring.system
    pmu = monitoring.pmu
    wls = JuliaGrid.pmuStateEstimation(monitoring)
    Ht = sparse(transpose(wls.method.coefficient))                  # CSC of H' = CSR of H, columns of a row ascending
    rowptr = Int64.(Ht.colptr .- 1)
    col = Int64.(Ht.rowval)
    token = Ref{Int64}(0)
    check(ccall((:jg_pmulav_create, lib), Cint, (Ref{Int64}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int64, Cint),
        token, system.bus.number, pmu.number, rowptr, col, Ht.nzval, pmuLavStatus(monitoring), batch, device))
    b = PmuLavStateEstimationBatch(token[], system, monitoring, batch, iteration, tolerance, repeat(pmu.magnitude.mean, 1, batch), repeat(pmu.angle.mean, 1, batch),
        zeros(system.bus.number, batch), zeros(system.bus.number, batch), zeros(Int32, batch), zeros(batch), zeros(Int32, batch), zeros(2 * pmu.number, batch),
        zeros(2 * pmu.number, batch), zeros(batch), true, false)
    finalizer(x -> (x.token != 0 && ccall((:jg_pmulav_destroy, lib), Cvoid, (Int64,), x.token); x.token = 0), b)
    return b
end
"{buses, pmus, batch, ld, entries of G, factor entries, factorisation levels, forward levels, backward levels, sweep launches, bytes per lane, in-service PMUs, factorisations, iterations of the last solve}"
function dims(b::PmuLavStateEstimationBatch)
    d = zeros(Int64, 14)
    check(ccall((:jg_pmulav_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, d))
    return d
end
"the phasors of lanes lane0 .. (0-based): `magnitude`, `angle` [pmu, count] in device order"
function setReadings!(b::PmuLavStateEstimationBatch, magnitude::Matrix{Float64}, angle::Matrix{Float64}; lane0::Int64 = 0)
    b.magnitudeReading[:, (lane0 + 1):(lane0 + size(magnitude, 2))] .= magnitude
    b.angleReading[:, (lane0 + 1):(lane0 + size(angle, 2))] .= angle
    check(ccall((:jg_pmulav_set_readings, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}), b.token, lane0, size(magnitude, 2), magnitude, angle))
    return nothing
end
"the status of every PMU (0 / 1): the next solve! starts anew on the changed set, nothing symbolic is redone"
function setPmuStatus!(b::PmuLavStateEstimationBatch, status::Vector{Int32})
    check(ccall((:jg_pmulav_set_status, lib), Cint, (Int64, Ptr{Int32}), b.token, status))
    return nothing
end
"one positive scale per row [2 pmu], the same for every lane: what a row's reading is multiplied by (the rows of H handed to the constructor are the caller's)"
function setRowScale!(b::PmuLavStateEstimationBatch, scale::Vector{Float64})
    check(ccall((:jg_pmulav_set_scale, lib), Cint, (Int64, Ptr{Float64}), b.token, scale))
    return nothing
end
"setInitialPoint!: `magnitude`, `angle` [bus, batch] replace the unit-weight least-squares estimate in the start of the NEXT solve!"
function JuliaGrid.setInitialPoint!(b::PmuLavStateEstimationBatch, magnitude::Matrix{Float64}, angle::Matrix{Float64})
    check(ccall((:jg_pmulav_set_initial, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}), b.token, magnitude, angle))
    return nothing
end
"solve!(analysis) for every lane; every call starts anew (interior-point iterations are not warm-started)"
function JuliaGrid.solve!(b::PmuLavStateEstimationBatch)
    if b.stale
        check(ccall((:jg_pmulav_set_readings, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}), b.token, 0, b.batch, b.magnitudeReading, b.angleReading))
        b.stale = false
    end
    check(ccall((:jg_pmulav_solve, lib), Cint, (Int64, Cint, Float64), b.token, b.iteration, b.tolerance))
    check(ccall((:jg_pmulav_get_voltage, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
        b.token, b.magnitude, b.angle, b.status, b.objective, b.iterations))
    check(ccall((:jg_pmulav_get_residual, lib), Cint, (Int64, Ptr{Float64}), b.token, b.residual))
    check(ccall((:jg_pmulav_get_dual, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}), b.token, b.dual, b.gap))
    return nothing
end
"power! and current! of every lane: [2, branch, batch] from, to and series currents (magnitude, angle), from, to, series and charging powers (active, reactive) and [2, bus, batch] the injected power"
function pmuLavFlows(b::PmuLavStateEstimationBatch)
    system = b.system
    br = system.branch
    ac = system.model.ac
    if !b.branches
        tij = (1.0 ./ br.parameter.turnsRatio) .* exp.(-im .* br.parameter.shiftAngle)
        param = zeros(Float64, 16, br.number)
        for (c, z) in enumerate((ac.nodalFromFrom, ac.nodalFromTo, ac.nodalToFrom, ac.nodalToTo, ac.admittance, tij))
            param[2 * c - 1, :] .= real.(z)
            param[2 * c, :] .= imag.(z)
        end
        param[13, :] .= br.parameter.conductance
        param[14, :] .= br.parameter.susceptance
        param[15, :] .= 1.0 ./ br.parameter.turnsRatio
        check(ccall((:jg_pmulav_set_branches, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int8}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            b.token, br.number, br.layout.from, br.layout.to, br.layout.status, param, system.bus.shunt.conductance, system.bus.shunt.susceptance))
        b.branches = true
    end
    out = [zeros(Float64, 2, br.number, b.batch) for _ in 1:7]
    injection = zeros(Float64, 2, system.bus.number, b.batch)
    check(ccall((:jg_pmulav_get_flows, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.token, out[1], out[2], out[3], out[4], out[5], out[6], out[7], injection))
    return (fromCurrent = out[1], toCurrent = out[2], seriesCurrent = out[3], from = out[4], to = out[5], series = out[6], charging = out[7], injection = injection)
end
"the devices whose phasor residual exceeds `threshold` (per unit): rho and flag [pmu, batch], the count and the device (0-based) of the largest rho per lane"
function pmuLavSuspect(b::PmuLavStateEstimationBatch, threshold::Float64)
    number = b.monitoring.pmu.number
    rho = zeros(Float64, number, b.batch)
    flag = zeros(Int32, number, b.batch)
    count = zeros(Int32, b.batch)
    worst = zeros(Int32, b.batch)
    check(ccall((:jg_pmulav_suspect, lib), Cint, (Int64, Float64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}), b.token, threshold, rho, flag, count, worst))
    return rho, flag, count, worst
end
"milliseconds of `reps` runs (HIP events): 0 .. 4 as lavTimeKernel, 5 polar to rectangular readings, 6 rectangular to polar voltages, 7 the branch and bus pass, 8 the suspect pass"
function pmuLavTimeKernel(b::PmuLavStateEstimationBatch, kernel::Int, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_pmulav_time_kernel, lib), Cint, (Int64, Cint, Cint, Ptr{Float64}), b.token, kernel, reps, ms))
    return ms
end
export PmuLavStateEstimationBatch, pmuLavStatus, setPmuStatus!, setRowScale!, pmuLavFlows, pmuLavSuspect, pmuLavTimeKernel

# ---- batched DC Huber / Schweppe-Huber state estimation (jgrid.h: jg_dchuber_*; csrc/jg_dchuber.hip) ---------------------------------------------
# The reference has no Huber estimator; the rows are those of its DC WLS model (dcseRows / dcseRowStatus above), row i scaled by 1 / sigma_i here, and the
# bound of row i is threshold * omega[i].  Every lane runs the interior-point method of the LAV batch on the Huber QP.  The C handle is an Int64 token.
"""
    DcHuberStateEstimationBatch

What `dcHuberStateEstimation(monitoring, HIP; batch, threshold, omega)` returns: `se` holds the rows of the reference's WLS model, `readings` [row, batch]
the lanes' means (unscaled), `kappa` the bounds, and after `solve!` `angle` [bus, batch], `status` (0 solved, 5 iteration limit, 1 unobservable, 3 a bad
pivot in the lane), `objective` (the Huber loss of the scaled residuals), `iterations`, `residual` (unscaled), `weight`, `dual` [row, batch], `gap`.
"""
mutable struct DcHuberStateEstimationBatch
    token::Int64
    system::PowerSystem
    monitoring::Measurement
    se::Any
    batch::Int64
    iteration::Int64
    tolerance::Float64
    sigma::Vector{Float64}
    kappa::Vector{Float64}
    readings::Matrix{Float64}
    angle::Matrix{Float64}
    status::Vector{Int32}
    objective::Vector{Float64}
    iterations::Vector{Int32}
    residual::Matrix{Float64}
    weight::Matrix{Float64}
    dual::Matrix{Float64}
    gap::Vector{Float64}
    from::Matrix{Float64}
    rowStatus::Vector{Int32}
    stale::Bool
end
function dcHuberStateEstimation(monitoring::Measurement, ::Type{HIP}; batch::Int64 = 1, threshold::Float64 = 1.345, omega::Union{Nothing, Vector{Float64}} = nothing,
        floor::Float64 = 1e-3, iteration::Int64 = 50, tolerance::Float64 = 1e-8, device::Int64 = 0)
    system = monitoring.system
    coefficient, mean, precision, power, index, number, inservice = JuliaGrid.dcStateEstimationWls(system, monitoring)
    se = (coefficient = coefficient, mean = mean, index = index, number = number, inservice = inservice)
    rowptr, col, val = dcseRows(system, monitoring, coefficient)
    status = dcseRowStatus(monitoring, index, number)
    sigma = [1.0 / sqrt(precision[i, i]) for i in 1:number]
    scaled = copy(val)
    for i in 1:number, p in (rowptr[i] + 1):rowptr[i + 1]
        scaled[p] /= sigma[i]
    end
    kappa = threshold .* (omega === nothing ? ones(number) : clamp.(omega, floor, 1.0))
    slack = system.bus.layout.slack
    token = Ref{Int64}(0)
    check(ccall((:jg_dchuber_create, lib), Cint, (Ref{Int64}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Int64, Cint),
        token, system.bus.number, number, rowptr, col, scaled, status, kappa, sigma, slack, system.bus.voltage.angle[slack], batch, device))
    b = DcHuberStateEstimationBatch(token[], system, monitoring, se, batch, iteration, tolerance, sigma, kappa, repeat(mean, 1, batch), zeros(system.bus.number, batch),
        zeros(Int32, batch), zeros(batch), zeros(Int32, batch), zeros(number, batch), zeros(number, batch), zeros(number, batch), zeros(batch),
        zeros(system.branch.number, batch), status, true)
    finalizer(x -> (x.token != 0 && ccall((:jg_dchuber_destroy, lib), Cvoid, (Int64,), x.token); x.token = 0), b)
    br = system.branch
    check(ccall((:jg_dchuber_set_branches, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
        b.token, br.number, br.layout.from, br.layout.to, system.model.dc.admittance, br.parameter.shiftAngle))
    return b
end
"as dims of the LAV batch"
function dims(b::DcHuberStateEstimationBatch)
    d = zeros(Int64, 14)
    check(ccall((:jg_dchuber_dims, lib), Cint, (Int64, Ptr{Int64}), b.token, d))
    return d
end
"the means of lanes lane0 .. (0-based), a [row, count] matrix in the order of se.mean, unscaled"
function setReadings!(b::DcHuberStateEstimationBatch, z::Matrix{Float64}; lane0::Int64 = 0)
    b.readings[:, (lane0 + 1):(lane0 + size(z, 2))] .= z
    b.stale = true
    return nothing
end
"the status of every row (0 / 1): the next solve! starts anew on the changed set, nothing symbolic is redone"
function setRowStatus!(b::DcHuberStateEstimationBatch, status::Vector{Int32})
    check(ccall((:jg_dchuber_set_status, lib), Cint, (Int64, Ptr{Int32}), b.token, status))
    b.rowStatus .= status
    return nothing
end
"new bounds kappa [row] (threshold * omega, all positive); the next solve! starts anew, as every solve! does"
function setBounds!(b::DcHuberStateEstimationBatch, kappa::Vector{Float64})
    check(ccall((:jg_dchuber_set_bounds, lib), Cint, (Int64, Ptr{Float64}), b.token, kappa))
    b.kappa .= kappa
    return nothing
end
"solve!(analysis) for every lane; every call starts anew (interior-point iterations are not warm-started)"
function JuliaGrid.solve!(b::DcHuberStateEstimationBatch)
    if b.stale
        check(ccall((:jg_dchuber_set_readings, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}), b.token, 0, b.batch, b.readings ./ b.sigma))
        b.stale = false
    end
    check(ccall((:jg_dchuber_solve, lib), Cint, (Int64, Cint, Float64), b.token, b.iteration, b.tolerance))
    check(ccall((:jg_dchuber_get_angle, lib), Cint, (Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}), b.token, b.angle, b.status, b.objective, b.iterations))
    check(ccall((:jg_dchuber_get_residual, lib), Cint, (Int64, Ptr{Float64}), b.token, b.residual))
    check(ccall((:jg_dchuber_get_weight, lib), Cint, (Int64, Ptr{Float64}), b.token, b.weight))
    check(ccall((:jg_dchuber_get_dual, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}), b.token, b.dual, b.gap))
    return nothing
end
"power!(analysis) branch part (dcAnalysis.jl:353-374): from [branch, batch]; to = -from"
function JuliaGrid.power!(b::DcHuberStateEstimationBatch)
    check(ccall((:jg_dchuber_get_flows, lib), Cint, (Int64, Ptr{Float64}), b.token, b.from))
    return nothing
end
"milliseconds of `reps` runs (HIP events): 0 a whole iteration but its update, 1 assembly, 2 factorisation, 3 one sweep pair, 4 the row, column and step passes"
function huberTimeKernel(b::DcHuberStateEstimationBatch, kernel::Int, reps::Int = 20)
    ms = zeros(Float64, reps)
    check(ccall((:jg_dchuber_time_kernel, lib), Cint, (Int64, Cint, Cint, Ptr{Float64}), b.token, kernel, reps, ms))
    return ms
end
export DcHuberStateEstimationBatch, dcHuberStateEstimation, setBounds!, huberTimeKernel

# ---- Gauss-Seidel power flow, one scenario per lane (jgrid.h: jg_gs_*; csrc/jg_gs.hip) ---------------------------------------------------
# gaussSeidel / mismatch! / solve! / powerFlow! (src/powerFlow/acPowerFlow.jl:563-619, 732-764, 985-1041, 1389-1433) for `batch` scenarios of one grid: a
# sweep is sequential over the buses of a scenario, so a lane runs the reference's update sequence unchanged and a powerFlow! is ONE launch.  The C
# handle is an Int64 token.  Matrices are [bus, batch].
"""
    gaussSeidel(system, HIP; batch = 1, device = 0) -> GaussSeidelBatch

`magnitude`, `angle`, `voltage` (the reference's complex `method.voltage`), `pq`, `pv`, `iteration` and `status` per scenario (0 converged, 1 the
iteration limit, 3 a mismatch that is not finite).  `power!` / `current!` / `reactiveLimit!` are not offered: `setInitialPoint!(newtonRaphson(system, HIP), b)`.
"""
mutable struct GaussSeidelBatch
    token::Int64
    system::PowerSystem
    batch::Int64
    magnitude::Matrix{Float64}
    angle::Matrix{Float64}
    voltage::Matrix{ComplexF64}
    pq::Vector{Int64}
    pv::Vector{Int64}
    iteration::Vector{Int32}
    status::Vector{Int32}
    topology::Int64                                   # the signature of acPowerFlow.jl:611-614
    type::Int64
    outages::Vector{Int64}
end
"generator.voltage.magnitude of the first in-service generator of every bus that has one (acPowerFlow.jl:1032-1033), 0 elsewhere"
function gsSetpoint(system::PowerSystem)
    g = zeros(Float64, system.bus.number)
    for (i, gens) in system.bus.supply.generator
        g[i] = system.generator.voltage.magnitude[gens[1]]
    end
    return g
end
function gaussSeidel(system::PowerSystem, ::Type{HIP}; batch::Int64 = 1, device::Int64 = 0)
    JuliaGrid.checkSlackBus(system)
    JuliaGrid.model!(system, system.model.ac)
    magnitude, angle = JuliaGrid.initializeACPowerFlow(system)
    ac, bus = system.model.ac, system.bus
    token = Ref{Int64}(0)
    yt = collect(reinterpret(Float64, ac.nodalMatrixTranspose.nzval))
    check(ccall((:jg_gs_create, lib), Cint, (Ref{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int8}, Int64, Ptr{Float64}, Int64, Cint),
        token, bus.number, ac.nodalMatrix.colptr, ac.nodalMatrix.rowval, yt, bus.layout.type, bus.layout.slack, gsSetpoint(system), batch, device))
    b = GaussSeidelBatch(token[], system, batch, zeros(bus.number, batch), zeros(bus.number, batch), zeros(ComplexF64, bus.number, batch),
        findall(==(1), bus.layout.type), findall(==(2), bus.layout.type), zeros(Int32, batch), zeros(Int32, batch),
        copy(system.model.revision.topology), copy(system.model.revision.type), zeros(Int64, batch))
    finalizer(x -> (x.token != 0 && ccall((:jg_gs_destroy, lib), Cvoid, (Int64,), x.token); x.token = 0), b)
    pushInjection!(b)
    check(ccall((:jg_gs_set_voltage, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Int64), b.token, magnitude, angle, 0))
    pullVoltage!(b)
    return b
end
"bus.supply - bus.demand of the system into every lane"
function pushInjection!(b::GaussSeidelBatch)
    bus = b.system.bus
    check(ccall((:jg_gs_set_injection, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64),
        b.token, 0, b.batch, bus.supply.active .- bus.demand.active, bus.supply.reactive .- bus.demand.reactive, 0))
end
"""
    setInjections!(b, active, reactive; lane0 = 0)

Lanes lane0 .. lane0 + size(active, 2) - 1 (0-based) get net injections supply - demand of their own, [bus, count] each.
"""
function setInjections!(b::GaussSeidelBatch, active::Matrix{Float64}, reactive::Matrix{Float64}; lane0::Int64 = 0)
    check(ccall((:jg_gs_set_injection, lib), Cint, (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64),
        b.token, lane0, size(active, 2), active, reactive, size(active, 1)))
end
function pullVoltage!(b::GaussSeidelBatch)
    re, im = similar(b.magnitude), similar(b.magnitude)
    check(ccall((:jg_gs_get_voltage, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.token, b.magnitude, b.angle, re, im))
    b.voltage .= complex.(re, im)
    return nothing
end
"the system's nodal matrix again (updateBranch! / updateBus!(shunt) on the system, branch.jl:473-475); the lanes' outages follow the new values"
function pushYbus!(b::GaussSeidelBatch)
    yt = collect(reinterpret(Float64, b.system.model.ac.nodalMatrixTranspose.nzval))
    check(ccall((:jg_gs_set_ybus, lib), Cint, (Int64, Ptr{Float64}), b.token, yt))
    any(!=(0), b.outages) && setOutages!(b, b.outages)
    return nothing
end
"scenario `lane0 + s` (0-based lanes) loses branch `labels[s]` (index, 0 = none): 4 positions in the TRANSPOSED values and 4 complex deltas per lane"
function setOutages!(b::GaussSeidelBatch, labels::Vector{Int64}; lane0::Int64 = 0)
    ac, br = b.system.model.ac, b.system.branch
    Y = ac.nodalMatrix
    pos(r, c) = first(searchsorted(view(Y.rowval, Y.colptr[c]:(Y.colptr[c + 1] - 1)), r)) + Y.colptr[c] - 1
    position = zeros(Int64, 4, length(labels))
    delta = zeros(ComplexF64, 4, length(labels))
    for (s, k) in enumerate(labels)
        k == 0 && continue
        i, j = br.layout.from[k], br.layout.to[k]
        position[:, s] = [pos(i, i), pos(j, j), pos(j, i), pos(i, j)]        # Ybus entry (i, j) sits where nodalMatrix holds (j, i)
        delta[:, s] = -[ac.nodalFromFrom[k], ac.nodalToTo[k], ac.nodalFromTo[k], ac.nodalToFrom[k]]
    end
    check(ccall((:jg_gs_set_outages, lib), Cint, (Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
        b.token, lane0, length(labels), position, collect(reinterpret(Float64, vec(delta)))))
    b.outages[(lane0 + 1):(lane0 + length(labels))] .= labels
    return nothing
end
function staleCheck(b::GaussSeidelBatch)                       # acPowerFlow.jl:993-995
    rev = b.system.model.revision
    if rev.topology != b.topology || rev.type != b.type
        JuliaGrid.errorTypeConversion()
    end
end
"mismatch!(analysis) of every scenario (acPowerFlow.jl:732-764) -> (stopP, stopQ), [batch] each"
function mismatch!(b::GaussSeidelBatch)
    p, q = zeros(Float64, b.batch), zeros(Float64, b.batch)
    check(ccall((:jg_gs_mismatch, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}), b.token, p, q))
    return p, q
end
"the maxima of the last mismatch! / of the last check of powerFlow!"
function lastMismatch(b::GaussSeidelBatch)
    p, q = zeros(Float64, b.batch), zeros(Float64, b.batch)
    check(ccall((:jg_gs_get_mismatch, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}), b.token, p, q))
    return p, q
end
"solve!(analysis) of every scenario: one sweep (acPowerFlow.jl:985-1041)"
function solve!(b::GaussSeidelBatch)
    staleCheck(b)
    check(ccall((:jg_gs_solve, lib), Cint, (Int64,), b.token))
    b.iteration .+= 1
    pullVoltage!(b)
    return nothing
end
"powerFlow!(analysis; iteration, tolerance) of every scenario in one launch (acPowerFlow.jl:1389-1433)"
function powerFlow!(b::GaussSeidelBatch; iteration::Int64 = 20, tolerance::Float64 = 1e-8)
    staleCheck(b)
    check(ccall((:jg_gs_run, lib), Cint, (Int64, Int64, Float64, Ptr{Int32}, Ptr{Int32}), b.token, iteration, tolerance, b.iteration, b.status))
    pullVoltage!(b)
    return nothing
end
"setInitialPoint!(target, source) (acPowerFlow.jl:1281-1295): `magnitude`, `angle` [bus] for every scenario or [bus, batch]"
function setInitialPoint!(b::GaussSeidelBatch, magnitude::VecOrMat{Float64}, angle::VecOrMat{Float64})
    check(ccall((:jg_gs_set_voltage, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Int64), b.token, magnitude, angle, ndims(magnitude) == 1 ? 0 : size(magnitude, 1)))
    pullVoltage!(b)
    return nothing
end
"method.voltage = `voltage` bit for bit, [bus] for every scenario or [bus, batch]: the state of a batch moved to a new handle"
function setVoltage!(b::GaussSeidelBatch, voltage::VecOrMat{ComplexF64})
    check(ccall((:jg_gs_set_voltage_rect, lib), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Int64), b.token, real.(voltage), imag.(voltage), ndims(voltage) == 1 ? 0 : size(voltage, 1)))
    pullVoltage!(b)
    return nothing
end
"method.voltage[idx] = magnitude[s] * cis(angle[s]) in every scenario s: what _updateBus! (bus.jl:350-362) and _updateGenerator! (generator.jl:425-430) set"
function setBusVoltage!(b::GaussSeidelBatch, idx::Int64, magnitude::Vector{Float64}, angle::Vector{Float64})
    check(ccall((:jg_gs_set_bus_voltage, lib), Cint, (Int64, Int64, Ptr{Float64}, Ptr{Float64}), b.token, idx, magnitude, angle))
    pullVoltage!(b)
    return nothing
end
"updateGenerator!(analysis; ...) after the system changed (generator.jl:410-431): injections, set-points, and the bus at its new magnitude"
function refreshGenerator!(b::GaussSeidelBatch, idx::Int64)
    staleCheck(b)
    pushInjection!(b)
    bus = b.system.generator.layout.bus[idx]
    if b.system.bus.layout.type[bus] in (2, 3)
        g = gsSetpoint(b.system)
        check(ccall((:jg_gs_set_setpoint, lib), Cint, (Int64, Ptr{Float64}), b.token, g))
        setBusVoltage!(b, bus, fill(g[bus], b.batch), b.angle[bus, :])
    end
    return nothing
end
"milliseconds of `reps` runs (HIP events): 0 powerFlow!'s launch with `sweeps` as the limit and tolerance 0, 1 the mismatch, 2 one sweep"
function timeKernel(b::GaussSeidelBatch, kernel::Int, sweeps::Int64, reps::Int = 10)
    ms = zeros(Float64, reps)
    check(ccall((:jg_gs_time_kernel, lib), Cint, (Int64, Cint, Int64, Cint, Ptr{Float64}), b.token, kernel, sweeps, reps, ms))
    return ms
end

export HIP, HIPOrthogonal, NewtonRaphsonBatch, BaseCase, baseInfo, baseInverseOnPattern, attach!, startFromBase!, firstIteration!, firstIterationCounts, setOutages!, shareDevice!, keepIncrement!, branchQuantities, screenSummary, powerFlowDefer!, moveLanes!, finish!, resume!, jacobian!,
       largestNormalizedResidual, normalizedResiduals, commUniqueId, Comm, shard, contingencyAnalysis, clearPlanCache,
       deviceCount, dims, setRefinement!, deviceMaps, setOutage!, snapshotVoltage!, restoreVoltage!, iterations, voltageDevice!, packResults!, packRows!,
       allgatherDevice, commRank, commWorld, timeKernel, setBusType!, busType, GaussNewtonBatch, setRealisations!, monteCarloEstimation, fastPatch!, setReadings!, drawNoise!, measurementDevice,
       DcPowerFlowBatch, setInjections!, setOutagePairs!, pairScreenBuild!, pairScreen, pairTimeKernel, pairScreenRelease!, pairScreenIslandMode!, pairScreenShed, seriesScreenIslandMode!, seriesScreenShed, transferScreenIslandMode!, transferScreenShed, generatorScreenBuild!, generatorScreen, generatorScreenFlows, generatorTimeKernel, generatorScreenRelease!, generatorScreenIslandMode!, generatorScreenShed, groupScreenBuild!, groupScreenDims, groupScreenCandidates, groupScreenBase, groupScreen, groupTimeKernel, groupScreenRelease!, cascadeScreenBuild!, cascadeScreen, cascadeScreenDims, cascadeScreenCandidates, cascadeScreenBase, cascadeTimeKernel, cascadeScreenRelease!, seriesScreenBuild!, seriesScreen, seriesTimeKernel, seriesScreenRelease!, setIslandMode!, islands, islandTable, fromPower, angleDevice, DcStateEstimationBatch, removedRows, removeRows!, criticalScreen, criticalTimeKernel, topologyCandidates!, topologyDenominators, topologyScreen, topologyCorrect, topologyTimeKernel, DcOptimalPowerFlowBatch, dcOptimalPowerFlowBatch, opfHostModel, opfRho, setBounds!, setStart!, opfSolution, setBranchOutages!, clearBranchOutages!, opfTimeKernel,
       GaussSeidelBatch, lastMismatch, setBusVoltage!, refreshGenerator!

end # module
