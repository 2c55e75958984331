// jg_lanes.hpp -- internal: what the Newton-Raphson and the Gauss-Newton handle share.  Both keep their per-scenario arrays batch-minor ([rows][ld], the
// scenarios as lanes) and hand the host scenario-major rows, so both need the same two transposes, the same staging buffer for rows in transit, the same
// wait for the pinned verdict word of an iteration graph and the same snapshot of two state arrays.  jg_nr and jg_gn derive from Lanes and fill in stream,
// batch and ld when they are created.
// Lanes also OWNS the handle's device and pinned memory: every block is allocated through alloc / upload / pin / arena into a pointer member of the handle,
// and release_all() frees whatever was allocated -- a destroy function names no pointer, and a new first-use allocation needs no second place.  The handles
// say how many ints the verdict word and what follows it take (pin(&h_counter, count)).
// Graph is ONE captured hipGraph: every iteration graph of the two handles is captured by Graph::capture, which always ends the capture it began and leaves
// nothing half-built.
// Every function that returns int returns 0 or a code whose text is behind jg_last_error() (jg::api_fail).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

namespace jg {

struct Graph {
    hipGraph_t g = nullptr; hipGraphExec_t x = nullptr;
    explicit operator bool() const { return x != nullptr; }
    // Takes capture_mutex() (for this ONE capture), begins a thread-local capture on st, runs body (0 or the project's code, its text already behind
    // jg_last_error()), ALWAYS ends the capture and instantiates only if begin, body and end all succeeded.  Any failure leaves the Graph empty and returns
    // the body's code or 2 (HIP).
    template <class Body> int capture(hipStream_t st, Body&& body) { if (int rc = begin(st)) return rc; return end(st, body()); }
    hipError_t launch(hipStream_t st) const { return hipGraphLaunch(x, st); }
    void reset();
private:
    int begin(hipStream_t st);                          // empty, locked, capturing -- or unlocked and the code
    int end(hipStream_t st, int rc);                    // ends the capture, instantiates if rc == 0, unlocks
};

// The loop control of powerFlow! and stateEstimation! for one scenario, after a check: converged = every norm STRICTLY below the tolerance
// (acPowerFlow.jl:1410, acStateEstimation.jl:1307); bad = a zero or non-finite pivot (LU status bit 4) or a NaN norm; the scenario goes on while it is real,
// neither converged nor bad and below the iteration limit (acPowerFlow.jl:1414, acStateEstimation.jl:1311).  A scenario that goes on counts its next solve!
// at once (iteration += 1, acPowerFlow.jl:908) and is counted among the active ones: the caller's stores.  Status 0 converged, 3 numeric failure, 1 neither.
// iters by address: it is read only where the rest of the rule leaves the question open, as k_check and k_gn_check always read it (a reference would let
// the compiler load it ahead of the branch).
struct Verdict { int go; int status; };          // go: 0 or 1 (an int: a bool member comes back through a byte and costs k_gn_check a register)
__device__ __forceinline__ Verdict verdict(bool conv, int lu_status, bool nan, const int* iters, int maxit, bool real) {
    const bool bad = (lu_status & 4) || nan;
    return Verdict{real && !conv && !bad && *iters < maxit, conv ? 0 : (bad ? 3 : 1)};
}

struct Part {                                           // one array of an arena: where its pointer goes, how many bytes it takes
    void** p; size_t bytes;
    template <class T> Part(T** p_, size_t bytes_) : p((void**)p_), bytes(bytes_) {}
};

struct Lanes {
    hipStream_t stream = nullptr;
    int batch = 0, ld = 0;                              // real scenarios, padded to a multiple of 64 lanes
    double* d_stage = nullptr; size_t stage_bytes = 0;  // rows on their way up or down (put_rows / get_rows): grows, goes with the handle
    int* h_counter = nullptr;                           // pinned: the word the verdict of an iteration graph lands in, and what the handle keeps behind it
    double wait_us = 0.0;                               // running mean of the host's waits for a verdict (wait: polls the word while this is short)

    // ---- the handle's memory.  p: a pointer member of the handle (its address is what is registered; the handle does not move).  A pointer that already
    // holds a block gets a new one: the old block is freed first (a grow path is one call).  The copies and fills are synchronised on the stream.
    // NEVER a part of the arena (d_vm, d_F, ...): those point INTO the one block and go with it.
    template <class T> hipError_t alloc(T** p, size_t count, bool zero = false) { return block((void**)p, count * sizeof(T), nullptr, 0, zero); }
    template <class T> int upload(T** p, const std::vector<T>& src) {                                // a block of max(size, 1) elements holding src
        return upload_fail(block((void**)p, std::max<size_t>(src.size(), 1) * sizeof(T), src.data(), src.size() * sizeof(T), false));
    }
    template <class T> hipError_t pin(T** p, size_t count) { return pinned((void**)p, count * sizeof(T)); }   // page-locked host memory
    // ONE allocation and ONE fill (zero) behind all the parts, in their order, each on a 256-byte boundary
    hipError_t arena(std::initializer_list<Part> parts);
    template <class T> void release(T** p) { drop((void**)p); }                                       // one block, now (device or pinned); *p = nullptr
    void release_all();

    // [rows][ld] -> scenario-major on the device, stream-ordered and not synchronised: ONE array into dst [batch][rows]; TWO arrays into the columns
    // [0, rows) and [rows, 2 rows) of a record dst [batch][stride]
    void collect(const double* src, double* dst, int rows) const;
    void collect2(const double* a, const double* b, double* dst, int rows, long long stride) const;
    // the columns behind them, at off: iterations | status and, obj not null, the objective -- of every scenario; stream-ordered
    void pack_tail(const int* iters, const int* status, const double* obj, double* dst, long long stride, int off) const;
    void add_iter(int* iters) const;                                   // one solve! outside the loop: iteration += 1 in every lane; stream-ordered

    // host [batch][rows] (stride = rows), ONE [rows] for every scenario (stride 0) or rows at a pitch of the caller's own -> device dst [rows][ld]; lanes
    // beyond the batch repeat the last scenario.  Synchronised.
    int put_rows(double* dst, const double* src, int64_t stride, int rows);
    int get_rows(const double* src, double* dst, size_t rows);         // device [rows][ld] -> host [batch][rows]
    int get_rows2(const double* src, double* dst, size_t rows) const;  // device [rows][ld][2] -> host [batch][rows][2]

    // a and b ([rows][ld] each) -> *a0 and *b0, allocated on first use (synchronised), and back (stream-ordered)
    int snapshot(const double* a, const double* b, double** a0, double** b0, int rows);
    int restore(double* a, double* b, const double* a0, const double* b0, int rows) const;

    // The host learns the verdict of an iteration graph from h_counter[0]: arm() before the launch, wait() after it.  whole: the wait is a whole solve of one
    // scenario -- polled whatever its length and not counted into wait_us.
    void arm() const;
    hipError_t wait(bool whole = false);

private:
    void* d_arena = nullptr;
    std::vector<void**> dev_, pinned_;                  // the pointer members that hold a block of device / pinned memory
    hipError_t block(void** p, size_t bytes, const void* src, size_t src_bytes, bool zero);
    hipError_t pinned(void** p, size_t bytes);
    void drop(void** p);
    static int upload_fail(hipError_t e);               // 0, or 2 with "upload: <HIP's text>"
    int stage_room(size_t bytes);
};

}  // namespace jg
