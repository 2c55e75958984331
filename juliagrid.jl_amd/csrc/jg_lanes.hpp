// jg_lanes.hpp -- internal: what the Newton-Raphson and the Gauss-Newton handle share of their host I/O.  Both keep their per-scenario arrays batch-minor
// ([rows][ld], the scenarios as lanes) and hand the host scenario-major rows, so both need the same two transposes, the same staging buffer for rows in
// transit, the same wait for the pinned verdict word of an iteration graph and the same snapshot of two state arrays.  jg_nr and jg_gn derive from Lanes and
// fill in stream, batch, ld and h_counter when they are created; they free d_stage and h_counter when they go.
// Every function that returns int returns 0 or a code whose text is behind jg_last_error() (jg::api_fail).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace jg {

struct Lanes {
    hipStream_t stream = nullptr;
    int batch = 0, ld = 0;                              // real scenarios, padded to a multiple of 64 lanes
    double* d_stage = nullptr; size_t stage_bytes = 0;  // rows on their way up or down (put_rows / get_rows): grows, goes with the handle
    int* h_counter = nullptr;                           // pinned: the word the verdict of an iteration graph lands in (the handle allocates it, and what follows it)
    double wait_us = 0.0;                               // running mean of the host's waits for a verdict (wait: polls the word while this is short)

    // [rows][ld] -> scenario-major on the device, stream-ordered and not synchronised: ONE array into dst [batch][rows]; TWO arrays into the columns
    // [0, rows) and [rows, 2 rows) of a record dst [batch][stride]
    void collect(const double* src, double* dst, int rows) const;
    void collect2(const double* a, const double* b, double* dst, int rows, long long stride) const;

    // host [batch][rows] (stride = rows), ONE [rows] for every scenario (stride 0) or rows at a pitch of the caller's own -> device dst [rows][ld]; lanes
    // beyond the batch repeat the last scenario.  Synchronised.
    int put_rows(double* dst, const double* src, int64_t stride, int rows);
    int get_rows(const double* src, double* dst, size_t rows);         // device [rows][ld] -> host [batch][rows]
    int get_rows2(const double* src, double* dst, size_t rows) const;  // device [rows][ld][2] -> host [batch][rows][2]

    // a and b ([rows][ld] each) -> *a0 and *b0, allocated on first use (synchronised), and back (stream-ordered)
    int snapshot(const double* a, const double* b, double** a0, double** b0, int rows) const;
    int restore(double* a, double* b, const double* a0, const double* b0, int rows) const;

    // The host learns the verdict of an iteration graph from h_counter[0]: arm() before the launch, wait() after it.  whole: the wait is a whole solve of one
    // scenario -- polled whatever its length and not counted into wait_us.
    void arm() const;
    hipError_t wait(bool whole = false);

private:
    int stage_room(size_t bytes);
};

}  // namespace jg
