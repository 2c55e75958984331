// jg_compact.hpp -- internal: everything that decides or carries out a lane move of the Newton-Raphson handle.  Scenarios converge after different
// iteration counts (2..10 on N-1 sets).  Once enough have finished, the still-active ones are packed into the leading lanes so whole 64-lane groups drop
// out of every later launch (k_compact decides, k_lanes_permute / k_lanes_move carry the rows); the stragglers of a paused batch continue in another handle
// of the same grid (k_move_plan, k_move_rows).  The handle fills ONE Compaction when it is created and says, per call, which rows travel; nothing here knows
// what the rows mean, and nothing here allocates: the arrays are parts of the handle's arena.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace jg {

// The compaction flags, eight ints on the device, by the names every reader outside k_compact / k_verdict64 uses: PERMUTE -- this verdict's compaction moves
// lanes (the lane moves and the re-assembly behind it do nothing otherwise); ACTIVE lanes; lane GROUPS in use; length of the LIST glist, the ids of the groups
// that still hold an active lane (the launches spread exactly those); HOLD -- the batch stops for a hand-off, the active lanes stay where they are and
// dest[0 .. active) lists them.  [5 .. 7]: zero.
enum CompactFlag { CF_PERMUTE = 0, CF_ACTIVE = 1, CF_GROUPS = 2, CF_LIST = 3, CF_HOLD = 4 };

struct CompactArgs {
    int* active; int* iters; int* status; int* lu_status; int* lid; int* ppos; int mp;
    int* dest; int* group; int* glist; int* flags; int* tmp; int ld; int restore;
    int* host_count;           // nullable: pinned host word that receives the number of active scenarios (what the host loop polls:
                               // a store from this kernel instead of a memset node and a 4-byte copy node per iteration, ~20 us each)
    int* host_res;             // nullable (handles of ONE lane group): pinned host words [128] that receive iterations | status of the 64 lanes when the last scenario
                               // has finished -- jg_nr_run then returns them without two blocking 4-byte-per-lane copies (~25 us each: a tenth of a single instance's solve
                               // went into run_setup's and run_finish's small transfers, round 6)
    const double* params;      // [2] = defer_at of the run (jg_nr_run_defer; 0: none).  Once at most that many scenarios are active the host stops the batch and
                               // hands them to a pool (jg_nr_move_lanes): packing them into the first lane group -- and sending every lane home again when the
                               // batch finishes -- moved every row of the handle twice for lanes that leave anyway (round 6: k_lanes_permute was 5.8 % of the GPU
                               // time of the pipeline).  The lanes stay where they are; dest[0 .. n_active) lists them for the hand-off, flags[CF_HOLD] says so.
};

struct LaneRows { double* x; int rows; int elem; };                 // an array that travels with its lane: [rows][ld][elem] doubles (elem 1 or 2)
struct LanePair { const double* src; double* dst; int rows; };      // ... from one handle to another: [rows][ld] on both sides

// the hand-off's words on the device (the destination's): map [64] | home [64] | count [1] | source lane [64]
constexpr int MOVE_HOME = 64, MOVE_COUNT = 128, MOVE_SRCL = 129, MOVE_WORDS = 193;

struct Compaction {
    int* active; int* iters; int* status; int* lu_status; int* lid; int* ppos; int* dest; int* group; int* glist; int* cflags; int* itmp;
    int mp; int ld; double* params;
    int* report;               // pinned, device-visible: the verdict word, then iterations [64] | status [64] of a handle of one lane group
    double* stage; size_t stage_bytes;      // the two-pass move's staging area: the factor storage, dead between a verdict and the next factorisation

    // report: the count of active scenarios goes to the pinned verdict word -- and, from a handle of ONE lane group, iterations | status behind it
    CompactArgs args(int restore, bool report_) const {
        return CompactArgs{active, iters, status, lu_status, lid, ppos, mp, dest, group, glist, cflags, itmp, ld, restore,
                           report_ ? report : nullptr, report_ && ld == 64 ? report + 1 : nullptr, params};
    }
    bool fits(size_t doubles_per_lane) const { return doubles_per_lane * (size_t)ld * sizeof(double) <= stage_bytes; }
    // parameters of the run, every real scenario active with zero iterations (keep_iters: as they are), lanes in home order, all lane groups in use
    void run_setup(hipStream_t st, double tol, double max_iter, double defer_at, int lanes, bool keep_iters) const;
    // pack the active scenarios into the leading lanes (restore = 1: send every lane back home) and move `rows` (at most eight) with them
    void launch_compact(hipStream_t st, int restore, bool report_, const std::vector<LaneRows>& rows) const;
    // the hand-off of the active scenarios of this (paused) handle to lanes lane0 ... of dst: the per-lane integers, then the rows (at most six); both on st
    void launch_move_plan(hipStream_t st, const Compaction& dst, int* move, int lane0, int cap) const;
    void launch_move_rows(hipStream_t st, const Compaction& dst, const int* move, const std::vector<LanePair>& rows) const;
};

}  // namespace jg
