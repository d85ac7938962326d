// The decisions of one flush as a pure function: what tick_launch (gwaoi_world.cpp) knows when a
// flush begins (FlushFacts) -> how the flush runs (FlushPlan).  No HIP, no world: plain values in,
// plain values out, so tests/cpp/plan_test.cpp checks every combination on the host.  DESIGN.md,
// "The flush plan", lists each decision with what it switches.
#pragma once

#include <cstddef>
#include <cstdint>

namespace gw {

// The flush's stages (stage timing: bit s of timing_mask = stage s is timed with events).
inline namespace stages {
enum Stage { ST_APPLY, ST_KEYGEN, ST_SORT, ST_GATHER, ST_CELLS, ST_COMBINED, ST_SPECIAL, ST_FINISH, ST_D2H, ST_N };
}

// A flush whose queue is only device batches, at most this many, is applied in a single pass.
constexpr uint32_t MAX_MOVE_RUNS = 4;

struct FlushFacts {
    // ---- counts
    uint32_t n_prev;      // entries of the previous frame
    uint32_t n_app_host;  // slots the host Enter calls append to S'
    uint32_t dev_app;     // ... and the queued device Enter batches
    uint32_t n_alive;     // live entities after this flush's ops
    uint32_t n_ops;       // ops in the queue
    size_t host_ops;      // ... of them in host runs
    size_t n_runs;
    uint32_t max_slots;
    uint32_t tiles_new, tiles_prev;  // combined_tiles(n_alive), combined_blocks(n_prev)
    // ---- the runs: every one a plain Moved batch (a device run, RUN_MOVE, implicit seqs, no space per op)
    bool all_plain_moves;
    // ---- world state
    bool dev_struct;     // a device Enter/Leave batch is queued
    bool unique_moves;   // GWAOI_F_UNIQUE_MOVES
    bool have_bucketed;  // the bucketed apply's buffers exist
    bool force_radix, force_copy, check_stages;  // GWAOI_F_TEST_*
    uint32_t timing_mask;
    bool ovl_ok;    // a speculative launch
    bool mid_last;  // the previous flush recorded its set's mid event
    bool gen_same;  // nothing but that flush was queued on the stream since its launch (gen == gen_launch)
    // that flush's special pass rode on its sort (its plan's sp_fused; true when no flush preceded): it
    // has read keygen's special-tile flags before its mid event
    bool prev_sp_fused;
    // ---- grid
    uint32_t total_cells;
    bool prev_grid_same;   // the previous frame was cut with this flush's grid (cells and every space's grid)
    bool frame_grid_same;  // the frame this flush writes holds this grid on the device already
    uint32_t sort_tiles;   // incr_sort_tiles(total_cells): the fused gather's bbox parts
    uint32_t parts_max;    // gather_parts(max_slots): the parts a flush set has room for
    uint32_t parts_new;    // gather_parts(n_alive): the separate gather's parts
    // ---- rotation
    int cur;         // frame of the last committed flush
    int launch_set;  // flush set this launch uses
    uint64_t seq_floor;
};

struct FlushPlan {
    int set, p_idx, n_idx;  // flush set; previous / new frame
    uint64_t seq_base;      // every seq of this flush is >= seq_base > every earlier one
    uint32_t n_app, n_total, n_new;  // appended entries, entries of S', entries of the new frame
    size_t entries;                  // per-tile event totals: [enters: new tiles | previous tiles][leaves: same]
    uint32_t n_copy;                 // previous-frame entries the prologue copies into S'
    uint32_t n_unique;               // ops of a unique-moves flush (0: no check)
    uint32_t n_parts;                // bbox parts the gather writes
    bool grid_same;      // no grid upload
    bool incr;           // incremental sort on the previous frame's cells (else the radix sort + cell count)
    bool ovl;            // early kernels on the early stream, beside the previous flush's pair passes
    bool moves_only;     // single-pass apply of device runs
    bool virt;           // virtual S': no copy of the previous frame, its spaces are S' spaces
    bool bucketed;       // the apply through slot buckets
    bool uniq;           // no claims, no fixup: keygen's count checks the promise
    bool mark_run0;      // the prologue stores run 0's claims
    bool skip_prologue;  // keygen does the per-flush zeroing (TickZero)
    bool sp_fused;       // the special pass rides on the sort's arrival launch
    bool ga_fused;       // the gather rides on the sort's merge launch
};

// What the flush must have room for before the plan is made (growing a buffer is an enqueue on the
// stream, which the plan's overlap decision reads as gen_same).
inline size_t flush_entries(const FlushFacts &f) { return 2 * ((size_t)f.tiles_new + f.tiles_prev); }
inline uint32_t flush_n_total(const FlushFacts &f) { return f.n_prev + f.n_app_host + f.dev_app; }
// the previous frame was cut with the same grid: its cells and keys are this flush's
inline bool flush_incr(const FlushFacts &f) { return !f.force_radix && f.n_prev > 0 && f.prev_grid_same; }

inline FlushPlan plan_flush(const FlushFacts &f) {
    FlushPlan p{};
    p.set = f.launch_set;
    p.p_idx = f.cur;
    p.n_idx = (f.cur + 1) % 3;  // a frame no flush that may still be re-run reads
    p.seq_base = f.seq_floor;
    p.n_app = f.n_app_host + f.dev_app;
    p.n_total = flush_n_total(f);
    p.n_new = f.n_alive;
    p.entries = flush_entries(f);
    p.grid_same = f.frame_grid_same;
    p.incr = flush_incr(f);
    // Overlap (speculative launches): only when nothing else was queued on the stream since the
    // previous flush's launch, and with no stage timing but the combined pass's.  The early kernels
    // rewrite the world's one special-tile flag array (keygen), which the previous flush's special
    // pass reads: behind its mid event unless it was fused, so only a fused flush may be overlapped.
    p.ovl = f.ovl_ok && f.mid_last && f.gen_same && f.prev_sp_fused && p.incr && f.n_prev > 0 &&
            (f.timing_mask & ~(1u << ST_COMBINED)) == 0 && !f.check_stages;
#ifdef GWAOI_EXP_NO_OVERLAP
    p.ovl = false;  // diagnostics build only: one flush at a time (the A/B of the overlap)
#endif
    // device runs only (device Enter/Leave batches included: their ops carry the space, the appended
    // entries are initialised first and S' is copied, so the single-pass apply handles them)
    p.moves_only = f.n_ops && f.host_ops == 0 && f.n_runs <= MAX_MOVE_RUNS && f.n_ops <= f.max_slots;
    // a flush of Moved batches only (or of nothing) changes no space and appends no entry
    p.virt = p.n_app == 0 && f.host_ops == 0 && !f.dev_struct && (p.moves_only || f.n_ops == 0) && !f.force_copy;
    p.bucketed = p.moves_only && f.have_bucketed;
    p.uniq = f.unique_moves && p.moves_only && p.virt && !p.bucketed && f.all_plain_moves;
    p.mark_run0 = p.moves_only && !p.bucketed && !p.uniq;
    p.n_unique = p.uniq ? f.n_ops : 0u;
    p.n_copy = p.virt ? 0u : f.n_prev;
    // a unique-moves flush on the previous grid: its apply writes only sc->err_apply / ndrop (zero
    // whenever a flush begins)
    p.skip_prologue = p.uniq && p.incr;
    p.sp_fused = p.incr && !(f.timing_mask >> ST_SPECIAL & 1u) && f.n_prev > 0;  // unless it is timed
    // unless it is timed or the grid has more scan tiles than the set has parts
    p.ga_fused = p.incr && !(f.timing_mask >> ST_GATHER & 1u) && f.sort_tiles <= f.parts_max;
#ifdef GWAOI_EXP_UNFUSED_GATHER
    p.ga_fused = false;  // diagnostics build only: the two launches
#endif
    p.n_parts = p.ga_fused ? f.sort_tiles : f.parts_new;
    return p;
}

}  // namespace gw
