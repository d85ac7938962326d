// Stand-alone test of csrc/gwaoi_plan.h: the flush's decisions as a pure function.  Part 1: named
// flushes, the expected plan written out by hand from the conditions DESIGN.md ("The flush plan")
// lists.  Part 2: the implications between the decisions, over every combination of the boolean
// facts with the counts drawn from {0, 1, 300}.  Part 3: chains of flushes, each planned with what the
// one before it left behind (no overlap directly behind a flush whose special pass was not fused).
// Prints "ok".
#include "gwaoi_plan.h"

#include <cstdio>

using gw::FlushFacts;
using gw::FlushPlan;
using gw::plan_flush;
using namespace gw::stages;

static int g_fail = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++g_fail;                                              \
        }                                                          \
    } while (0)

// A steady world: 2000 entities in a frame cut with this flush's grid (8 combined tiles, 8
// previous-frame tiles, one scan tile, room for 16 bbox parts), nothing queued, not speculative.
static FlushFacts steady() {
    FlushFacts f{};
    f.n_prev = 2000;
    f.n_alive = 2000;
    f.max_slots = 4096;
    f.tiles_new = 8;
    f.tiles_prev = 8;
    f.all_plain_moves = true;  // (no run is anything else)
    f.gen_same = true;
    f.prev_sp_fused = true;
    f.total_cells = 900;
    f.prev_grid_same = true;
    f.frame_grid_same = true;
    f.sort_tiles = 1;
    f.parts_max = 16;
    f.parts_new = 8;
    f.cur = 1;
    f.launch_set = 1;
    f.seq_floor = 1001;
    return f;
}
// ... with one plain device Moved batch of 100 ops queued
static FlushFacts one_batch() {
    FlushFacts f = steady();
    f.n_ops = 100;
    f.n_runs = 1;
    return f;
}
// ... launched speculatively behind a flush that recorded its mid event
static FlushFacts speculative() {
    FlushFacts f = one_batch();
    f.ovl_ok = true;
    f.mid_last = true;
    return f;
}

static void scenarios() {
    {  // 1. first flush: host Enters into an empty world
        FlushFacts f{};
        f.n_app_host = 2000;
        f.n_alive = 2000;
        f.n_ops = 2000;
        f.host_ops = 2000;
        f.n_runs = 1;
        f.max_slots = 4096;
        f.tiles_new = 8;
        f.gen_same = true;
        f.total_cells = 900;
        f.sort_tiles = 1;
        f.parts_max = 16;
        f.parts_new = 8;
        f.seq_floor = 1;
        const FlushPlan p = plan_flush(f);
        CHECK(p.set == 0 && p.p_idx == 0 && p.n_idx == 1 && p.seq_base == 1);
        CHECK(p.n_app == 2000 && p.n_total == 2000 && p.n_new == 2000 && p.entries == 16);
        CHECK(!p.grid_same && !p.incr && !p.virt && !p.moves_only && !p.bucketed && !p.uniq && !p.mark_run0);
        CHECK(!p.skip_prologue && p.n_copy == 0 && p.n_unique == 0);
        CHECK(!p.sp_fused && !p.ga_fused && !p.ovl && p.n_parts == 8);
    }
    {  // 2. host Moved calls on an unchanged grid
        FlushFacts f = steady();
        f.n_ops = 50;
        f.host_ops = 50;
        f.n_runs = 1;
        f.all_plain_moves = false;
        const FlushPlan p = plan_flush(f);
        CHECK(p.set == 1 && p.p_idx == 1 && p.n_idx == 2 && p.seq_base == 1001);
        CHECK(p.n_app == 0 && p.n_total == 2000 && p.n_new == 2000 && p.entries == 32);
        CHECK(p.grid_same && p.incr && !p.virt && p.n_copy == 2000 && !p.moves_only && !p.mark_run0 && !p.uniq);
        CHECK(!p.skip_prologue && p.sp_fused && p.ga_fused && p.n_parts == 1 && !p.ovl);
    }
    {  // 3. one plain device Moved batch, unchanged grid
        const FlushPlan p = plan_flush(one_batch());
        CHECK(p.incr && p.moves_only && p.virt && p.mark_run0 && !p.uniq && !p.bucketed);
        CHECK(p.n_copy == 0 && p.n_unique == 0 && !p.skip_prologue && p.sp_fused && p.ga_fused);
    }
    {  // 4. the same with unique_moves
        FlushFacts f = one_batch();
        f.unique_moves = true;
        const FlushPlan p = plan_flush(f);
        CHECK(p.moves_only && p.virt && p.uniq && p.skip_prologue && p.n_unique == 100 && !p.mark_run0);
        f.cur = 2;  // the frames rotate over three
        CHECK(plan_flush(f).p_idx == 2 && plan_flush(f).n_idx == 0);
    }
    {  // 5. unique_moves, one run carries a space per op (or explicit seqs, or is no Moved batch)
        FlushFacts f = one_batch();
        f.unique_moves = true;
        f.all_plain_moves = false;
        const FlushPlan p = plan_flush(f);
        CHECK(p.moves_only && p.virt && !p.uniq && !p.skip_prologue && p.n_unique == 0 && p.mark_run0);
    }
    {  // 6. unique_moves with bucketed buffers
        FlushFacts f = one_batch();
        f.unique_moves = true;
        f.have_bucketed = true;
        const FlushPlan p = plan_flush(f);
        CHECK(p.moves_only && p.virt && p.bucketed && !p.uniq && !p.mark_run0 && !p.skip_prologue);
    }
    {  // 7. five device runs: more than MAX_MOVE_RUNS
        FlushFacts f = one_batch();
        f.n_runs = 5;
        f.n_ops = 500;
        const FlushPlan p = plan_flush(f);
        CHECK(!p.moves_only && !p.virt && p.n_copy == 2000 && !p.mark_run0);
        f.n_runs = 4;
        CHECK(plan_flush(f).moves_only && plan_flush(f).virt);
    }
    {  // 8. force_copy
        FlushFacts f = one_batch();
        f.unique_moves = true;
        f.force_copy = true;
        const FlushPlan p = plan_flush(f);
        CHECK(p.moves_only && !p.virt && !p.uniq && p.n_copy == 2000 && p.mark_run0 && !p.skip_prologue);
    }
    for (int k = 0; k < 2; ++k) {  // 9. force_radix, or a changed grid
        FlushFacts f = speculative();
        f.unique_moves = true;
        if (k == 0) f.force_radix = true;
        else f.prev_grid_same = f.frame_grid_same = false;
        const FlushPlan p = plan_flush(f);
        CHECK(!p.incr && !p.sp_fused && !p.ga_fused && !p.ovl && p.n_parts == 8);
        CHECK(p.uniq && !p.skip_prologue);  // the prologue runs, and (not incremental) zeroes cell_start
        CHECK(p.grid_same == (k == 0));
    }
    {  // 10. a speculative launch, untimed or with only the combined pass timed
        FlushFacts f = speculative();
        CHECK(plan_flush(f).ovl);
        f.timing_mask = 1u << ST_COMBINED;
        const FlushPlan p = plan_flush(f);
        CHECK(p.ovl && p.sp_fused && p.ga_fused);
        f.gen_same = false;
        CHECK(!plan_flush(f).ovl);
        f.gen_same = true;
        f.mid_last = false;
        CHECK(!plan_flush(f).ovl);
        f.mid_last = true;
        f.ovl_ok = false;
        CHECK(!plan_flush(f).ovl);
        f.ovl_ok = true;
        f.prev_sp_fused = false;  // the previous flush's special pass still has the flags to read
        const FlushPlan q = plan_flush(f);
        CHECK(!q.ovl && q.incr && q.sp_fused && q.ga_fused);
        f.prev_sp_fused = true;
        CHECK(plan_flush(f).ovl);
    }
    {  // 11. the special pass timed too
        FlushFacts f = speculative();
        f.timing_mask = 1u << ST_COMBINED | 1u << ST_SPECIAL;
        const FlushPlan p = plan_flush(f);
        CHECK(p.incr && !p.sp_fused && p.ga_fused && !p.ovl);
    }
    {  // 12. the gather timed too
        FlushFacts f = speculative();
        f.timing_mask = 1u << ST_COMBINED | 1u << ST_GATHER;
        const FlushPlan p = plan_flush(f);
        CHECK(p.incr && p.sp_fused && !p.ga_fused && p.n_parts == 8 && !p.ovl);
    }
    {  // 13. check_stages
        FlushFacts f = speculative();
        f.check_stages = true;
        const FlushPlan p = plan_flush(f);
        CHECK(p.incr && p.sp_fused && p.ga_fused && !p.ovl);
    }
    {  // 14. an empty queue on a populated world
        const FlushPlan p = plan_flush(steady());
        CHECK(p.virt && !p.moves_only && p.n_copy == 0 && !p.mark_run0 && !p.uniq && p.incr);
    }
    {  // 15. a device Enter batch
        FlushFacts f = steady();
        f.dev_app = 10;
        f.dev_struct = true;
        f.n_ops = 10;
        f.n_runs = 1;
        f.all_plain_moves = false;
        f.n_alive = 2010;
        const FlushPlan p = plan_flush(f);
        CHECK(p.n_app == 10 && p.n_total == 2010 && p.n_new == 2010);
        CHECK(p.moves_only && !p.virt && p.n_copy == 2000 && p.mark_run0);
        f.dev_app = 0;  // a device Leave batch appends nothing, and still is no virtual S'
        CHECK(!plan_flush(f).virt);
    }
    {  // 16. more scan tiles than the set has bbox parts
        FlushFacts f = one_batch();
        f.sort_tiles = 17;
        const FlushPlan p = plan_flush(f);
        CHECK(p.incr && p.sp_fused && !p.ga_fused && p.n_parts == 8);
        f.sort_tiles = 16;
        CHECK(plan_flush(f).ga_fused && plan_flush(f).n_parts == 16);
    }
}

static void check_invariants(const FlushFacts &f) {
    const FlushPlan p = plan_flush(f);
    bool ok = true;
    ok &= !p.uniq || (p.moves_only && p.virt && !p.bucketed);
    ok &= !p.virt || (p.n_app == 0 && f.host_ops == 0);
    // n_copy == 0 <=> virt, for a world that has a previous frame (an empty one has nothing to copy)
    ok &= p.n_copy == (p.virt ? 0u : f.n_prev);
    ok &= (p.n_copy == 0) == (p.virt || f.n_prev == 0);
    ok &= p.skip_prologue == (p.uniq && p.incr);
    ok &= p.mark_run0 == (p.moves_only && !p.bucketed && !p.uniq);
    ok &= !p.sp_fused || (p.incr && f.n_prev > 0);
    ok &= !p.ga_fused || p.incr;
    ok &= !p.ovl || (p.incr && f.ovl_ok && f.mid_last);
    ok &= !p.ovl || f.prev_sp_fused;
    ok &= p.n_unique == (p.uniq ? f.n_ops : 0u);
    ok &= p.n_total == f.n_prev + p.n_app && p.n_new == f.n_alive;
    if (!ok && g_fail++ < 10)
        std::printf("invariant broken: n_prev %u app %u+%u ops %u host %zu runs %zu slots %u mask %x\n", f.n_prev,
                    f.n_app_host, f.dev_app, f.n_ops, f.host_ops, f.n_runs, f.max_slots, f.timing_mask);
}

static void invariants() {
    const uint32_t counts[3] = {0, 1, 300};
    const uint32_t masks[5] = {0, 1u << ST_COMBINED, 1u << ST_SPECIAL, 1u << ST_GATHER, (1u << ST_N) - 1u};
    FlushFacts f{};
    f.total_cells = 900;
    for (uint32_t bits = 0; bits < (1u << 13); ++bits) {
        f.all_plain_moves = bits & 1u;
        f.dev_struct = bits >> 1 & 1u;
        f.unique_moves = bits >> 2 & 1u;
        f.have_bucketed = bits >> 3 & 1u;
        f.force_radix = bits >> 4 & 1u;
        f.force_copy = bits >> 5 & 1u;
        f.check_stages = bits >> 6 & 1u;
        f.ovl_ok = bits >> 7 & 1u;
        f.mid_last = bits >> 8 & 1u;
        f.gen_same = bits >> 9 & 1u;
        f.prev_grid_same = bits >> 10 & 1u;
        f.frame_grid_same = bits >> 11 & 1u;
        f.prev_sp_fused = bits >> 12 & 1u;
        for (uint32_t c = 0; c < 6561; ++c) {  // 3^8: the eight counts
            uint32_t d = c;
            auto next = [&] {
                const uint32_t v = counts[d % 3];
                d /= 3;
                return v;
            };
            f.n_prev = next();
            f.n_app_host = next();
            f.dev_app = next();
            f.n_alive = next();
            f.n_ops = next();
            f.host_ops = next();
            f.n_runs = next();
            f.max_slots = next();
            f.tiles_new = (f.n_alive + 255) / 256;
            f.tiles_prev = (f.n_prev + 255) / 256;
            f.parts_max = f.max_slots > 256 ? 2 : 1;
            f.parts_new = f.n_alive > 256 ? 2 : 1;
            for (uint32_t m = 0; m < 5; ++m) {
                f.timing_mask = masks[m];
                for (f.sort_tiles = 1; f.sort_tiles <= 2; ++f.sort_tiles) check_invariants(f);
            }
        }
    }
}

// Part 3: chains.  Flush t+1 is planned with what flush t left behind, as tick_launch does it:
// prev_sp_fused is flush t's sp_fused and mid_last says that flush t was launched speculatively.
// The first flush of a chain is tick_begin's (not speculative), every later one is speculative.
enum Step { STEADY, GRID_CHANGE, SPECIAL_TIMED, FORCE_RADIX };

static void chain(const char *name, const Step *steps, int n) {
    bool prev_fused = true, prev_spec = false;  // no flush preceded
    int lost = 0;  // overlaps lost directly behind a non-fused flush
    for (int t = 0; t < n; ++t) {
        FlushFacts f = one_batch();
        f.ovl_ok = t > 0;
        f.mid_last = prev_spec;
        f.prev_sp_fused = prev_fused;
        if (steps[t] == GRID_CHANGE) f.prev_grid_same = f.frame_grid_same = false;
        if (steps[t] == SPECIAL_TIMED) f.timing_mask = 1u << ST_SPECIAL;
        if (steps[t] == FORCE_RADIX) f.force_radix = true;
        const FlushPlan p = plan_flush(f);
        bool ok = p.sp_fused == (steps[t] == STEADY);
        // behind a speculative flush: overlapped exactly when both that flush and this one are fused
        // (this one: incremental and untimed)
        const bool want = prev_spec && prev_fused && steps[t] == STEADY;
        ok &= p.ovl == want;
        if (prev_spec && !prev_fused) {
            ok &= !p.ovl;
            ++lost;
        }
        if (!ok && g_fail++ < 10) std::printf("chain %s: flush %d: ovl %d sp_fused %d\n", name, t, p.ovl, p.sp_fused);
        prev_fused = p.sp_fused;
        prev_spec = f.ovl_ok;
    }
    // every chain below has a non-fused speculative flush with two flushes behind it: the first loses
    // its overlap, the second (checked above: want) overlaps again
    CHECK(lost >= 1);
}

static void chains() {
    const Step grid[] = {STEADY, STEADY, GRID_CHANGE, STEADY, STEADY};
    const Step timed[] = {STEADY, STEADY, SPECIAL_TIMED, STEADY, STEADY};
    const Step radix[] = {STEADY, STEADY, FORCE_RADIX, STEADY, STEADY};
    const Step twice[] = {STEADY, STEADY, GRID_CHANGE, GRID_CHANGE, STEADY, STEADY, SPECIAL_TIMED, STEADY, STEADY};
    chain("grid change", grid, 5);
    chain("special timed", timed, 5);
    chain("force_radix", radix, 5);
    chain("two grid changes, then timed", twice, 9);
    // the overlap comes back: flush 4 of the first chain, planned on its own
    FlushFacts f = speculative();
    f.prev_sp_fused = false;
    CHECK(!plan_flush(f).ovl && plan_flush(f).sp_fused);
    f.prev_sp_fused = plan_flush(f).sp_fused;
    CHECK(plan_flush(f).ovl);
}

int main() {
    scenarios();
    chains();
    invariants();
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
