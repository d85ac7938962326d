"""Speculative chains whose flushes are not all incremental and fused.

gwaoi_tick_finish(GWAOI_END_NEXT) launches flush t+1 before flush t is committed, and an overlapped
flush t+1 runs its early kernels on the early stream beside flush t's pair passes.  Keygen is one of
them and rewrites the world's one special[] flag array (a flag per previous-frame tile of 256
entries).  That is harmless only when flush t's special pass has read the flags already, i.e. rode on
its sort's arrival launch (plan.sp_fused).  A flush on a new grid, or with its special pass timed, is
not fused: its special pass runs as k_pairs on the stream behind its k_combined and reads the flags
there.  The gate (gwaoi_plan.h: `ovl` needs `prev_sp_fused`) keeps the flush behind such a flush off
the early stream.

Every scenario here runs one chain in which some flush is not fused and the flush behind it is
launched speculatively, keeps the GPU overlap alive (every batch on the device before the chain, the
events through the copy-out stream, all comparison after the chain), and compares the events of every
flush, exactly, with a second world (cells_per_dist=4, host batches, serial tick()) and with the
closed form.  The workload makes a lost flag visible: the 64 entities that jump in a flush come from
one band of the frame's row axis (z: the cell key is cz * gx + cx) on even flushes and from the
other on odd ones, and no entity of the other band moves by more than FAR_FRAC * D, so the tiles one
flush flags are tiles the next flush clears.  From the debug counters each launch is classified
(speculative, incremental, overlapped) and the overlap is asserted launch by launch: none directly
behind a flush that was not fused, every other one that can overlap does.  That identity also shows
that no buffer grew inside the chain (a growth switches the overlap off on its own).

The scout of scenarios 1 and 4 goes out to 5 x the side, not 3.5 x: the return must violate
`area_grid <= 4 * area_box + 1` in choose_grids, and (0.5 + 3.5) * 2200 + 4 D against 2200 + 4 D is
a ratio of 3.5 only.

No flush of a chain may overflow its event set by accident: a re-run of the pair passes grows a
buffer, which counts as an enqueue and takes the overlap from the next launches on its own, and that
would hide what the chain is there to show.  So every warm-up opens with one flush per flush set
that no normal flush of the chain can outgrow (Workload.shuffle, checked on the CPU).  The
event_capacity=1024 chain (workload bbox_regrow) overflows on purpose, and only in its rebuilt
flushes: in the two flushes that first see a new box (6 and 11, by when the host learns a flush's
boxes; the assertions read the counters, not these numbers) everyone outside the other parity's
band trades places, 205,000 events against sets that the Enter (131,000 events) sized to 164,000.
The rebuilt flush is clipped, its successor is launched (not overlapped: the gate), and at its commit
its pair passes run again over every tile with no flags (rerun, J.special = nullptr).  event_regrows
is read after every call, so the launch model knows the re-run: launch t+2 behind a re-run of flush t
does not overlap, launch t+3 may not (the twin set matches a grown event count).

What the code before the gate did with this file, one run each on an MI355X (per launch:
s = speculative, r = not incremental, T = special pass timed, o = overlapped, x = re-run).

On the parent commit as it was, the chains with a grid change did not get as far as the flags: the
flush behind the rebuilt one ended in "live-count mismatch" and a poisoned world, in scenario 1
already in the serial reference world.  That was a second bug, in the incremental sort's scratch
(test_incremental_sort_on_regrown_grid_gpu in test_gpu_parity.py).  Scenario 3 has no grid change:

  timing  - s so so so sT so so so so sT so so so   launches 6 and 11 overlapped behind the timed
          flushes; flush 5 lost 3,266 of 6,020 leaves and flush 10 3,884 of 5,624, against both
          references, every other flush equal.  Half of the lost leaves have a jumper of the flush
          as their source, the other half are their mirror images.

With the scratch bug fixed and still no gate, every scenario reached the hazard and lost leaves in
exactly the flushes that were not fused, nowhere else:

  bbox    - s so so so so sr so so so so sr so so so so   launches 7 and 12 overlapped; flush 6 lost
          3,090 of 5,534 leaves, flush 11 4,088 of 5,950
  auto    - s so so so so so so so so so so so sr so so so so   launch 14 overlapped; flush 13 lost
          4,448 of 8,124 leaves
  timing  as on the parent
  spaces  - s so so so so sr so so so so sr so so so so   launches 7 and 12 overlapped; flush 6 lost
          2,496 of 5,280 leaves, flush 11 2,422 of 5,600

(bbox with event_capacity=1024 lost the same leaves; its warm-up was lighter then, and flushes of
the chain re-ran their pair passes when their events landed unevenly on the eight streams of the
scratch, which is why the warm-up now opens with the shuffles.)

With the gate the pictures are the same but for the launch behind every r and T, which is `s` and
no longer `so` (bbox and spaces: 2 rebuilt flushes, 2 overlaps given up, 10 of 15 speculative
launches overlapped; auto: 1, 1 and 14 of 17; timing: 2 timed, 2 given up, 8 of 13), no flush of a
chain is re-run but the heavy ones of bbox_regrow, and every flush equals both references.
bbox_regrow: - s so so so so srx s s s so srx s s so so (both rebuilt flushes re-ran; the first grew
the event count, so launches 8 and 9 gave their overlap up, the second only the scratch: launch 13).
"""
import numpy as np
import pytest

from goworld_amd import World, pair_keys

D = np.float32(100.0)
FAR = np.float32(0.25) * D  # FAR_FRAC * D: a larger displacement on an axis makes an entity special
N = 4096                    # 16 previous-frame tiles of 256, the granule of special[]
SIDE = 2200.0               # about 34 neighbours each (31 with the border's share)
JUMPERS = 64
JITTER = 2.0
SCOUT_OUT = 5.0             # x of the scout when it is out, in sides of its space (see the module docstring)


class Workload:
    """The op log of one scenario, made on the CPU: the Enter, the warm-up batches and the chain's
    batches (every batch moves every slot once), what the closed form gives for every flush of the
    chain, and who jumped in it."""

    def __init__(self, name, flushes, space_n=(N,), scout_space=None, jumper_spaces=(0,), shrink=1.0, seed=1,
                 heavy=()):
        self.name, self.flushes, self.heavy = name, flushes, tuple(heavy)
        self.space_n = space_n
        rng = np.random.default_rng(seed)
        n = self.n = int(sum(space_n))
        self.sp = np.repeat(np.arange(len(space_n), dtype=np.uint32), space_n)
        self.side = np.array([SIDE * np.sqrt(k / N) for k in space_n])  # the density of the one-space workload
        side_of = self.side[self.sp]
        self.x0 = (rng.uniform(-0.5, 0.5, n) * side_of).astype(np.float32)
        self.z0 = (rng.uniform(-0.5, 0.5, n) * side_of).astype(np.float32)
        first = np.concatenate([[0], np.cumsum(space_n)[:-1]])
        self.scout = None if scout_space is None else int(first[scout_space])
        if self.scout is not None:  # its home: above both bands
            self.x0[self.scout] = self.z0[self.scout] = np.float32(0.4 * self.side[scout_space])
        self.seq = np.zeros(n, np.uint64)
        self.seq[:] = 1 + np.arange(n, dtype=np.uint64)  # enter_batch per space, in slot order
        self.nxt = n + 1
        self.px, self.pz = self.x0.copy(), self.z0.copy()
        self.h = self.side.copy()  # the crowd's extent on z, per space
        self.ops = []       # (order, x, z): warm-up, then chain
        self.jumpers = []   # per chain flush
        self.band_max = []  # per chain flush: the largest displacement in the other parity's band
        self.rng = rng
        self.scout_space, self.jumper_spaces, self.shrink = scout_space, jumper_spaces, shrink

    def _emit(self):
        order = self.rng.permutation(self.n).astype(np.uint32)
        self.ops.append((order, self.px[order].copy(), self.pz[order].copy()))
        self.seq[order] = self.nxt + np.arange(self.n, dtype=np.uint64)
        self.nxt += self.n

    def _scout_to(self, out):
        if self.scout is not None:
            s = self.side[self.scout_space]
            self.px[self.scout] = np.float32((SCOUT_OUT if out else 0.4) * s)
            self.pz[self.scout] = np.float32(0.4 * s)

    def warm(self, scout_out=False, zscale=None):
        """One warm-up flush: the chain's jitter and twice its jumpers, from anywhere to anywhere (the
        event sets and their scratch reach more than a flush of the chain needs), the scout where
        asked, the crowd's z scaled where asked."""
        rng, n = self.rng, self.n
        if zscale is not None:
            self.pz = (self.z0 * np.float32(zscale)).astype(np.float32)
            self.px = self.x0.copy()
        self.px = (self.px + rng.uniform(-JITTER, JITTER, n).astype(np.float32)).astype(np.float32)
        self.pz = (self.pz + rng.uniform(-JITTER, JITTER, n).astype(np.float32)).astype(np.float32)
        ids = rng.choice(n, 2 * JUMPERS, replace=False)
        half = self.side[self.sp[ids]] / 2
        self.px[ids] = (rng.uniform(-1, 1, ids.size) * half).astype(np.float32)
        self.pz[ids] = (rng.uniform(-1, 1, ids.size) * half * (zscale or 1.0)).astype(np.float32)
        self._scout_to(scout_out)
        self._emit()

    def shuffle(self, part=None):
        """One warm-up flush in which the entities of every space trade places at random: nearly every
        pair of the relation leaves and as many enter, 250,000 events.  The pair passes' scratch is
        grown to 1.25 x the extent a flush reached, and n events can reach an extent of 8 n at the
        most (ev_worst_extent: all in one of the eight streams, which happens to some degree with
        16 tiles), so after one such flush per flush set no flush of the chain (25,000 events at
        the most) can overflow, however its blocks land on the XCDs.  part: only so many entities
        of every space trade places (the chain whose rebuilt flushes are to overflow)."""
        for s in range(len(self.space_n)):
            ids = np.nonzero(self.sp == s)[0]
            if part is not None:
                ids = self.rng.choice(ids, part, replace=False)
            perm = self.rng.permutation(ids)
            self.px[ids], self.pz[ids] = self.px[perm], self.pz[perm]
        self._scout_to(False)
        self._emit()

    def band(self, parity, z, h):
        """Who is in a parity's band: the quarter of the extent below (even) or above (odd) z = 0."""
        q = (h / 4.0)[self.sp]
        return (z >= -q) & (z < 0) if parity == 0 else (z >= 0) & (z < q)

    def step(self, t, scout_out=None):
        """Flush t of the chain: jitter (and the contraction) for everyone, the jumpers of t's parity."""
        rng, n = self.rng, self.n
        ox, oz = self.px.copy(), self.pz.copy()
        self.px = (ox + rng.uniform(-JITTER, JITTER, n).astype(np.float32)).astype(np.float32)
        self.pz = (oz * np.float32(self.shrink) + rng.uniform(-JITTER, JITTER, n).astype(np.float32)).astype(np.float32)
        h_new = self.h * self.shrink
        cand = self.band(t & 1, oz, self.h)
        if self.scout is not None:
            cand[self.scout] = False
        jump = []
        for s in self.jumper_spaces:
            ids = np.nonzero(cand & (self.sp == s))[0]
            ids = rng.choice(ids, JUMPERS // len(self.jumper_spaces), replace=False)
            lo, hi = (-h_new[s] / 4, 0.0) if (t & 1) == 0 else (0.0, h_new[s] / 4)
            todo = np.ones(ids.size, bool)
            while todo.any():  # a random point of the own band, at least 3 D away on an axis
                k = int(todo.sum())
                self.px[ids[todo]] = rng.uniform(-0.5, 0.5, k).astype(np.float32) * np.float32(self.side[s])
                self.pz[ids[todo]] = rng.uniform(lo, hi, k).astype(np.float32)
                far = np.maximum(np.abs(self.px[ids] - ox[ids]), np.abs(self.pz[ids] - oz[ids])) >= 3 * D
                inband = (self.pz[ids] >= np.float32(lo)) & (self.pz[ids] < np.float32(hi))
                todo = ~(far & inband)
            jump.append(ids)
        if t in self.heavy:  # everyone outside the other parity's band trades places: more events than any flush before
            ids = np.nonzero(~self.band(1 - (t & 1), oz, self.h))[0]
            ids = np.setdiff1d(ids, np.concatenate(jump + [[self.scout]]))
            perm = rng.permutation(ids)
            self.px[ids], self.pz[ids] = ox[perm], (oz[perm] * np.float32(self.shrink)).astype(np.float32)
        if scout_out is not None:
            self._scout_to(scout_out)
        self.jumpers.append(np.concatenate(jump).astype(np.uint64))
        other = self.band(1 - (t & 1), oz, self.h)
        disp = np.maximum(np.abs(self.px - ox), np.abs(self.pz - oz))  # float32, the operands of is_near
        self.band_max.append(float(disp[other].max()))
        self.h = h_new
        self._emit()


_workloads = {}


def workload(name):
    """The scenario's op log (made once, shared by the tests that read it, never changed)."""
    if name in _workloads:
        return _workloads[name]
    if name == "bbox":  # 1. the scout goes out at flush 4 and comes home at flush 9
        wl = Workload(name, 16, scout_space=0, seed=101)
    elif name == "bbox_regrow":  # ... and the flushes that first see the new box overflow the event sets
        wl = Workload(name, 16, scout_space=0, seed=105, heavy=(6, 11))
    elif name == "auto":  # 2. the crowd thickens along z until the recommendation crosses to D/3
        wl = Workload(name, 18, shrink=0.96, seed=102)
    elif name == "timing":  # 3. the special pass timed for flushes 5 and 10
        wl = Workload(name, 14, seed=103)
    else:  # 4. three spaces, the scout in space 1, the jumpers in spaces 0 and 2
        assert name == "spaces"
        wl = Workload(name, 16, space_n=(1366, 1365, 1365), scout_space=1, jumper_spaces=(0, 2), seed=104)
    # The warm-up visits every grid the chain will meet, three flushes and more each (the frames
    # rotate over three), and ends where the chain starts.  First, one flush per flush set that
    # no flush of the chain can outgrow.
    if wl.heavy:
        # ... here only for the normal flushes: the Enter sizes one flush set (count and scratch), a
        # partial shuffle the other set's scratch, and both stay below what a heavy flush needs
        wl.shuffle(part=1150)
    else:
        wl.shuffle()
        wl.shuffle()
    if wl.scout is not None:
        for k in range(8):
            wl.warm(scout_out=k < 4)
    elif name == "auto":
        for k in range(12):  # a crowd denser than where the chain switches, then the start again
            wl.warm(zscale=0.55 if k < 6 else 1.0)
    else:
        for k in range(3):
            wl.warm()
    wl.n_warm = len(wl.ops)
    wl.start = (wl.px.copy(), wl.pz.copy(), wl.seq.copy())
    for t in range(wl.flushes):
        wl.step(t, scout_out={4: True, 9: False}.get(t) if wl.scout is not None else None)
    wl.ref = None  # the closed form's (enters, leaves) per chain flush: closed_form()
    wl.serial = None  # ... and the serial world's: serial_events()
    _workloads[name] = wl
    return wl


def closed_form(wl, oracle_mod):
    if wl.ref is None:
        Ds = {s: D for s in range(len(wl.space_n))}
        # the events of the Enter and of every warm-up flush (the first ones size the event sets)
        px, pz, seq = wl.x0.copy(), wl.z0.copy(), 1 + np.arange(wl.n, dtype=np.uint64)
        prev = oracle_mod.closed_form_pairs(px, pz, seq, wl.sp, Ds)
        wl.warm_events = [prev.size]
        for k, (order, x, z) in enumerate(wl.ops[:wl.n_warm]):
            px[order], pz[order] = x, z
            seq[order] = (k + 1) * wl.n + 1 + np.arange(wl.n, dtype=np.uint64)
            cur = oracle_mod.closed_form_pairs(px, pz, seq, wl.sp, Ds)
            wl.warm_events.append(np.setdiff1d(cur, prev).size + np.setdiff1d(prev, cur).size)
            prev = cur
        px, pz, seq = (a.copy() for a in wl.start)
        prev = oracle_mod.closed_form_pairs(px, pz, seq, wl.sp, Ds)
        nxt = int(seq.max()) + 1
        wl.ref, wl.mean_nb = [], []
        for order, x, z in wl.ops[wl.n_warm:]:
            px[order], pz[order] = x, z
            seq[order] = nxt + np.arange(wl.n, dtype=np.uint64)
            nxt += wl.n
            cur = oracle_mod.closed_form_pairs(px, pz, seq, wl.sp, Ds)
            wl.ref.append((np.setdiff1d(cur, prev), np.setdiff1d(prev, cur)))
            wl.mean_nb.append(cur.size / wl.n)
            prev = cur
    return wl.ref


def enter_all(w, wl):
    for s, k in enumerate(wl.space_n):
        assert w.space_create(D) == s
        ids = np.nonzero(wl.sp == s)[0].astype(np.uint32)
        w.enter_batch(s, ids, wl.x0[ids], wl.z0[ids])
    w.tick()


def serial_events(wl):
    """The same ops through another apply path and another grid, never speculative: host batches and
    tick() on a world with cells_per_dist=4.  Returns its events per chain flush and the world's
    neighbour rows for a stride of slots."""
    if wl.serial is None:
        with World(wl.n, max_spaces=len(wl.space_n), cells_per_dist=4.0) as B:
            enter_all(B, wl)
            ev = []
            for k, (order, x, z) in enumerate(wl.ops):
                B.moved_batch(order, x, z)
                e, l = B.tick()
                if k >= wl.n_warm:
                    ev.append((pair_keys(e), pair_keys(l)))
            assert B.debug_counters()["speculative_launches"] == 0
            wl.serial = (ev, {i: B.neighbors(i) for i in range(0, wl.n, 97)})
    return wl.serial


def run_chain(w, wl, dev, hooks):
    """The chain: flush 0 by tick_begin, every later one inside the tick_end_begin that commits the
    one before it.  Nothing else happens between two calls but queueing the next batch, the
    scenario's hook and one read of the host-side counters.  hooks: {flush: stages}, set before the
    call that launches the flush and cleared before the next call.  Returns the events per flush
    (host arrays, as returned) and the counters read after every launch."""
    T = wl.flushes
    ptrs = [tuple(b.data_ptr() for b in d) for d in dev]
    w.stage_names()
    w.set_stage_timing([])  # (caches the stage names: no lookup inside the chain)
    events, counters = [], [w.debug_counters()]
    if 0 in hooks:
        w.set_stage_timing(hooks[0])
    w.moved_batch_device(*ptrs[0], wl.n)
    w.tick_begin()
    counters.append(w.debug_counters())
    for t in range(T - 1):
        w.moved_batch_device(*ptrs[t + 1], wl.n)
        if t + 1 in hooks:
            w.set_stage_timing(hooks[t + 1])
        elif t in hooks:
            w.set_stage_timing([])
        events.append(w.tick_end_begin())
        counters.append(w.debug_counters())
    events.append(w.tick_end())
    counters.append(w.debug_counters())
    return events, counters


def classify(counters, hooks, T):
    """Per flush of the chain, from the counter deltas around its launch: speculative, incremental,
    overlapped; timed: its special pass was (the hooks say so); fused: its special pass rode on the
    sort (incremental and not timed); rerun: its pair passes ran again after an overflow (counted in
    the call that commits it, one call after its launch); expect: whether the gated plan overlaps it.
    A re-run of flush t grows a buffer after launch t+1: an enqueue that takes the overlap from launch
    t+2 (grew), and from launch t+3 when the twin set has to match a grown event count (maybe)."""
    rr = np.array([b["event_regrows"] - a["event_regrows"] for a, b in zip(counters[1:T + 1], counters[2:T + 2])])
    rerun = rr > 0
    grew, maybe = np.zeros(T, bool), np.zeros(T, bool)
    grew[2:], maybe[3:] = rerun[:-2], rerun[:-3]
    c = {k: np.array([b[k] - a[k] for a, b in zip(counters[:T], counters[1:T + 1])])
         for k in ("speculative_launches", "incremental_sorts", "overlapped_flushes")}
    assert all(v.min() >= 0 and v.max() <= 1 for v in c.values()), c
    spec, incr, ovl = (c[k].astype(bool) for k in ("speculative_launches", "incremental_sorts", "overlapped_flushes"))
    timed = np.array([f in hooks for f in range(T)])
    fused = incr & ~timed
    mid = spec  # the flush recorded its mid event
    behind = np.zeros(T, bool)  # directly behind a speculative flush that was not fused
    behind[1:] = spec[:-1] & ~fused[:-1]
    expect = spec & incr & ~timed & ~behind & ~grew
    expect[1:] &= mid[:-1]
    expect[0] = False
    return dict(spec=spec, incr=incr, ovl=ovl, timed=timed, fused=fused, mid=mid, behind=behind, expect=expect,
                rerun=rerun, grew=grew, maybe=maybe)


def picture(cl):
    return " ".join(("s" if s else "-") + ("r" if not i else "") + ("T" if t else "") + ("o" if o else "") + ("x" if x else "")
                    for s, i, t, o, x in zip(cl["spec"], cl["incr"], cl["timed"], cl["ovl"], cl["rerun"]))


def compare_events(wl, events, ref, serial):
    """Every flush against both references, exactly.  Returns one line per flush that differs."""
    bad = []
    for t, (e, l) in enumerate(events):
        ge, gl = pair_keys(e), pair_keys(l)
        for what, (re_, rl) in (("serial world", serial[t]), ("closed form", ref[t])):
            if np.array_equal(ge, re_) and np.array_equal(gl, rl):
                continue
            lost = np.setdiff1d(rl, gl)
            src = np.isin(lost >> np.uint64(32), wl.jumpers[t])
            bad.append(f"flush {t} vs {what}: enters {ge.size}/{re_.size}, leaves {gl.size}/{rl.size}, "
                       f"{lost.size} leaves lost, {int(src.sum())} of them sourced at the flush's jumpers")
    return bad


def check_workload(wl, ref):
    """What the workload promises, from the CPU side alone."""
    assert len(wl.jumpers) == wl.flushes == len(ref)
    # no entity of the other parity's band is special: the flags of a flush's jumper tiles are
    # flags the next flush clears (else an overwritten flag array could hide a loss)
    assert max(wl.band_max) <= float(FAR), wl.band_max
    # No normal flush of the chain can outgrow what the first two flushes of the world (one per flush
    # set: the Enter and a shuffle, or two shuffles behind it) left: its worst extent (every event in
    # one of the 8 streams, whole chunks of 256) is below their events, hence below their extents
    # (an extent is at least the events less 8 chunks) and the scratch grown to them.
    total = [e.size + l.size for e, l in ref]
    worst = max(-(-n // 256) * 8 * 256 for t, n in enumerate(total) if t not in wl.heavy)
    sized = wl.warm_events[:2] if wl.heavy else wl.warm_events[1:3]
    assert worst <= min(sized) - 8 * 256, (worst, wl.warm_events)
    # A heavy flush has more events than a set holds: a set is grown to 1.25 x the events of the
    # flush that overflowed it (or doubled, from 1,024), and the twin is grown to match.
    # (The first one, for certain; a later one meets sets the first has grown, and re-runs only if
    # its extent exceeds its own set's scratch.)
    for t in wl.heavy[:1]:
        assert total[t] > 1.25 * max(wl.warm_events + total[:t]) + 2048, (t, total, wl.warm_events)
    for t, (e, l) in enumerate(ref):
        assert e.size and l.size, t
        assert wl.jumpers[t].size == JUMPERS
        assert np.isin(l >> np.uint64(32), wl.jumpers[t]).sum() >= JUMPERS, t  # leaves sourced at a jumper


SCENARIOS = ["bbox", "bbox_regrow", "auto", "timing", "spaces"]
TIMED = {5: ["special"], 10: ["special"]}  # scenario 3: one odd flush, one even


@pytest.mark.parametrize("name", SCENARIOS)
def test_chain_workloads_keep_their_conditions(oracle_mod, name):
    """The band condition, enters and leaves in every flush, leaves sourced at the jumpers: decided by
    the reference alone (no GPU).  The automatic cell size must cross from D/2 to D/3 early enough for
    the switch and the flushes behind it to fall inside the chain."""
    wl = workload(name)
    check_workload(wl, closed_form(wl, oracle_mod))
    if name == "auto":
        # The library recommends D/3 from a mean of 48 neighbours (the GPU test asserts the
        # switch itself).  Well below it at the start, well above it five flushes before the end: two
        # commits recommending D/3, the switching launch and a launch behind it fall inside the chain.
        assert max(wl.mean_nb[:4]) < 40 and min(wl.mean_nb[-5:]) > 55, wl.mean_nb


def chain_scenario(oracle_mod, name, event_capacity=0):
    torch = pytest.importorskip("torch")
    wl = workload(name)
    ref = closed_form(wl, oracle_mod)
    check_workload(wl, ref)
    hooks = TIMED if name == "timing" else {}
    dev = [[torch.from_numpy(a).to("cuda:0") for a in (o.astype(np.int32), x, z)] for o, x, z in wl.ops]
    torch.cuda.synchronize()
    serial, nbrs = serial_events(wl)
    with World(wl.n, max_spaces=len(wl.space_n), event_capacity=event_capacity,
               cells_per_dist=0.0 if name == "auto" else 3.0) as A:
        enter_all(A, wl)
        for d in dev[:wl.n_warm]:  # the warm-up, serial: every buffer reaches the size the chain needs
            A.moved_batch_device(*(b.data_ptr() for b in d), wl.n)
            A.tick()
        warm = A.debug_counters()
        events, counters = run_chain(A, wl, dev[wl.n_warm:], hooks)
        cl = classify(counters, hooks, wl.flushes)
        bad = compare_events(wl, events, ref, serial)
        end = A.debug_counters()
        print(f"chain {name} cap {event_capacity}: {picture(cl)} | behind a non-fused flush: "
              f"{np.nonzero(cl['behind'])[0].tolist()}, overlapped there: {np.nonzero(cl['behind'] & cl['ovl'])[0].tolist()}"
              f" | regrows warm-up {warm['event_regrows']} chain {end['event_regrows'] - warm['event_regrows']}"
              f" switches in chain {end['cell_size_switches'] - warm['cell_size_switches']}"
              f" cells_per_dist {warm['cells_per_dist']}->{end['cells_per_dist']} | {bad if bad else 'events equal'}")
        assert not bad, "\n".join(bad)
        for i, row in nbrs.items():
            np.testing.assert_array_equal(A.neighbors(i), row, err_msg=f"neighbors({i})")
        # ---- the launches
        spec, incr, ovl, behind, maybe = cl["spec"], cl["incr"], cl["ovl"], cl["behind"], cl["maybe"]
        assert spec[1:].all() and not spec[0], picture(cl)
        assert not (ovl & behind).any(), f"overlapped behind a flush that was not fused: {picture(cl)}"
        assert not (ovl & cl["grew"]).any(), f"overlapped behind a buffer growth: {picture(cl)}"
        if not wl.heavy:
            assert not cl["rerun"].any(), f"a flush of the chain overflowed: {picture(cl)}"
        # every launch as the gated plan decides it (but the one that may have matched a twin set)
        np.testing.assert_array_equal(ovl[~maybe], cl["expect"][~maybe], err_msg=picture(cl))
        lost = ~incr | behind | cl["timed"] | cl["grew"] | ~np.concatenate([[False], cl["mid"][:-1]])
        assert int(ovl[~maybe].sum()) == int((spec & ~lost & ~maybe).sum())
        assert end["overlapped_flushes"] - warm["overlapped_flushes"] == int(ovl.sum())
    return cl, warm, end


@pytest.mark.gpu
@pytest.mark.parametrize("event_capacity", [0, 1024])
def test_chain_grid_rebuilt_by_bbox_gpu(oracle_mod, event_capacity):
    """A scout leaves the crowd at flush 4 (the box leaves the grid) and comes home at flush 9 (the
    grid is more than four times the box): two flushes of the chain take a new grid, launched
    speculatively, with another speculative launch behind each.  Which flushes they are follows
    from when the host learns a flush's boxes (its commit, after the next launch), so the counters
    say it.  event_capacity=1024: in the flushes that first see the new box everyone outside the
    other parity's band trades places, more events than the event sets hold, so a rebuilt flush
    overflows and re-runs its pair passes (every tile, no flags) behind its successor's launch."""
    cl, warm, end = chain_scenario(oracle_mod, "bbox_regrow" if event_capacity else "bbox", event_capacity)
    rebuilt = np.nonzero(~cl["incr"])[0]
    assert rebuilt.size >= 2, picture(cl)
    assert all(cl["spec"][f] and f + 1 < cl["spec"].size and cl["spec"][f + 1] for f in rebuilt), picture(cl)
    if event_capacity:
        assert end["event_regrows"] - warm["event_regrows"] > 0, picture(cl)
        assert (cl["rerun"] & ~cl["incr"]).any() and not (cl["rerun"] & cl["incr"]).any(), picture(cl)


@pytest.mark.gpu
def test_chain_automatic_cell_size_gpu(oracle_mod):
    """cells_per_dist = 0: the crowd thickens along z by 4 % per flush until two commits in a row
    recommend D/3; the flush that rebuilds every grid is launched speculatively in the chain."""
    cl, warm, end = chain_scenario(oracle_mod, "auto")
    assert warm["cells_per_dist"] == 2 and end["cells_per_dist"] == 3
    assert end["cell_size_switches"] - warm["cell_size_switches"] >= 1
    rebuilt = np.nonzero(~cl["incr"])[0]
    assert rebuilt.size >= 1 and all(cl["spec"][f] and f + 1 < cl["spec"].size and cl["spec"][f + 1] for f in rebuilt), picture(cl)


@pytest.mark.gpu
def test_chain_stage_timing_toggled_in_flight_gpu(oracle_mod):
    """gwaoi_set_stage_timing with a flush in flight: flushes 5 and 10 are launched with the special
    pass timed (not fused), the flushes behind them with the mask cleared.  The grid never changes."""
    cl, warm, end = chain_scenario(oracle_mod, "timing")
    assert cl["incr"].all() and cl["timed"].sum() == 2
    assert cl["behind"].sum() == 2 and cl["ovl"].sum() == cl["spec"].sum() - 5, picture(cl)


@pytest.mark.gpu
def test_chain_several_spaces_gpu(oracle_mod):
    """Three spaces: the scout of space 1 gives that space a new grid, which makes the whole flush
    non-incremental; the jumpers, whose leaves are at stake, are in spaces 0 and 2."""
    cl, warm, end = chain_scenario(oracle_mod, "spaces")
    rebuilt = np.nonzero(~cl["incr"])[0]
    assert rebuilt.size >= 2 and all(cl["spec"][f] and f + 1 < cl["spec"].size and cl["spec"][f + 1] for f in rebuilt), picture(cl)
