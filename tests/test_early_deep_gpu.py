"""The deep keygen of an overlapped flush ("Overlapped flushes"): a flush that is
queued beside the previous flush's combined pass (gwaoi_tick_finish(NEXT), FlushPlan::ovl) runs its
keygen in a form that takes more entries per thread than the form of a flush running alone (the
cell scan folds that form's per-block partials).  Sizes around the block sizes of the apply and of
the deep keygen (partial last block, exact block, one entry past it), batches that leave entries unwritten (the virtual-S' restore), dropped ops, a
repeated slot on a claims world (the last call wins) and on a unique-moves world (reported, the
next flush clean), and three spaces so that a block straddles spaces.  Every tick's enter and leave
pairs are compared as sets with the closed form (oracle/closed_form.c), for the chained loop
(overlapped flushes) and for a plain gwaoi_tick_device loop on the same inputs (flushes running
alone: the shallow forms).

Reference: XZListAOIManager.Moved (/root/reference/engine/entity/Space.go:259), one call per move,
the last call of a slot wins; go-aoi itself is absent, so parity is against the restatement
(DESIGN.md §2).
"""
import ctypes as C

import numpy as np
import pytest

from goworld_amd import World, pair_keys
from goworld_amd._lib import GwaoiError

pytestmark = pytest.mark.gpu

ESTATE = -3
NONE = 0xFFFFFFFF  # an op placeholder (a skipped decoded sync record): no op
APPLY_PER, KG_DEEP = 4, 4  # GWAOI_APPLY_PER (the apply kept one form), GWAOI_KG_PER_DEEP (csrc/gwaoi_kernels.hip)
BA, BK = 256 * APPLY_PER, 256 * KG_DEEP
# (8209 = 2 * 4096 + 17: the size of the 16-moves-per-thread apply that was tried and lost, kept as a large case)
SIZES = [1, 255, BK - 1, BK, BK + 1, 2 * BA + 17, 3 * BK + 257, 8209]
D0 = 10.0
TICKS = 8


def _device_events(w, ne, nl):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    e, l = w.events_device()
    out = []
    for ptr, k in ((e, ne), (l, nl)):
        a = np.empty((k, 2), np.uint32)
        if k:
            assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        out.append(a)
    return out


def _scene(n, n_spaces, seed):
    """Base positions (about 8 neighbours each) and the space of every slot; a tick's position is the
    base plus a jitter of at most D/2 per axis, so every grid stays the first flush's."""
    rng = np.random.default_rng(seed)
    Ds = [np.float32(D0 * (1 + 0.5 * s)) for s in range(n_spaces)]
    sp = (np.arange(n) % n_spaces).astype(np.uint32)
    rng.shuffle(sp)
    L = max(4 * D0, 2 * D0 * np.sqrt(n / n_spaces / 8.0))
    base = rng.uniform(0, L, (n, 2)).astype(np.float32)
    return rng, Ds, sp, base


def _batch(rng, base, sp, Ds, slots):
    d = np.array([Ds[s] for s in sp[slots]], np.float32) if slots.size else np.empty(0, np.float32)
    j = rng.uniform(-0.5, 0.5, (slots.size, 2)).astype(np.float32)
    return (slots.astype(np.uint32), (base[slots, 0] + j[:, 0] * d).astype(np.float32),
            (base[slots, 1] + j[:, 1] * d).astype(np.float32))


def _schedule(rng, n, base, sp, Ds, dup_tick):
    """TICKS batches: every entity once; n - 3 moves; two dropped ops; and on dup_tick one slot named twice."""
    out = []
    for t in range(TICKS):
        order = rng.permutation(n)
        if t == 1 and n > 3:
            order = order[:-3]
        sl, x, z = _batch(rng, base, sp, Ds, order)
        if t == 2:  # two placeholders among the ops
            for at in (min(1, sl.size), sl.size // 2 + 1):
                sl = np.insert(sl, at, NONE)
                x = np.insert(x, at, np.float32(1.0))
                z = np.insert(z, at, np.float32(2.0))
        if t == dup_tick:  # one slot a second time, later in the batch
            k = int(rng.integers(0, n))
            v = int(sl[k])
            at = int(rng.integers(k + 1, sl.size + 1))
            sl = np.insert(sl, at, v)
            x = np.insert(x, at, np.float32(x[k] + 0.3 * D0))
            z = np.insert(z, at, np.float32(z[k] - 0.2 * D0))
        out.append((sl.astype(np.uint32), x.astype(np.float32), z.astype(np.float32)))
    return out


def _to_device(torch, batches):
    dev = [[torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (sl.view(np.int32), x, z)]
           for sl, x, z in batches]
    torch.cuda.synchronize()
    return dev


def _populate(w, n, Ds, sp, base, state):
    """Enter every slot at its base position, space by space; the oracle's state follows."""
    x, z, seq, osp = state
    nxt = 1
    for s, D in enumerate(Ds):
        assert w.space_create(float(D)) == s
    for s in range(len(Ds)):
        slots = np.flatnonzero(sp == s).astype(np.uint32)
        if slots.size:
            w.enter_batch(s, slots, base[slots, 0], base[slots, 1])
        x[slots], z[slots] = base[slots, 0], base[slots, 1]
        seq[slots] = nxt + np.arange(slots.size, dtype=np.uint64)
        osp[slots] = s
        nxt += slots.size
    w.tick_device()
    return nxt


def _apply(state, batch, nxt, skip=None):
    """The oracle's state after a batch: the last op of a slot wins; op i takes seq nxt + i (a
    placeholder too).  skip: an op index left out (the repeated slot's other call)."""
    x, z, seq, _ = state
    sl, nx, nz = batch
    keep = sl != NONE
    if skip is not None:
        keep[skip] = False
    i = np.flatnonzero(keep)
    x[sl[i]], z[sl[i]] = nx[i], nz[i]  # (numpy keeps the last of a repeated index)
    seq[sl[i]] = nxt + i.astype(np.uint64)
    return nxt + sl.size


def _run(w, dev, host, chained):
    """The GPU's (enter keys, leave keys) per tick: the chained speculative loop, or one flush at a time."""
    got = []
    if chained:
        w.moved_batch_device(*(b.data_ptr() for b in dev[0]), host[0][0].size)
        w.tick_begin()
    for t in range(len(host)):
        if chained:
            if t + 1 < len(host):
                w.moved_batch_device(*(b.data_ptr() for b in dev[t + 1]), host[t + 1][0].size)
                ne, nl = w.tick_end_begin_device()
            else:
                ne, nl = w.tick_end_device()
        else:
            w.moved_batch_device(*(b.data_ptr() for b in dev[t]), host[t][0].size)
            ne, nl = w.tick_device()
        ge, gl = _device_events(w, ne, nl)
        got.append((pair_keys(ge), pair_keys(gl)))
    return got


def _check_case(oracle_mod, n, unique, n_spaces=1):
    torch = pytest.importorskip("torch")
    O = oracle_mod
    rng, Ds, sp, base = _scene(n, n_spaces, 0xEA51 + 7 * n + n_spaces + (1 if unique else 0))
    host = _schedule(rng, n, base, sp, Ds, dup_tick=-1 if unique else 4)
    dev = _to_device(torch, host)
    Dmap = {s: float(D) for s, D in enumerate(Ds)}
    # the closed form's events per tick, once for both worlds
    state = (np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint64), np.full(n, O.DEAD, np.uint32))
    want = []
    with World(n + 4, max_spaces=n_spaces, unique_moves=unique, device=0) as A, \
            World(n + 4, max_spaces=n_spaces, unique_moves=unique, device=0) as B:
        nxt = _populate(A, n, Ds, sp, base, state)
        _populate(B, n, Ds, sp, base, tuple(a.copy() for a in state))
        for b in host:
            before = tuple(a.copy() for a in state)
            nxt = _apply(state, b, nxt)
            want.append(O.closed_form_diff(before, state, Dmap))
        d0 = A.debug_counters()
        got_a = _run(A, dev, host, chained=True)
        d1 = A.debug_counters()
        b0 = B.debug_counters()
        got_b = _run(B, dev, host, chained=False)
        b1 = B.debug_counters()
    print(f"n={n} unique={unique} spaces={n_spaces}: overlapped {d1['overlapped_flushes'] - d0['overlapped_flushes']} of "
          f"{TICKS} chained flushes, events/tick {[int(e.size + l.size) for e, l in want]}")
    assert d1["overlapped_flushes"] > d0["overlapped_flushes"], (d0, d1)
    assert b1["overlapped_flushes"] == b0["overlapped_flushes"], (b0, b1)
    if unique:
        assert d1["unique_flushes"] - d0["unique_flushes"] == TICKS, (d0, d1)
    for t, (we, wl) in enumerate(want):
        for name, got in (("chained", got_a), ("plain", got_b)):
            np.testing.assert_array_equal(got[t][0], we, err_msg=f"{name} tick {t}: enters")
            np.testing.assert_array_equal(got[t][1], wl, err_msg=f"{name} tick {t}: leaves")
    if n >= 255:
        assert sum(e.size + l.size for e, l in want) > 0


@pytest.mark.parametrize("unique", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_deep_early_kernels_match_closed_form_gpu(oracle_mod, n, unique):
    _check_case(oracle_mod, n, unique)


def test_deep_early_kernels_three_spaces_gpu(oracle_mod):
    """Three spaces of different D: S' is in cell order, space after space, so blocks straddle spaces."""
    _check_case(oracle_mod, 3 * BK + 257, True, n_spaces=3)


def test_deep_unique_repeated_slot_is_reported_gpu(oracle_mod):
    """A unique-moves world in the chained loop, one batch naming a slot twice (n = BK + 1, so the
    count spans keygen blocks): that flush reports GWAOI_ESTATE (ERR_DUP_SLOT) and commits with one of
    the slot's two positions; the flushes after it report nothing and match the closed form."""
    torch = pytest.importorskip("torch")
    O = oracle_mod
    n, dup = BK + 1, 3
    rng, Ds, sp, base = _scene(n, 1, 0xD0B1)
    host = _schedule(rng, n, base, sp, Ds, dup_tick=dup)
    dev = _to_device(torch, host)
    Dmap = {0: float(Ds[0])}
    sl = host[dup][0]
    v = [int(s) for s in sl if s != NONE and np.count_nonzero(sl == s) == 2][0]
    calls = np.flatnonzero(sl == v)
    state = (np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint64), np.full(n, O.DEAD, np.uint32))
    with World(n + 4, unique_moves=True, device=0) as w:
        nxt = _populate(w, n, Ds, sp, base, state)
        d0 = w.debug_counters()
        w.moved_batch_device(*(b.data_ptr() for b in dev[0]), host[0][0].size)
        w.tick_begin()
        states = [state]  # the states the frame may hold: two after the repeated slot's flush
        for t in range(TICKS):
            if t + 1 < TICKS:
                w.moved_batch_device(*(b.data_ptr() for b in dev[t + 1]), host[t + 1][0].size)
            fin = w.tick_end_begin_device if t + 1 < TICKS else w.tick_end_device
            if t == dup:
                with pytest.raises(GwaoiError) as ei:
                    fin()
                assert ei.value.code == ESTATE and "UNIQUE" in str(ei.value), str(ei.value)
                ne, nl = ei.value.counts
            else:
                ne, nl = fin()  # (a stale error word or drop count would raise here)
            ge, gl = _device_events(w, ne, nl)
            ge, gl = pair_keys(ge), pair_keys(gl)
            nexts = []
            for st in states:
                for skip in (calls if t == dup else [None]):
                    after = tuple(a.copy() for a in st)
                    _apply(after, host[t], nxt, skip=skip)
                    we, wl = O.closed_form_diff(st, after, Dmap)
                    if np.array_equal(ge, we) and np.array_equal(gl, wl):
                        nexts.append(after)
            assert nexts, f"tick {t}: the events match no state the frame may hold"
            states = nexts
            nxt += host[t][0].size
        d1 = w.debug_counters()
        assert d1["overlapped_flushes"] > d0["overlapped_flushes"], (d0, d1)
        assert d1["unique_flushes"] - d0["unique_flushes"] == TICKS, (d0, d1)
