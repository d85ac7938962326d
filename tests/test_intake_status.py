"""The op intake's statuses that no other test reaches: what gwaoi_moved_batch_stage / _commit /
_pinned and the host batch calls return around an open reservation, a launch that takes the
reserved half, a full staging half, and calls made while a flush is in flight (the deferred
path with the space column and deferred boxes).

One world of 256 slots, one space, 200 entities entered and flushed once; batches of 64 moves
(kStageMin, the smallest batch that is staged).  Every case asserts GwaoiError.code; where a
call succeeds, the events of the following tick() are those of a twin world driven through
plain moved_batch / enter / leave in the same order."""
import numpy as np
import pytest

from goworld_amd import World, pair_keys
from goworld_amd._lib import GwaoiError

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ENONFINITE, ECAPACITY = -1, -3, -6, -9
SLOTS, N, K, D, SIDE = 256, 200, 64, 10.0, 100.0


class Twins:
    """World A (the calls under test) and its twin B (plain calls), both entered and flushed once."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.A, self.B = World(SLOTS), World(SLOTS)
        x0, z0 = self.pos(N)
        for w in (self.A, self.B):
            assert w.space_create(D) == 0
            w.enter_batch(0, np.arange(N, dtype=np.uint32), x0, z0)
            w.tick()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.close()
        self.B.close()

    def pos(self, n):
        return (self.rng.uniform(0, SIDE, n).astype(np.float32), self.rng.uniform(0, SIDE, n).astype(np.float32))

    def batch(self, n=K, without=()):
        """n moves of live slots (repeats allowed), none of `without`."""
        live = np.setdiff1d(np.arange(N, dtype=np.uint32), np.asarray(without, np.uint32))
        return (self.rng.choice(live, n).astype(np.uint32), *self.pos(n))

    def stage_commit(self, b, reserve=None):
        views = self.A.stage_moves(reserve or b[0].size)
        for v, src in zip(views, b):
            v[:b[0].size] = src
        self.A.commit_moves(b[0].size)

    def same_events(self, ev_a, ev_b, what=""):
        for a, b, kind in zip(ev_a, ev_b, ("enter", "leave")):
            np.testing.assert_array_equal(pair_keys(a), pair_keys(b), err_msg=f"{what} {kind} events")
        return len(ev_a[0]) + len(ev_a[1])

    def ticks_match(self, what=""):
        return self.same_events(self.A.tick(), self.B.tick(), what)


def code_of(call, *args):
    with pytest.raises(GwaoiError) as ei:
        call(*args)
    return ei.value.code


def no_events(ev):
    return len(ev[0]) == 0 and len(ev[1]) == 0


def test_one_reservation_and_a_bad_commit_closes_it():
    """1. A second _stage without a commit is GWAOI_ESTATE; a commit of more than was reserved is
    GWAOI_EINVAL and the reservation is gone: a further commit is GWAOI_ESTATE."""
    with Twins(1) as t:
        t.A.stage_moves(K)
        assert code_of(t.A.stage_moves, K) == ESTATE
        assert code_of(t.A.commit_moves, K + 1) == EINVAL
        assert code_of(t.A.commit_moves, 1) == ESTATE
        assert no_events(t.A.tick())
        b = t.batch()  # staging works again
        t.stage_commit(b)
        t.B.moved_batch(*b)
        assert t.ticks_match("after the closed reservation") > 0


def test_launch_takes_the_reserved_half():
    """2. _stage, gwaoi_tick_begin, _commit: GWAOI_ESTATE (the launch took that half).  The flush
    ends with no events and the next staged batch works."""
    with Twins(2) as t:
        t.A.stage_moves(K)
        t.A.tick_begin()
        assert code_of(t.A.commit_moves, K) == ESTATE
        assert no_events(t.A.tick_end())
        b = t.batch()
        t.stage_commit(b)
        t.B.moved_batch(*b)
        assert t.ticks_match("after the void reservation") > 0


def test_second_launch_brings_the_reserved_half_back():
    """After _stage and two launches the reserved half is current again: a _commit made while the
    second flush is in flight queues the caller's moves for the flush after it."""
    with Twins(7) as t:
        b = t.batch()
        for v, src in zip(t.A.stage_moves(K), b):
            v[:] = src
        t.A.tick_begin()
        assert no_events(t.A.tick_end())
        t.A.tick_begin()
        t.A.commit_moves(K)
        assert no_events(t.A.tick_end())
        t.B.moved_batch(*b)
        assert t.ticks_match("the commit after two launches") > 0


def test_full_half_refuses_a_bigger_reservation():
    """3. After a committed batch of 64, a reservation of 70,000 moves in the same flush is
    GWAOI_ECAPACITY: the first allocation is 4 << 16 words and a half that holds a queued batch
    may not move.  The first batch still flushes correctly."""
    with Twins(3) as t:
        b = t.batch()
        t.stage_commit(b)
        assert code_of(t.A.stage_moves, 70000) == ECAPACITY
        t.B.moved_batch(*b)
        assert t.ticks_match("the batch before the refused reservation") > 0


def test_open_reservation_blocks_other_staging():
    """4. With a reservation open, gwaoi_moved_batch of 64 queues as host ops ahead of the later
    commit, and gwaoi_moved_batch_pinned of 64 is GWAOI_ESTATE."""
    with Twins(4) as t:
        first, second = t.batch(), t.batch()
        views = t.A.stage_moves(K)
        for v, src in zip(views, first):
            v[:] = src
        t.A.moved_batch(*second)
        ptr, pinned = t.A.pinned_batch(K)
        for v, src in zip(pinned, t.batch()):
            v[:] = src
        assert code_of(t.A.moved_batch_pinned, pinned, K) == ESTATE
        t.A.commit_moves(K)
        t.B.moved_batch(*second)
        t.B.moved_batch(*first)
        assert t.ticks_match("host ops ahead of the commit") > 0
        t.A.free_pinned_batch(ptr)


def test_calls_in_flight_join_the_next_flush():
    """5. While a flush is in flight: enter, a staged moved_batch of 64 that includes the slot
    just entered, leave of another slot, moved of a third, _stage / _commit of 64.  After
    tick_end and one more tick the events are the twin's, which made the same calls after its
    tick (deferred ops, the space column, deferred boxes)."""
    with Twins(5) as t:
        before = t.batch()
        ex, ez = t.pos(1)
        mx, mz = t.pos(1)
        b1 = t.batch()
        b1[0][10] = N  # the slot entered in flight
        b2 = t.batch(without=[5])  # slot 5 leaves in between
        t.A.moved_batch(*before)
        t.A.tick_begin()
        t.A.enter(0, N, ex[0], ez[0])
        t.A.moved_batch(*b1)
        t.A.leave(5)
        t.A.moved(7, mx[0], mz[0])
        t.stage_commit(b2)
        ev_a = t.A.tick_end()
        t.B.moved_batch(*before)
        assert t.same_events(ev_a, t.B.tick(), "the flush in flight") > 0
        t.B.enter(0, N, ex[0], ez[0])
        t.B.moved_batch(*b1)
        t.B.leave(5)
        t.B.moved(7, mx[0], mz[0])
        t.B.moved_batch(*b2)
        assert t.ticks_match("the calls made in flight") > 0


def test_bad_batches_queue_nothing():
    """6. gwaoi_enter_batch with a duplicate slot, gwaoi_leave_batch with a dead slot and a
    gwaoi_moved_batch of 10 (host-op fallback) with a NaN in its last element each return the
    status of the per-slot call for that element and queue nothing: the next tick has no events."""
    with Twins(6) as t:
        A = t.A
        x, z = t.pos(3)
        assert code_of(A.enter_batch, 0, np.array([N + 10, N + 11, N + 10], np.uint32), x, z) == ESTATE
        assert no_events(A.tick())
        assert code_of(A.leave_batch, np.array([3, N + 50], np.uint32)) == ESTATE
        assert no_events(A.tick())
        sl, x, z = t.batch(10)
        z[9] = np.nan
        assert code_of(A.moved_batch, sl, x, z) == ENONFINITE
        assert no_events(A.tick())
        # the world is as it was: the same batch without the NaN gives the twin's events
        z[9] = 1.0
        A.moved_batch(sl, x, z)
        t.B.moved_batch(sl, x, z)
        assert t.ticks_match("after the refused batches") > 0
