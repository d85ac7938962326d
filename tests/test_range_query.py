"""Range reads on the GPU (include/gwaoi_sync.h, "range reads"): the entities within a caller-chosen
radius of an entity or of a point (gwaoi_range_batch, gwaoi_range_count_batch and their device
forms) -- Monster.attack for everyone inside GetAttackRange (Monster.go:72,108,143-151), an aggro
radius, a trigger zone about a point, a count of players within r.

The model is built here over the sequential restatement (oracle/entity_sync.py) driven by
tests/sync_scenario.py: a brute force over the entities with e.aoi and e.space == the query's
space, the sum in numpy float32 step by step, the distance np.float32(np.sqrt(np.float64(d2))) and
the test d <= np.float32(r).  Items are compared as sorted sets, distances bit for bit after sorting
by slot.
"""
import functools

import numpy as np
import pytest

import sync_scenario as SS
from oracle.entity_sync import GameEntities, records_by_gate
from test_broadcast import _d2h  # device memory to host through the HIP runtime the process loaded
from test_interest_query import EID, scenario_tags

from goworld_amd import RANGE_PLANAR, RANGE_POINT, RANGE_QUERY

F32 = np.float32
RADII = [0, 3, 25, 60, 100, 250, 2000]


# --------------------------------------------------------------- model ------

def frame_of(g):
    """{space: (slots, x, y, z)} of the entities in the frame: e.aoi and e.space == space."""
    by = {}
    for e in g.by_slot.values():
        if e.aoi:
            by.setdefault(e.space, []).append(e)
    return {sp: (np.array([e.slot for e in v], np.uint32), np.array([e.x for e in v], F32),
                 np.array([e.y for e in v], F32), np.array([e.z for e in v], F32)) for sp, v in by.items()}


def range_model(g, q, tags):
    """[(slots sorted, their distances)] per query; an exact-boundary count (d == r) beside it."""
    fr = frame_of(g)
    tags = np.asarray(tags, np.uint32)
    rows, on_rim = [], 0
    none = (np.empty(0, np.uint32), np.empty(0, F32))
    for x in q:
        center, fl = int(x["center"]), int(x["flags"])
        if fl & RANGE_POINT:
            sp, c, me = center, (F32(x["x"]), F32(x["y"]), F32(x["z"])), None
        else:
            e = g.by_slot.get(center)
            if e is None or not e.aoi:
                rows.append(none)
                continue
            sp, c, me = e.space, (F32(e.x), F32(e.y), F32(e.z)), center
        if sp not in fr:
            rows.append(none)
            continue
        s, bx, by, bz = fr[sp]
        with np.errstate(over="ignore", under="ignore"):
            dx, dy, dz = bx - c[0], by - c[1], bz - c[2]  # float32 arrays: every step rounds to float32
            d2 = (dx * dx + dz * dz) if fl & RANGE_PLANAR else ((dx * dx + dy * dy) + dz * dz)
            assert d2.dtype == np.float32
            d = np.sqrt(d2.astype(np.float64)).astype(np.float32)
        hit = (d <= F32(x["radius"])) & ((tags[s] & np.uint32(x["mask"])) == np.uint32(x["want"]))
        if me is not None:
            hit &= s != me
        on_rim += int((hit & (d == F32(x["radius"]))).sum())
        o = np.argsort(s[hit])
        rows.append((s[hit][o], d[hit][o]))
    return rows, on_rim


def flat(rows):
    """(offsets, items, dists) of model rows."""
    off = np.zeros(len(rows) + 1, np.uint32)
    off[1:] = np.cumsum([r[0].size for r in rows])
    if not off[-1]:
        return off, np.empty(0, np.uint32), np.empty(0, F32)
    return off, np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])


def same_rows(got, rows):
    """A library answer (offsets, items, dists) against model rows: the offsets, every row's set of
    slots, and every distance bit for bit (rows sorted by slot)."""
    off, items, dists = got
    eoff, eitems, edists = flat(rows)
    if not np.array_equal(off, eoff) or items.size != off[-1] or dists.size != off[-1]:
        return False
    rid = np.repeat(np.arange(len(rows)), np.diff(off.astype(np.int64)))
    o = np.lexsort((items, rid))
    return (np.array_equal(items[o], eitems) and
            np.array_equal(dists[o].view(np.uint32), edists.view(np.uint32)))


def queries(centers, radii, **kw):
    from goworld_amd import World
    return World.range_queries(centers, radii, **kw)


# ------------------------------------------------------------------ CPU ------

def test_library_entry_points_validate_without_a_gpu():
    from goworld_amd import World, _lib, build
    build.build()
    L = _lib.load()
    assert L.gwaoi_range_batch(None, None, 0, None) == -1
    assert L.gwaoi_range_batch_device(None, None, 0, None) == -1
    assert L.gwaoi_range_count_batch(None, None, 0, None) == -1
    assert L.gwaoi_range_count_batch_device(None, None, 0, None) == -1
    assert RANGE_QUERY.itemsize == 32 and (RANGE_POINT, RANGE_PLANAR) == (1, 2) == (World.RANGE_POINT, World.RANGE_PLANAR)
    assert [RANGE_QUERY.fields[k][1] for k in ("center", "flags", "x", "y", "z", "radius", "mask", "want")] == \
        [0, 4, 8, 12, 16, 20, 24, 28]
    q = World.range_queries([3, 4], 2.5, masks=9, points=[[1, 2, 3], [4, 5, 6]], planar=[False, True])
    assert q.dtype == RANGE_QUERY and q["flags"].tolist() == [1, 3] and q["radius"].tolist() == [2.5, 2.5]
    assert q["y"].tolist() == [2.0, 5.0] and q["mask"].tolist() == [9, 9] == q["want"].tolist()
    q = World.range_queries([7], [1.0])
    assert q["flags"].tolist() == [0] and q["mask"].tolist() == [0] and q["center"].tolist() == [7]


def small_world():
    """Entity 0 at the origin, 1 at (3, 0, 4), 2 at (3, 12, 4), 3 at the origin too, in one AOI space
    with D = 1: InterestedIn pairs 0 with 3 and 1 with 2 (same x and z) and nobody else."""
    g = GameEntities({0: 1.0}, 8)
    for i, (x, y, z) in enumerate([(0, 0, 0), (3, 0, 4), (3, 12, 4), (0, 0, 0)]):
        g.create(EID[i], i, x, y, z, 0.0)
        g.enter_space(i, 0, x, y, z)
    return g


def test_expected_answers_on_the_small_world():
    g = small_world()
    tags = np.array([1, 1, 1, 2, 0, 0, 0, 0], np.uint32)
    below5 = np.nextafter(F32(5), F32(0))

    def ask(q):
        rows, _ = range_model(g, q, tags)
        return [(r[0].tolist(), r[1].tolist()) for r in rows]

    # the 3-4-5 triangle: inclusive at 5, not at the float below it; 0 is never in its own row
    assert ask(queries([0, 0], [5.0, below5])) == [([1, 3], [5.0, 0.0]), ([3], [0.0])]
    # (3, 12, 4) is 13 away: a hit at 13, and at 5 once dy is dropped
    assert ask(queries([0, 0], [13.0, np.nextafter(F32(13), F32(0))])) == [([1, 2, 3], [5.0, 13.0, 0.0]), ([1, 3], [5.0, 0.0])]
    assert ask(queries([0], [5.0], planar=True)) == [([1, 2, 3], [5.0, 5.0, 0.0])]
    # a point on an entity includes it
    assert ask(queries([0], [0.0], points=[[0, 0, 0]])) == [([0, 3], [0.0, 0.0])]
    assert ask(queries([0], [5.0], points=[[3, 0, 4]])) == [([0, 1, 3], [5.0, 0.0, 5.0])]
    # the filter: tag 2 only; mask 0 with want != 0 finds nobody
    assert ask(queries([1, 1], [13.0, 13.0], masks=[2, 0], wants=[2, 1])) == [([3], [5.0]), ([], [])]
    # InterestedIn (D = 1, x and z only) holds none of the pairs 5 or 13 apart
    assert g.by_slot[0].In == {3} and g.by_slot[1].In == {2}


def scenario_range_queries(i, sc, g=None):
    """The 200 queries after flush i."""
    rng = np.random.default_rng(5000 + i)
    n = sc["n"]
    q = np.zeros(200, RANGE_QUERY)
    for m in range(200):
        q[m]["radius"] = RADII[m % 7]
        fl = (RANGE_PLANAR if (m // 7) % 2 else 0) | (RANGE_POINT if (m // 14) % 2 else 0)
        q[m]["flags"] = fl
        if fl & RANGE_POINT:
            q[m]["center"] = rng.integers(0, 2)
            q[m]["x"], q[m]["y"], q[m]["z"] = rng.uniform(-400, 400), rng.uniform(0, 10), rng.uniform(-400, 400)
        else:
            q[m]["center"] = rng.integers(0, n + 8)  # (the last 8 were never bound)
        q[m]["mask"] = q[m]["want"] = 9 if m % 3 == 0 else 0
    return q


def row_stats(g, q, rows, on_rim):
    slot_q = [(x, r) for x, r in zip(q, rows) if not x["flags"] & RANGE_POINT]
    return {
        "in_frame": sum(1 for x in q if x["flags"] & RANGE_POINT or
                        (int(x["center"]) in g.by_slot and g.by_slot[int(x["center"])].aoi)),
        "empty": sum(1 for r in rows if r[0].size == 0),
        "items": sum(r[0].size for r in rows),
        "longest": max(r[0].size for r in rows),
        "beyond_aoi": sum(sum(1 for b in r[0].tolist() if b not in g.by_slot[int(x["center"])].In) for x, r in slot_q),
        "point_items": sum(r[0].size for x, r in zip(q, rows) if x["flags"] & RANGE_POINT),
        "planar_items": sum(r[0].size for x, r in zip(q, rows) if x["flags"] & RANGE_PLANAR),
        "filtered_items": sum(r[0].size for x, r in zip(q, rows) if x["mask"]),
        "spaces": sorted({int(x["center"]) for x in q if x["flags"] & RANGE_POINT}),
        "on_rim": on_rim,
    }


@functools.lru_cache(maxsize=None)
def scenario_expected():
    """The scenario and, per flush, the queries, the model rows, the sync collect and the class counts
    (computed once on the restatement, shared and left unchanged by the tests)."""
    sc = SS.make(seed=21, n=600, flushes=4)
    tags = scenario_tags(sc["n"])
    exp = []

    def on_flush(i, g):
        q = scenario_range_queries(i, sc)
        rows, on_rim = range_model(g, q, tags)
        exp.append({"q": q, "rows": rows, "stats": row_stats(g, q, rows, on_rim), "sync": g.collect()})

    SS.run_oracle(sc, on_flush)
    return sc, tags, exp


def test_scenario_covers_every_class_of_query():
    """Checked on the restatement (no GPU): at every flush the draw has centres outside the frame,
    empty rows, rows longer than two groups of 128 candidates, point and planar and filtered queries
    with items, both spaces, and thousands of items that the centre's InterestedIn does not hold, so
    a scenario change cannot hollow the GPU test out.  The bounds are this model's own figures."""
    sc, tags, exp = scenario_expected()
    assert len(exp) == len(sc["flushes"]) + 1 == 5
    for e in exp:
        st = e["stats"]
        print(st)
        assert 190 <= st["in_frame"] <= 195
        assert 80 <= st["empty"] <= 86
        assert 6964 <= st["items"] <= 7738
        assert 279 <= st["longest"] <= 280  # (more than two groups of 128 candidates)
        assert 2777 <= st["beyond_aoi"] <= 3434
        assert 3661 <= st["point_items"] <= 4101 and 3416 <= st["planar_items"] <= 3764
        assert 888 <= st["filtered_items"] <= 978
        assert st["spaces"] == [0, 1]
        assert st["on_rim"] == 0  # (no drawn hit has d == r: the boundary gets hand-built cases)


# ------------------------------------------------------------------ GPU ------

def _dev_q(q):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(q, RANGE_QUERY).view(np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def device_range(w, q):
    """range_batch_device on a torch tensor -> (offsets, items, dists), read back from the pointers."""
    dq = _dev_q(q)
    op, ip, dp, k = w.range_batch_device(dq.data_ptr() if q.size else 0, q.size)
    off = np.frombuffer(_d2h(op, 4 * (q.size + 1)), np.uint32)
    assert off[-1] == k
    return off, np.frombuffer(_d2h(ip, 4 * k), np.uint32), np.frombuffer(_d2h(dp, 4 * k), np.float32)


def device_count(w, q):
    import torch
    dq = _dev_q(q)
    out = torch.full((q.size,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    w.range_count_batch_device(dq.data_ptr(), q.size, out.data_ptr())
    return out.cpu().numpy().view(np.uint32)


def check_all_forms(w, q, rows, what=""):
    """Host form, device form, count form and device count form against the model; the host and
    device items in the same order.  Returns the host answer."""
    counts = np.array([r[0].size for r in rows], np.uint32)
    got = w.range_batch(q)
    assert same_rows(got, rows), f"{what}: host form"
    dgot = device_range(w, q)
    assert same_rows(dgot, rows), f"{what}: device form"
    assert np.array_equal(dgot[1], got[1]) and np.array_equal(dgot[2].view(np.uint32), got[2].view(np.uint32)), \
        f"{what}: host and device rows differ in order"
    assert np.array_equal(w.range_count_batch(q), counts), f"{what}: count form"
    if q.size:
        assert np.array_equal(device_count(w, q), counts), f"{what}: device count form"
    return got


@pytest.mark.gpu
def test_range_queries_scenario_matches_oracle():
    """After every flush: the four forms against the model, a second call identical, and then the
    sync collect still equals the restatement's (the queries changed nothing)."""
    from goworld_amd import World
    sc, tags, exp = scenario_expected()
    n = sc["n"]
    seen = []

    def on_flush(i, w, ent=None, lev=None):
        if i == 0:
            w.entity_set_tag(np.arange(n + 8), tags)
        e = exp[i]
        got = check_all_forms(w, e["q"], e["rows"], f"flush {i}")
        again = w.range_batch(e["q"])
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again)), \
            f"flush {i}: a second call differs"
        assert records_by_gate(w.collect_sync_infos()) == e["sync"], f"flush {i}: sync records after the queries"
        seen.append(int(got[0][-1]))

    with World(n + 8, max_spaces=4, device=0) as w:
        SS.run_gpu(sc, w, on_flush)  # (the scenario's spaces 0 and 1 are the world's first two ids)
    assert seen == [e["stats"]["items"] for e in exp] and min(seen) > 0


@pytest.mark.gpu
def test_range_queries_dense_crowd_regrows_rows():
    """Everyone within reach of everyone (a 60 x 60 square, r = 2000): rows of about 290, longer than
    two groups of 128 candidates.  A 1-query call first, then every slot plus 64 copies of one (more
    than 100,000 items): the write pass, queued with the small call's outputs, declines; items and
    dists regrow together and the relaunch matches."""
    from goworld_amd import World
    sc = SS.make(seed=23, n=600, n_outside=20, flushes=2, L=60.0)
    n = sc["n"]
    left = {op[1] for ops in sc["flushes"] for op in ops if op[0] == "leave"}
    hot = next(op[1] for op in sc["setup"] if op[0] == "enter" and op[1] not in left)  # in a space throughout
    tags = scenario_tags(n)[:n]
    q = queries(np.concatenate([np.arange(n), np.full(64, hot)]), 2000.0)
    drawn = [scenario_range_queries(i, sc) for i in range(3)]
    exp = []

    def oracle_flush(i, g):
        exp.append((range_model(g, q, tags)[0], range_model(g, drawn[i], tags)[0]))

    SS.run_oracle(sc, oracle_flush)
    for rows, drows in exp:
        assert 289 <= max(r[0].size for r in rows) <= 290 and sum(r[0].size for r in rows) > 100_000
        assert 290 <= max(r[0].size for r in drows) <= 291 and 16_943 <= sum(r[0].size for r in drows) <= 17_538

    def on_flush(i, w, ent=None, lev=None):
        if i == 0:
            w.entity_set_tag(np.arange(n), tags)
            assert same_rows(w.range_batch(q[:1]), exp[0][0][:1])
            assert same_rows(w.range_batch(q), exp[0][0]), "the regrown relaunch"
            assert same_rows(device_range(w, q[:1]), exp[0][0][:1])
        check_all_forms(w, q, exp[i][0], f"flush {i}")
        check_all_forms(w, drawn[i], exp[i][1], f"flush {i}, drawn")

    with World(n + 8, max_spaces=4, device=0) as w:  # (the drawn centres include 8 slots never bound)
        SS.run_gpu(sc, w, on_flush)


@pytest.mark.gpu
def test_range_queries_tall_window():
    """A window of more than 64, and of more than 128, grid rows: one space with D = 3 and 6,000
    entities over 400 x 400 (a grid may have four cells per entity, so a 300-entity world cannot have
    129 rows; the corners are occupied, so the grid is square and total_cells > 128^2 means more than
    128 rows).  r = 0.5, 50, 150 and 1000, slot-centred and about points, against the model."""
    from goworld_amd import World
    n = 6000
    rng = np.random.default_rng(77)
    pos = rng.uniform(-200, 200, (n, 3)).astype(np.float32)
    pos[:, 1] = rng.uniform(0, 10, n)
    pos[:4, 0], pos[:4, 2] = [-200, -200, 200, 200], [-200, 200, -200, 200]
    g = GameEntities({0: 3.0}, n)
    tags = np.zeros(n, np.uint32)
    with World(n, device=0) as w:
        sp = w.space_create(3.0)
        w.enter_batch(sp, np.arange(n), pos[:, 0], pos[:, 2])
        for s in range(n):
            g.create(s.to_bytes(16, "little"), s, *pos[s], 0.0)
            g.enter_space(s, 0, *pos[s])
        # y through the sync layer's position record (x and z are the frame's)
        for s in range(0, n, 7):
            w.entity_set_position_yaw(s, *pos[s], 0.0)
        for s in range(n):
            if s % 7:
                g.by_slot[s].y = F32(0)
        w.tick()
        assert w.info()["total_cells"] > 128 * 128
        cs = rng.integers(0, n, 6)
        pts = np.concatenate([rng.uniform(-220, 220, (5, 3)), [[0, 0, 0]]]).astype(np.float32)
        pts[:, 1] = rng.uniform(0, 10, 6)
        for r in (0.5, 50.0, 150.0, 1000.0):
            q = np.concatenate([queries(cs, r), queries(np.zeros(6), r, points=pts),
                                queries(cs[:2], r, planar=True)])
            rows, _ = range_model(g, q, tags)
            check_all_forms(w, q, rows, f"r = {r}")
            if r >= 150.0:
                assert min(x[0].size for x in rows) > 100
        assert rows[0][0].size == n - 1 and rows[6][0].size == n


def edge_world(w, g):
    """Two AOI spaces (D = 6: cells of 2 or 3, so multiples of 1 are cell boundaries for either
    automatic cell size) holding the same coordinates, and one space without AOI."""
    pts = [
        (0, 0, 0), (3, 0, 4), (3, 12, 4), (0, 0, 0), (0, -0.0, 0),       # 0-4: the 3-4-5 cases, co-located, y = -0.0
        (1e-22, 0, 0), (1e-23, 0, 0), (0, 0, -1e-22), (0, 1e-23, 0),     # 5-8: offsets whose squares underflow
        (64, 0, 0), (np.nextafter(F32(64), F32(65)), 0, 0), (64, 1e-22, 1e-23),  # 9-11: the same about x = 64
        (1, 0, 1), (2, 0, 3), (6, 0, 6), (-6, 0, 12), (5, 0, 0), (-5, 0, 0), (0, 0, 5), (0, 0, -5),  # 12-19: on multiples of D/6
    ]
    slot = 0
    for sp in (0, 1):
        for p in pts:
            p = tuple(F32(v) for v in p)
            g.create(slot.to_bytes(16, "little"), slot, *p, 0.0)
            g.enter_space(slot, sp, *p)
            w.entity_bind([slot], [slot.to_bytes(16, "little")])
            w.entity_set_position_yaw(slot, *p, 0.0)
            w.enter(sp, slot, p[0], p[2])
            slot += 1
    # one in the space without AOI, one bound and never in a space (nilSpace)
    for k, plain in ((slot, True), (slot + 1, False)):
        g.create(k.to_bytes(16, "little"), k, 1.0, 0.0, 1.0, 0.0)
        w.entity_bind([k], [k.to_bytes(16, "little")])
        w.entity_set_position_yaw(k, 1.0, 0.0, 1.0, 0.0)
        if plain:
            g.enter_plain_space(k, 9, 1.0, 0.0, 1.0)
            w.entity_enter_plain(k, 1.0, 0.0, 1.0)
    return len(pts)


@pytest.mark.gpu
def test_range_queries_arithmetic_and_geometry_edges():
    from goworld_amd import World
    g = GameEntities({0: 6.0, 1: 6.0}, 64)
    tags = np.zeros(64, np.uint32)
    below5 = np.nextafter(F32(5), F32(0))
    with World(64, max_spaces=4, device=0) as w:
        assert [w.space_create(6.0), w.space_create(6.0)] == [0, 1]
        k = edge_world(w, g)
        empty_space = w.space_create(10.0)  # created, nobody ever enters
        w.tick()
        every = np.arange(2 * k + 2)
        qs = [
            queries([0, 0, 0, 0, 1, k], [5.0, below5, 13.0, np.nextafter(F32(13), F32(0)), 5.0, 5.0]),  # 3-4-5, 13
            queries([0, k + 2], 5.0, planar=True),
            queries(every, 0.0),                          # r = 0: the co-located ones and the underflowing offsets
            queries(every, 0.0, planar=True),
            queries(every, 1e-22), queries(every, F32(64) * F32(2.0 ** -23)),
            queries(every, 3e38), queries(every, 3e38, planar=True),
            queries(every, 1.0),
            queries(np.repeat(every, 3), np.tile([5.0, 6.0, np.sqrt(F32(72.0))], every.size)),
            # points: on entities, on cell boundaries, 1e6 outside the grid with r = 1 and r = 3e6, both spaces
            queries([0, 1, 0, 1], 0.0, points=[[0, 0, 0]] * 2 + [[64, 0, 0]] * 2),
            queries([0, 1] * 4, [1.0, 1.0, 3e6, 3e6] * 2, points=[[1e6, 0, 0]] * 4 + [[0, 0, -1e6]] * 4),
            queries([0] * 6, [0.0, 1.0, 2.0, 3.0, 6.0, 5.0], points=[[1, 0, 1], [2, 0, 2], [3, 0, 3], [0, 0, 6], [-6, 0, 6], [0, 0, 0]]),
            queries([1, 1], [1e-22, 5.0], points=[[1e-23, -0.0, 0], [0, 0, 0]], planar=[False, True]),
            queries([empty_space, empty_space], [0.0, 3e38], points=[[0, 0, 0]] * 2),  # a created space that is empty
        ]
        for j, q in enumerate(qs):
            rows, _ = range_model(g, q, tags)
            check_all_forms(w, q, rows, f"edge set {j}")
        # what the model itself says about the hand-checked ones
        rows = range_model(g, qs[0], tags)[0]
        assert 1 in rows[0][0] and 1 not in rows[1][0] and 2 in rows[2][0] and 2 not in rows[3][0]
        assert 0 not in rows[0][0] and {3, 4} <= set(rows[1][0].tolist())
        assert all(r[0].size and r[0].max() < k for r in rows[:5]) and rows[5][0].min() >= k  # only the query's space answers
        assert 2 in range_model(g, qs[1], tags)[0][0][0]
        r0 = range_model(g, qs[2], tags)[0]
        assert set(r0[0][0].tolist()) == {3, 4, 6, 8} and 5 not in r0[0][0]  # fl32(1e-23^2) = 0, fl32(1e-22^2) > 0
        assert r0[2 * k][0].size == 0 and r0[2 * k + 1][0].size == 0  # the space without AOI, nilSpace
        far = range_model(g, qs[11], tags)[0]
        assert far[0][0].size == 0 and far[2][0].size == k and far[6][0].size == k
        assert all(r[0].size == 0 for r in range_model(g, qs[14], tags)[0])
        # a world whose every entity has left: the frame is empty
        for s in range(2 * k):
            w.leave(s)
            g.leave_space(s)
        w.entity_leave_plain(2 * k)
        g.leave_space(2 * k)
        w.tick()
        q = np.concatenate([queries(every[:8], 3e38), queries([0, 1, empty_space], 3e38, points=[[0, 0, 0]] * 3)])
        rows, _ = range_model(g, q, tags)
        assert all(r[0].size == 0 for r in rows)
        check_all_forms(w, q, rows, "empty frame")


@pytest.mark.gpu
def test_range_queries_after_a_sparse_flush():
    """A flush of a few host Moved calls on a large world takes the sparse path, which patches the
    frame in place (also a move across many cells); the range reads then answer from that frame."""
    from goworld_amd import World
    n = 30000
    rng = np.random.default_rng(91)
    L = 2500.0
    x = rng.uniform(0, L, n).astype(np.float32)
    z = rng.uniform(0, L, n).astype(np.float32)
    g = GameEntities({0: 25.0}, n)
    tags = np.zeros(n, np.uint32)
    with World(n, device=0) as w:
        sp = w.space_create(25.0)
        w.enter_batch(sp, np.arange(n), x, z)
        w.tick()
        w.range_batch(queries([0], 1.0))  # (creates the sync layer before the sparse flush)
        movers = [5, 17, 4000, 29999]
        step = [(0.5, -0.5), (30.0, 0.0), (60.0, -45.0), (-1.0, 20.0)]  # within a cell, across one, across several
        for s, (ddx, ddz) in zip(movers, step):
            x[s], z[s] = np.clip(x[s] + F32(ddx), 0, L), np.clip(z[s] + F32(ddz), 0, L)
        s0 = w.debug_counters()["sparse_flushes"]
        for s in movers:
            w.moved(s, x[s], z[s])
        w.tick()
        assert w.debug_counters()["sparse_flushes"] == s0 + 1
        for s in range(n):
            g.create(s.to_bytes(16, "little"), s, x[s], 0.0, z[s], 0.0)
            e = g.by_slot[s]
            e.space, e.aoi = 0, True  # (the model reads positions only: no relation is built)
        cs = np.concatenate([movers, rng.integers(0, n, 12)])
        pts = np.array([[x[s], 0, z[s]] for s in movers] + [[x[4000] - 60, 0, z[4000] + 45]], np.float32)
        for r in (3.0, 25.0, 75.0):
            q = np.concatenate([queries(cs, r), queries(np.zeros(len(pts)), r, points=pts)])
            rows, _ = range_model(g, q, tags)
            check_all_forms(w, q, rows, f"r = {r}")
        assert all(s in rows[len(cs) + j][0] for j, s in enumerate(movers))


@pytest.mark.gpu
def test_range_queries_errors_leave_the_world_usable():
    import ctypes as C

    import torch
    from goworld_amd import GwaoiError, World
    from goworld_amd._lib import RangeRows
    n = 16
    nan, inf = np.float32(np.nan), np.float32(np.inf)

    def good(w):
        off, items, dists = w.range_batch(queries([0, 2, 0], [10.0, 25.0, 1.0], points=None))
        assert off.tolist() == [0, 1, 3, 3] and items[0] == 1 and sorted(items[1:].tolist()) == [0, 1]
        assert sorted(dists.tolist()) == [10.0, 10.0, 20.0]
        assert w.range_count_batch(queries([0], 15.0, points=[[5, 0, 0]])).tolist() == [3]

    def raises(code, f, *args):
        with pytest.raises(GwaoiError) as ei:
            f(*args)
        assert ei.value.code == code

    with World(n, max_spaces=3, device=0) as w:
        sp = w.space_create(100.0)
        gone = w.space_create(5.0)
        w.space_destroy(gone)
        w.entity_bind([0, 1, 2], EID[:3])
        for s in range(3):
            w.enter(sp, s, 10.0 * s, 0.0)
        ok = queries([0, 1], 15.0)
        # ops queued since the last flush; a flush in flight
        raises(-3, w.range_batch, ok)
        raises(-3, w.range_count_batch, ok)
        w.tick_begin()
        raises(-3, w.range_batch, ok)
        raises(-3, w.range_count_batch, ok)
        w.tick_end()
        good(w)
        # host forms, one class per call: nothing is produced and the previous result stays readable
        L, h = w._L, w._w
        r = RangeRows()
        assert L.gwaoi_range_batch(h, ok.ctypes.data_as(C.c_void_p), 2, C.byref(r)) == 0
        before = (r.n, r.offsets, r.items, r.dists)

        def prev():
            off = np.ctypeslib.as_array(C.cast(r.offsets, C.POINTER(C.c_uint32)), shape=(3,)).tolist()
            it = np.ctypeslib.as_array(C.cast(r.items, C.POINTER(C.c_uint32)), shape=(3,)).tolist()
            ds = np.ctypeslib.as_array(C.cast(r.dists, C.POINTER(C.c_float)), shape=(3,)).tolist()
            return off, it[:1], sorted(it[1:]), ds[:1], sorted(ds[1:])

        want_prev = ([0, 1, 3], [1], [0, 2], [10.0], [10.0, 10.0])
        assert prev() == want_prev

        def bad(field, value, point=False):
            q = queries([0, 0, 0], 15.0, points=[[0, 0, 0]] * 3) if point else queries([0, 1, 2], 15.0)
            q[1][field] = value
            return q

        classes = [
            (-1, bad("flags", 4)), (-1, bad("flags", 0x80000001)), (-1, bad("radius", -1.0)),
            (-6, bad("radius", nan)), (-6, bad("radius", inf)),
            (-6, bad("x", nan, True)), (-6, bad("y", inf, True)), (-6, bad("z", -inf, True)),
            (-2, bad("center", n)), (-2, bad("center", 0xFFFFFFFF)),
            (-7, bad("center", gone, True)), (-7, bad("center", 2, True)), (-7, bad("center", 3, True)),
        ]
        for code, q in classes:
            r2 = RangeRows(7, 1, 2, 3)
            assert L.gwaoi_range_batch(h, q.ctypes.data_as(C.c_void_p), 3, C.byref(r2)) == code
            assert (r2.n, r2.offsets, r2.items, r2.dists) == (7, 1, 2, 3)
            cnt = np.full(3, 7, np.uint32)
            assert L.gwaoi_range_count_batch(h, q.ctypes.data_as(C.c_void_p), 3, cnt.ctypes.data_as(C.c_void_p)) == code
            assert cnt.tolist() == [7, 7, 7]
            assert prev() == want_prev
        # -0.0 is 0; a NaN point without POINT is ignored
        q = queries([0, 1], [-0.0, 15.0])
        q["x"] = nan
        assert w.range_count_batch(q).tolist() == [0, 2]
        # null arguments
        qp = ok.ctypes.data_as(C.c_void_p)
        assert L.gwaoi_range_batch(h, None, 2, C.byref(r2)) == -1
        assert L.gwaoi_range_batch(h, qp, 2, None) == -1
        assert L.gwaoi_range_count_batch(h, None, 2, qp) == -1
        assert L.gwaoi_range_count_batch(h, qp, 2, None) == -1
        good(w)
        # device forms, one class per call among good queries: the bad query's row is empty, the others exact
        for code, q in classes:
            if code == -7 and q[1]["center"] < 3:
                continue  # (a space id below max_spaces is nothing the device can tell from an empty space)
            full = np.concatenate([queries([0], 15.0), q, queries([2], 25.0)])
            dq = _dev_q(full)
            assert L.gwaoi_range_batch_device(h, dq.data_ptr(), 5, C.byref(r2)) == code
            off = np.frombuffer(_d2h(r2.offsets, 24), np.uint32)
            point = bool(q[0]["flags"] & RANGE_POINT)
            c = 2 if point else 1
            assert r2.n == 5 and np.diff(off.astype(np.int64)).tolist() == [1, c, 0, c, 2], (code, off)
            items = np.frombuffer(_d2h(r2.items, 4 * int(off[-1])), np.uint32)
            dists = np.frombuffer(_d2h(r2.dists, 4 * int(off[-1])), np.float32)
            assert items[0] == 1 and dists[0] == 10.0 and sorted(items[-2:].tolist()) == [0, 1]
            assert sorted(dists[-2:].tolist()) == [10.0, 20.0]
            out = torch.full((5,), 7, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            assert L.gwaoi_range_count_batch_device(h, dq.data_ptr(), 5, out.data_ptr()) == code
            assert out.cpu().tolist() == [1, c, 0, c, 2]
            raises(code, w.range_batch_device, dq.data_ptr(), 5)
            good(w)
        # a destroyed or never created space below max_spaces on the device: nobody is in it
        dq = _dev_q(queries([gone, 2, sp], 3e38, points=[[0, 0, 0]] * 3))
        out = torch.full((3,), 7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        w.range_count_batch_device(dq.data_ptr(), 3, out.data_ptr())
        assert out.cpu().tolist() == [0, 0, 3]
        # a misaligned device array
        raises(-1, w.range_batch_device, dq.data_ptr() + 4, 1)
        # n == 0
        off, items, dists = w.range_batch(np.empty(0, RANGE_QUERY))
        assert off.tolist() == [0] and items.size == 0 and dists.size == 0
        assert w.range_count_batch(np.empty(0, RANGE_QUERY)).size == 0
        assert w.range_batch_device(0, 0)[3] == 0
        w.range_count_batch_device(0, 0, 0)
        good(w)
        w.moved(0, 1.0, 0.0)
        w.tick()  # flushes still run
        off, items, dists = w.range_batch(queries([0], 10.0))
        assert items.tolist() == [1] and dists.tolist() == [9.0]
