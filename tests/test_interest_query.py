"""Interest-set reads on the GPU (include/gwaoi_sync.h, "interest-set reads"): the batched forms
of what GoWorld's game logic reads from InterestedIn -- the rows themselves
(gwaoi_neighbors_batch: Monster.AI's loop, Monster.go:49-65; Avatar.go:281-307's count by type),
membership of a pair (gwaoi_related_batch: Entity.IsInterestedIn, Entity.go:248-251) and the
nearest neighbour that passes a tag filter (gwaoi_nearest_batch: Monster.AI's nearest living
Player by Entity.DistanceTo, Entity.go:253-256 with Vector3.go:22-28).

The models are built here over the sequential restatement (oracle/entity_sync.py) driven by
tests/sync_scenario.py: a row is sorted(e.In) (and e.In == e.By throughout), membership is
b in In[a], and the nearest is the candidate of the smallest (d2, slot) with d2 summed in numpy
float32 step by step and the distance np.float32(np.sqrt(np.float64(d2))).  Every comparison is
exact; distances are compared bit for bit.
"""
import functools

import numpy as np
import pytest

import sync_scenario as SS
from oracle.entity_sync import GameEntities, records_by_gate
from test_broadcast import _d2h  # device memory to host through the HIP runtime the process loaded

EID = [bytes([65 + i]) * 16 for i in range(16)]
CID = [bytes([97 + i]) * 16 for i in range(6)]
NO_SLOT = 0xFFFFFFFF
F32 = np.float32


# --------------------------------------------------------------- models ------

def rows_model(g, slots):
    """[sorted InterestedIn of each slot]; a slot that is no entity has an empty row."""
    rows = []
    for s in slots:
        e = g.by_slot.get(int(s))
        if e is not None:
            assert e.In == e.By, f"slot {s}: InterestedIn != InterestedBy"
            assert e.aoi or not e.In
        rows.append(sorted(e.In) if e is not None else [])
    return rows


def related_model(g, a, b):
    return np.array([int(y) in g.by_slot[int(x)].In if int(x) in g.by_slot else False for x, y in zip(a, b)], bool)


def dist2(ea, eb):
    """Vector3.DistanceTo's sum in float32, step by step (every operand and result is np.float32)."""
    dx, dy, dz = F32(eb.x) - F32(ea.x), F32(eb.y) - F32(ea.y), F32(eb.z) - F32(ea.z)
    return F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))


def nearest_model(g, tags, slots, masks=None, wants=None):
    out_s = np.full(len(slots), NO_SLOT, np.uint32)
    out_d = np.full(len(slots), np.inf, np.float32)
    ties = 0
    for m, s in enumerate(slots):
        e = g.by_slot.get(int(s))
        if e is None:
            continue
        cand = [(dist2(e, g.by_slot[b]), b) for b in e.In
                if masks is None or (int(tags[b]) & int(masks[m])) == int(wants[m])]
        if not cand:
            continue
        d2, b = min(cand)
        ties += sum(1 for c in cand if c[0] == d2) - 1
        out_s[m] = b
        out_d[m] = F32(np.sqrt(np.float64(d2)))
    return out_s, out_d, ties


def split_rows(off, items):
    return [sorted(items[off[m]:off[m + 1]].tolist()) for m in range(len(off) - 1)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------ CPU ------

def small_world():
    """tests/test_broadcast.py's small_world shape: entities 0..2 in one AOI space 10 apart (D = 100),
    entity 3 never in a space; y = 1."""
    g = GameEntities({0: 100.0}, 8)
    for i in range(4):
        g.create(EID[i], i, 10.0 * i, 1.0, 0.0, 0.5)
    for i in range(3):
        g.enter_space(i, 0, 10.0 * i, 1.0, 0.0)
    return g


def test_library_entry_points_validate_without_a_gpu():
    from goworld_amd import _lib, build
    build.build()
    L = _lib.load()
    assert L.gwaoi_neighbors_batch(None, None, 0, None) == -1
    assert L.gwaoi_neighbors_batch_device(None, None, 0, None) == -1
    assert L.gwaoi_related_batch(None, None, None, 0, None) == -1
    assert L.gwaoi_related_batch_device(None, None, None, 0, None) == -1
    assert L.gwaoi_entity_set_tag(None, 0, 0) == -1
    assert L.gwaoi_entity_set_tag_batch(None, None, None, 0) == -1
    assert L.gwaoi_nearest_batch(None, None, None, None, 0, None, None) == -1
    assert L.gwaoi_nearest_batch_device(None, None, None, None, 0, None, None) == -1
    from goworld_amd import NO_SLOT as exported, World
    assert exported == NO_SLOT == World.NO_SLOT


def test_expected_answers_on_the_small_world():
    g = small_world()
    assert rows_model(g, [0, 1, 2, 3, 5, 1]) == [[1, 2], [0, 2], [0, 1], [], [], [0, 2]]
    assert related_model(g, [0, 0, 2, 3, 0, 5], [1, 0, 0, 0, 3, 0]).tolist() == [True, False, True, False, False, False]
    tags = np.array([1, 2, 1, 1, 0, 0, 0, 0], np.uint32)
    s, d, _ = nearest_model(g, tags, [0, 1, 2, 3])
    assert s.tolist() == [1, 0, 1, NO_SLOT]  # entity 1 is 10 from both: the smaller slot wins
    assert d.tolist()[:3] == [10.0, 10.0, 10.0] and np.isinf(d[3])
    # tag bit 1 only: entity 0 sees 2 (20 away), entity 1 sees 0, entity 2 sees 0; nobody carries bit 4
    s, d, _ = nearest_model(g, tags, [0, 1, 2, 0], [1, 1, 1, 4], [1, 1, 1, 4])
    assert s.tolist() == [2, 0, 0, NO_SLOT] and d.tolist()[:3] == [20.0, 10.0, 20.0] and np.isinf(d[3])
    # y counts: lift entity 1 by 30 and entity 0's nearest is entity 2
    g.set_position_yaw_noflags(1, 10.0, 31.0, 0.0, 0.5)
    s, d, _ = nearest_model(g, tags, [0])
    assert s.tolist() == [2] and d.tolist() == [20.0]
    assert dist2(g.by_slot[0], g.by_slot[1]) == F32(1000.0)


def scenario_queries(i, n):
    """The sources queried after flush i: 150 drawn slots, then the 8 slots never bound."""
    rng = np.random.default_rng(2000 + i)
    return np.concatenate([rng.integers(0, n, 150), np.arange(n, n + 8)]).astype(np.uint32)


def scenario_tags(n):
    s = np.arange(n + 8)
    return ((1 << (s % 3)) | np.where(s % 5, 8, 0)).astype(np.uint32)


def scenario_pairs(i, g, n, slots):
    """Membership pairs after flush i, by class: true pairs from In, random pairs, cross-space pairs,
    a == b, pairs with a slot outside every AOI space."""
    rng = np.random.default_rng(3000 + i)
    drawn = [int(s) for s in slots[:150]]
    inside = [s for s in range(n) if g.by_slot[s].aoi]
    outside = [s for s in range(n) if not g.by_slot[s].aoi]
    by_sp = {sp: [s for s in inside if g.by_slot[s].space == sp] for sp in (0, 1)}
    cls = {
        "true": [(s, b) for s in drawn[:60] for b in sorted(g.by_slot[s].In)[:2]],
        "random": [tuple(p) for p in rng.integers(0, n, (200, 2)).tolist()],
        "cross": list(zip(rng.choice(by_sp[0], 40).tolist(), rng.choice(by_sp[1], 40).tolist())),
        "same": [(s, s) for s in drawn[:20]],
        "outside": ([(int(o), int(s)) for o, s in zip(rng.choice(outside, 20), rng.choice(inside, 20))] +
                    [(int(s), int(o)) for o, s in zip(rng.choice(outside, 20), rng.choice(inside, 20))] +
                    [(drawn[0], n + 3), (n + 1, drawn[1]), (n, n + 7)]),
    }
    pairs = np.array([p for v in cls.values() for p in v], np.uint32)
    return pairs[:, 0].copy(), pairs[:, 1].copy(), {k: len(v) for k, v in cls.items()}


@functools.lru_cache(maxsize=None)
def scenario_expected():
    """The scenario and, per flush, the expected rows, membership, nearest, sync collect and class
    counts (computed once on the restatement, shared and left unchanged by the tests)."""
    sc = SS.make(seed=21, n=600, flushes=4)
    n = sc["n"]
    tags = scenario_tags(n)
    exp = []

    def on_flush(i, g):
        slots = scenario_queries(i, n)
        rows = rows_model(g, slots)
        a, b, classes = scenario_pairs(i, g, n, slots)
        rel = related_model(g, a, b)
        mask = np.full(slots.size, 9, np.uint32)
        near = nearest_model(g, tags, slots, mask, mask)
        near_all = nearest_model(g, tags, slots)
        drawn = [g.by_slot[int(s)] for s in slots[:150]]
        stats = {
            "outside": sum(1 for e in drawn if not e.aoi),
            "repeats": 150 - len(set(slots[:150].tolist())),
            "spaces": sorted({e.space for e in drawn if e.aoi}),
            "none": sum(1 for e, s in zip(drawn, near[0][:150]) if e.aoi and s == NO_SLOT),
            "found": int((near[0] != NO_SLOT).sum()),
            "items": sum(len(r) for r in rows),
            "ties": near[2] + near_all[2],
            "classes": classes,
            "related_true": int(rel.sum()),
            "longest": max(len(r) for r in rows),
        }
        exp.append({"rows": rows, "pairs": (a, b), "rel": rel, "near": near[:2], "near_all": near_all[:2],
                    "sync": g.collect(), "stats": stats})

    SS.run_oracle(sc, on_flush)
    return sc, tags, exp


def test_scenario_covers_every_class_of_query():
    """Checked on the restatement (no GPU): at every flush the draw has sources outside every AOI
    space, repeated sources, sources in both AOI spaces, filtered searches that leave nobody and
    more than 100 that find someone, and membership pairs of every class, so a scenario change
    cannot hollow the GPU tests out."""
    sc, tags, exp = scenario_expected()
    assert len(exp) == len(sc["flushes"]) + 1 == 5
    for e in exp:
        st = e["stats"]
        print(st)
        assert 8 <= st["outside"] <= 14
        assert 9 <= st["repeats"] <= 24
        assert st["spaces"] == [0, 1]
        assert 5 <= st["none"] <= 11
        assert 125 <= st["found"] <= 132 and st["found"] >= 100
        assert 1714 <= st["items"] <= 1963
        assert st["ties"] == 0  # (ties get a test of their own)
        assert all(v > 0 for v in st["classes"].values()) and sorted(st["classes"]) == [
            "cross", "outside", "random", "same", "true"]
        assert st["classes"]["true"] <= st["related_true"] < len(e["rel"])
        assert st["outside"] + st["none"] + st["found"] == 150


# ------------------------------------------------------------------ GPU ------

def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def device_rows(w, slots):
    """neighbors_batch_device on a torch tensor -> (offsets, items), read back from the pointers."""
    ds = _dev(slots)
    op, ip, n_items = w.neighbors_batch_device(ds.data_ptr(), ds.numel())
    off = np.frombuffer(_d2h(op, 4 * (ds.numel() + 1)), np.uint32)
    assert off[-1] == n_items
    return off, np.frombuffer(_d2h(ip, 4 * n_items), np.uint32)


def device_related(w, a, b):
    import torch
    da, db = _dev(a), _dev(b)
    out = torch.full((da.numel(),), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    w.related_batch_device(da.data_ptr(), db.data_ptr(), da.numel(), out.data_ptr())
    return out.cpu().numpy().astype(bool)


def device_nearest(w, slots, masks=None, wants=None):
    import torch
    ds = _dev(slots)
    dm = _dev(masks) if masks is not None else None
    dw = _dev(wants) if masks is not None else None
    os_ = torch.zeros(ds.numel(), dtype=torch.int32, device="cuda:0")
    od = torch.zeros(ds.numel(), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    w.nearest_batch_device(ds.data_ptr(), dm.data_ptr() if dm is not None else 0,
                           dw.data_ptr() if dw is not None else 0, ds.numel(), os_.data_ptr(), od.data_ptr())
    return os_.cpu().numpy().view(np.uint32), od.cpu().numpy()


@pytest.mark.gpu
def test_interest_queries_scenario_matches_oracle():
    """After every flush: rows (host and device form), membership and nearest (host and device
    form) against the models, the same again with an identical result, and then the sync collect
    still equals the restatement's (the queries changed nothing)."""
    from goworld_amd import World
    sc, tags, exp = scenario_expected()
    n = sc["n"]
    seen = []

    def on_flush(i, w, ent=None, lev=None):
        if i == 0:
            w.entity_set_tag(np.arange(n + 8), tags)
        e = exp[i]
        slots = scenario_queries(i, n)
        mask = np.full(slots.size, 9, np.uint32)
        a, b = e["pairs"]
        off, items = w.neighbors_batch(slots)
        assert off.size == slots.size + 1 and off[0] == 0 and off[-1] == items.size
        assert split_rows(off, items) == e["rows"], f"flush {i}: rows"
        doff, ditems = device_rows(w, slots)
        assert np.array_equal(doff, off) and split_rows(doff, ditems) == e["rows"], f"flush {i}: device rows"
        assert np.array_equal(w.related_batch(a, b), e["rel"]), f"flush {i}: membership"
        assert np.array_equal(device_related(w, a, b), e["rel"]), f"flush {i}: device membership"
        for m, want in ((mask, e["near"]), (None, e["near_all"])):
            s, d = w.nearest_batch(slots, m, m)
            assert np.array_equal(s, want[0]) and same_bits(d, want[1]), f"flush {i}: nearest"
            s2, d2 = device_nearest(w, slots, m, m)
            assert np.array_equal(s2, want[0]) and same_bits(d2, want[1]), f"flush {i}: device nearest"
            s3, d3 = w.nearest_batch(slots, m, m)
            assert np.array_equal(s3, s) and same_bits(d3, d), f"flush {i}: a second nearest differs"
        off2, items2 = w.neighbors_batch(slots)
        assert np.array_equal(off2, off) and np.array_equal(items2, items), f"flush {i}: a second rows call differs"
        assert np.array_equal(ditems, items), f"flush {i}: host and device rows differ in order"
        assert np.array_equal(w.related_batch(a, b), e["rel"])
        # the queries left the sync flags (and positions, and the relation) alone
        assert records_by_gate(w.collect_sync_infos()) == e["sync"], f"flush {i}: sync records after the queries"
        seen.append(int(off[-1]))

    with World(n + 8, max_spaces=4, device=0) as w:
        SS.run_gpu(sc, w, on_flush)
    assert seen == [e["stats"]["items"] for e in exp] and min(seen) > 0


@pytest.mark.gpu
def test_interest_queries_dense_crowd_regrows_rows():
    """Everyone in everyone's window (a 60 x 60 square): the longest row is 285-289, longer than
    one group of 128 candidates.  A 1-query call, then every slot once plus 64 copies of one
    in-space slot (more than 100,000 items): the write pass, queued behind the count pass and the
    scan with the small call's output, declines; the host regrows the items and relaunches it.
    The nearest search runs over the same crowd."""
    from goworld_amd import World
    sc = SS.make(seed=23, n=600, n_outside=20, flushes=2, L=60.0)
    n = sc["n"]
    left = {op[1] for ops in sc["flushes"] for op in ops if op[0] == "leave"}
    hot = next(op[1] for op in sc["setup"] if op[0] == "enter" and op[1] not in left)  # in a space throughout
    slots = np.concatenate([np.arange(n), np.full(64, hot)]).astype(np.uint32)
    tags = scenario_tags(n)[:n]
    mask = np.full(slots.size, 9, np.uint32)
    exp = []

    def oracle_flush(i, g):
        exp.append((rows_model(g, slots), nearest_model(g, tags, slots, mask, mask)[:2],
                    nearest_model(g, tags, slots)[:2]))

    SS.run_oracle(sc, oracle_flush)
    for rows, _, _ in exp:
        assert 285 <= max(len(r) for r in rows) <= 289 and sum(len(r) for r in rows) > 100_000

    def on_flush(i, w, ent=None, lev=None):
        if i == 0:
            w.entity_set_tag(np.arange(n), tags)
            off, items = w.neighbors_batch(slots[:1])
            assert split_rows(off, items) == exp[0][0][:1]
        off, items = w.neighbors_batch(slots)
        assert split_rows(off, items) == exp[i][0], f"flush {i}: rows"
        doff, ditems = device_rows(w, slots)
        assert np.array_equal(doff, off) and np.array_equal(ditems, items), f"flush {i}: device rows"
        for m, want in ((mask, exp[i][1]), (None, exp[i][2])):
            s, d = w.nearest_batch(slots, m, m)
            assert np.array_equal(s, want[0]) and same_bits(d, want[1]), f"flush {i}: nearest"

    with World(n, max_spaces=4, device=0) as w:
        SS.run_gpu(sc, w, on_flush)


@pytest.mark.gpu
def test_interest_queries_window_bounds_and_ownership():
    """tests/test_broadcast.py's lattice: one space with D = 0.1f and 64 entities at pitch D around
    x = z = 1024, where fl32(w - D) / fl32(w + D) decide membership and depend on which entity
    owns the window (the later seq), moved in a seeded order so that owners differ.  Rows equal
    the sequential oracle's neighbours and the library's own gwaoi_neighbors for every slot, and
    membership is checked for all 64 x 64 pairs."""
    from goworld_amd import World
    from oracle.oracle import SpacesOracle
    D = np.float32(0.1)
    n = 64
    xs = (np.float32(1024.0) + D * np.arange(8, dtype=np.float32)).astype(np.float32)
    x = np.repeat(xs, 8)
    z = np.tile(xs, 8)
    order = np.random.default_rng(5).permutation(n)
    ora = SpacesOracle({0: float(D)}, n)
    with World(n, device=0) as w:
        sp = w.space_create(float(D))
        for s in range(n):
            w.enter(sp, s, x[s], z[s])
            ora.enter(0, s, x[s], z[s])
        w.tick()
        for s in order:  # same positions, new seqs: ownership of each pair follows this order
            w.moved(int(s), x[s], z[s])
            ora.moved(int(s), x[s], z[s])
        w.tick()
        want = [sorted(int(b) for b in ora.neighbors(s)) for s in range(n)]
        off, items = w.neighbors_batch(np.arange(n))
        assert split_rows(off, items) == want
        assert [w.neighbors(s).tolist() for s in range(n)] == want
        assert len({len(r) for r in want}) > 1  # corner, edge and inner entities differ
        a, b = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
        model = np.array([int(q) in want[int(p)] for p, q in zip(a, b)], bool)
        assert np.array_equal(w.related_batch(a, b), model)
        assert np.array_equal(device_related(w, a, b), model)
        assert 0 < model.sum() < n * n and np.array_equal(model.reshape(n, n), model.reshape(n, n).T)


@pytest.mark.gpu
def test_interest_queries_ties_and_filters():
    from goworld_amd import GwaoiError, World
    n = 32
    inf = np.float32(np.inf)
    with World(n, max_spaces=2, device=0) as w:
        sp = w.space_create(50.0)
        far = w.space_create(5.0)
        w.entity_bind(list(range(16)), EID)
        # ten co-located entities: everyone's nearest is the smallest other slot, at distance 0
        for s in range(10):
            w.entity_set_position_yaw(s, 3.0, 2.0, -7.0, 0.0)
            w.enter(sp, s, 3.0, -7.0)
        # slot 10 between two candidates at exactly -d and +d on x, far from the crowd; slot 13 alone
        for s, (px, py, pz) in {10: (1000.0, 0.0, 0.0), 12: (1012.5, 0.0, 0.0), 11: (987.5, 0.0, 0.0)}.items():
            w.entity_set_position_yaw(s, px, py, pz, 0.0)
            w.enter(sp, s, px, pz)
        w.entity_set_position_yaw(13, 0.0, 0.0, 0.0, 0.0)
        w.enter(far, 13, 0.0, 0.0)
        w.entity_set_tag([10, 11, 12], [1, 2, 2])
        w.tick()
        s, d = w.nearest_batch(np.arange(10))
        assert s.tolist() == [1] + [0] * 9 and same_bits(d, np.zeros(10, np.float32))
        rows = split_rows(*w.neighbors_batch(np.arange(14)))
        assert rows[:10] == [[b for b in range(10) if b != a] for a in range(10)]
        assert rows[10:] == [[11, 12], [10, 12], [10, 11], []]
        # +-12.5 on x: equal d2, the smaller slot wins
        s, d = w.nearest_batch([10], [2], [2])
        assert s.tolist() == [11] and same_bits(d, [12.5])
        s2, d2 = device_nearest(w, [10], [2], [2])
        assert s2.tolist() == [11] and same_bits(d2, [12.5])
        # clear the winner's tag bit (allowed at any time, no flush needed): the other wins
        w.entity_set_tag(11, 4)
        s, d = w.nearest_batch([10, 10], [2, 4], [2, 4])
        assert s.tolist() == [12, 11] and same_bits(d, [12.5, 12.5])
        # within one batch the last write of a slot wins
        w.entity_set_tag([11, 12, 11], [0, 2, 2])
        assert w.nearest_batch([10], [2], [2])[0].tolist() == [11]
        # unbind clears a tag
        w.entity_unbind(11)
        s, d = w.nearest_batch([10, 10], [2, 0], [2, 0])
        assert s.tolist() == [12, 11]
        w.entity_bind([11], [EID[11]])
        assert w.nearest_batch([10], [2], [2])[0].tolist() == [12]
        w.entity_set_tag(11, 2)
        # a y difference changes the winner: lift 11 by 1 (no AOI op: y is not an AOI coordinate)
        w.entity_set_position_yaw(11, 987.5, 1.0, 0.0, 0.0)
        s, d = w.nearest_batch([10, 12], [2, 0], [2, 0])
        d11 = F32(np.sqrt(np.float64(F32(F32(12.5 * 12.5) + F32(1.0)))))
        assert s.tolist() == [12, 10] and same_bits(d, [12.5, 12.5])
        s, d = w.nearest_batch([11])
        assert s.tolist() == [10] and same_bits(d, [d11])
        # a tag is kept across Leave / Enter
        w.leave(12)
        w.tick()
        assert w.nearest_batch([10], [2], [2])[0].tolist() == [11]
        w.enter(sp, 12, 1012.5, 0.0)
        w.tick()
        assert w.nearest_batch([10], [2], [2])[0].tolist() == [12]
        # an isolated entity, one never entered, one that left: empty row, NO_SLOT, +inf
        w.leave(9)
        w.tick()
        off, items = w.neighbors_batch([13, 20, 9])
        assert off.tolist() == [0, 0, 0, 0] and items.size == 0
        s, d = w.nearest_batch([13, 20, 9])
        assert s.tolist() == [NO_SLOT] * 3 and same_bits(d, [inf] * 3)
        assert not w.related_batch([13, 9, 0], [0, 0, 9]).any()
        with pytest.raises(GwaoiError) as ei:
            w.entity_set_tag(n, 1)
        assert ei.value.code == -2


@pytest.mark.gpu
def test_interest_queries_on_a_world_without_a_sync_layer():
    """Enter and tick only: the rows and membership calls work and create no sync layer (a world
    with one refuses device Leave batches, gwaoi_leave_batch_device; the first tag creates it)."""
    import torch
    from goworld_amd import GwaoiError, World
    with World(16, device=0) as w:
        sp = w.space_create(100.0)
        for s in range(3):
            w.enter(sp, s, 10.0 * s, 0.0)
        w.tick()
        assert split_rows(*w.neighbors_batch([0, 1, 2, 3])) == [[1, 2], [0, 2], [0, 1], []]
        assert split_rows(*device_rows(w, [2, 2])) == [[0, 1], [0, 1]]
        assert w.related_batch([0, 1, 3, 2], [2, 1, 0, 0]).tolist() == [True, False, False, True]
        assert device_related(w, [0, 1, 3, 2], [2, 1, 0, 0]).tolist() == [True, False, False, True]
        d = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        w.leave_batch_device(sp, d.data_ptr(), 0)  # still a world without a sync layer
        w.entity_set_tag(0, 1)
        with pytest.raises(GwaoiError) as ei:
            w.leave_batch_device(sp, d.data_ptr(), 0)
        assert ei.value.code == -3
        assert split_rows(*w.neighbors_batch([0])) == [[1, 2]]


@pytest.mark.gpu
def test_interest_queries_errors_leave_the_world_usable():
    import ctypes as C

    import torch
    from goworld_amd import GwaoiError, World
    from goworld_amd._lib import SlotRows
    n = 16
    inf = np.float32(np.inf)

    def good(w):
        assert split_rows(*w.neighbors_batch([0, 2])) == [[1, 2], [0, 1]]
        assert w.related_batch([0, 3], [2, 0]).tolist() == [True, False]
        s, d = w.nearest_batch([0, 2])
        assert s.tolist() == [1, 1] and same_bits(d, [10.0, 10.0])

    def raises(code, f, *args):
        with pytest.raises(GwaoiError) as ei:
            f(*args)
        assert ei.value.code == code

    with World(n, device=0) as w:
        sp = w.space_create(100.0)
        w.entity_bind([0, 1, 2], EID[:3])
        for s in range(3):
            w.enter(sp, s, 10.0 * s, 0.0)
        # ops queued since the last flush
        raises(-3, w.neighbors_batch, [0])
        raises(-3, w.related_batch, [0], [1])
        raises(-3, w.nearest_batch, [0])
        w.entity_set_tag(1, 5)  # a tag is no AOI op: allowed with ops queued
        w.tick()
        good(w)
        # slot == max_slots in the host forms: nothing produced
        raises(-2, w.neighbors_batch, [0, n, 2])
        raises(-2, w.related_batch, [0, n], [1, 1])
        raises(-2, w.related_batch, [0, 1], [1, n])
        raises(-2, w.nearest_batch, [0, n])
        good(w)
        # null arguments with n > 0
        L, h = w._L, w._w
        q = np.array([0, 2], np.uint32)
        qp = q.ctypes.data_as(C.c_void_p)
        r = SlotRows()
        assert L.gwaoi_neighbors_batch(h, None, 2, C.byref(r)) == -1
        assert L.gwaoi_neighbors_batch(h, qp, 2, None) == -1
        assert L.gwaoi_related_batch(h, qp, None, 2, qp) == -1
        assert L.gwaoi_related_batch(h, qp, qp, 2, None) == -1
        assert L.gwaoi_nearest_batch(h, qp, None, None, 2, None, qp) == -1
        assert L.gwaoi_nearest_batch(h, qp, qp, None, 2, qp, qp) == -1
        assert L.gwaoi_entity_set_tag_batch(h, qp, None, 2) == -1
        good(w)
        # device forms: the other rows and answers are delivered together with -2
        ds = torch.tensor([0, n, 2, 0x7FFFFFFF], dtype=torch.int32, device="cuda:0")
        db = torch.tensor([2, 0, n, 1], dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        raises(-2, w.neighbors_batch_device, ds.data_ptr(), 4)
        assert L.gwaoi_neighbors_batch_device(h, ds.data_ptr(), 4, C.byref(r)) == -2
        off = np.frombuffer(_d2h(r.offsets, 20), np.uint32)
        assert r.n == 4 and off.tolist() == [0, 2, 2, 4, 4]
        assert split_rows(off, np.frombuffer(_d2h(r.items, 16), np.uint32)) == [[1, 2], [], [0, 1], []]
        out = torch.full((4,), 7, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert L.gwaoi_related_batch_device(h, ds.data_ptr(), db.data_ptr(), 4, out.data_ptr()) == -2
        assert out.cpu().tolist() == [1, 0, 0, 0]
        os_ = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        od = torch.zeros(4, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        assert L.gwaoi_nearest_batch_device(h, ds.data_ptr(), None, None, 4, os_.data_ptr(), od.data_ptr()) == -2
        assert os_.cpu().numpy().view(np.uint32).tolist() == [1, NO_SLOT, 1, NO_SLOT]
        assert same_bits(od.cpu().numpy(), [10.0, inf, 10.0, inf])
        good(w)
        # empty batches
        off, items = w.neighbors_batch([])
        assert off.tolist() == [0] and items.size == 0
        assert w.neighbors_batch_device(0, 0)[2] == 0
        assert w.related_batch([], []).size == 0
        w.related_batch_device(0, 0, 0, 0)
        s, d = w.nearest_batch([])
        assert s.size == 0 and d.size == 0
        w.nearest_batch_device(0, 0, 0, 0, 0, 0)
        w.entity_set_tag([], [])
        # masks=None means every neighbour, whatever the tags; a filter nobody passes leaves nobody
        s, d = w.nearest_batch([0, 0, 0], [4, 4, 2], [4, 0, 2])
        assert s.tolist() == [1, 2, NO_SLOT] and same_bits(d, [10.0, 20.0, inf])
        assert w.nearest_batch([0])[0].tolist() == [1]
        assert device_nearest(w, [0, 2])[0].tolist() == [1, 1]
        w.moved(0, 1.0, 0.0)
        w.tick()  # flushes still run
        assert split_rows(*w.neighbors_batch([0, 2])) == [[1, 2], [0, 1]]
        s, d = w.nearest_batch([0, 2])
        assert s.tolist() == [1, 1] and same_bits(d, [9.0, 10.0])
