"""Broadcast fan-out (gwaoi_collect_broadcast, include/gwaoi_sync.h): GoWorld's
AllClients delivery -- Entity.CallAllClients (Entity.go:743-749), ForAllClients
(Entity.go:768-778) and the AllClients attribute notifications
(Entity.go:814-917) -- for a sparse batch of (source slot, flags) messages.

Expected records come from the sequential restatement (oracle/entity_sync.py)
driven by tests/sync_scenario.py: message m = (s, f) gives (e.cid, m, s, s) if
f & 1 and the source has a client, and (nb.cid, m, s, b) for every b in the
source's InterestedBy with a client if f & 2, each filed under the receiver's
gate.  Compared as sorted 32-byte records per gate (the order inside a gate is
unspecified, the multiset is exact).
"""
import functools
import struct

import numpy as np
import pytest

import sync_scenario as SS
from oracle.entity_sync import GameEntities, records_by_gate

EID = [bytes([65 + i]) * 16 for i in range(6)]
CID = [bytes([97 + i]) * 16 for i in range(6)]
OWN, NEIGHBORS = 1, 2


def cast_rec(cid, m, src, dst):
    return cid + struct.pack("<4I", m, src, dst, 0)


def expected_cast(g, slots, flags):
    """{gate: sorted 32-byte records} of the messages (slots[m], flags[m]) on the restatement g."""
    out = {}
    for m, (s, f) in enumerate(zip(slots, flags)):
        s, f = int(s), int(f)
        e = g.by_slot.get(s)
        if e is None:  # a slot never bound: no entity, no client, no neighbours
            continue
        if f & OWN and e.cid:
            out.setdefault(e.gate, []).append(cast_rec(e.cid, m, s, s))
        if f & NEIGHBORS:
            for b in e.By:
                nb = g.by_slot[b]
                if nb.cid:
                    out.setdefault(nb.gate, []).append(cast_rec(nb.cid, m, s, b))
    return {k: sorted(v) for k, v in out.items()}


# ------------------------------------------------------------------ CPU ------

def small_world():
    """tests/test_sync.py's small_world shape: entities 0..2 in one AOI space 10 apart (D = 100),
    clients on 0 and 1, entity 3 never in a space."""
    g = GameEntities({0: 100.0}, 8)
    for i in range(4):
        g.create(EID[i], i, 10.0 * i, 1.0, 0.0, 0.5)
    g.set_client(0, 1, CID[0])
    g.set_client(1, 2, CID[1])
    for i in range(3):
        g.enter_space(i, 0, 10.0 * i, 1.0, 0.0)
    return g


def test_library_entry_points_validate_without_a_gpu():
    from goworld_amd import _lib, build
    build.build()
    L = _lib.load()
    assert L.gwaoi_collect_broadcast(None, None, None, 0, None) == -1
    assert L.gwaoi_collect_broadcast_device(None, None, None, 0, None) == -1


def test_record_dtype_matches_the_record_size():
    from goworld_amd import CAST_DTYPE, CAST_REC
    assert CAST_DTYPE.itemsize == 32 == CAST_REC
    assert CAST_DTYPE.names == ("cid", "msg", "src", "dst", "pad")
    r = np.frombuffer(cast_rec(CID[0], 7, 3, 9), CAST_DTYPE)[0]
    assert bytes(r["cid"]) == CID[0] and (r["msg"], r["src"], r["dst"], r["pad"]) == (7, 3, 9, 0)


def test_expected_records_on_the_small_world():
    g = small_world()
    # entity 0: its own client plus entity 1's (entity 2 is interested too but has no client)
    assert g.by_slot[0].By == {1, 2}
    assert expected_cast(g, [0], [OWN | NEIGHBORS]) == {1: [cast_rec(CID[0], 0, 0, 0)], 2: [cast_rec(CID[1], 0, 0, 1)]}
    # entity 2 has no client: nothing of its own, its neighbours' clients still hear it
    assert expected_cast(g, [2], [OWN]) == {}
    assert expected_cast(g, [2], [OWN | NEIGHBORS]) == {1: [cast_rec(CID[0], 0, 2, 0)], 2: [cast_rec(CID[1], 0, 2, 1)]}
    # entity 3 is in nilSpace: its own client only, once it has one
    assert expected_cast(g, [3], [OWN | NEIGHBORS]) == {}
    g.set_client(3, 2, CID[3])
    assert expected_cast(g, [3, 3, 3], [OWN | NEIGHBORS, NEIGHBORS, 0]) == {2: [cast_rec(CID[3], 0, 3, 3)]}
    # the message index is the array position; slots 4.. were never bound
    assert expected_cast(g, [5, 1], [3, OWN]) == {2: [cast_rec(CID[1], 1, 1, 1)]}


# ------------------------------------------------------------------ GPU ------

def scenario_messages(i, n):
    """The messages broadcast after flush i: 150 drawn sources, then the 8 slots never bound."""
    rng = np.random.default_rng(1000 + i)
    slots = np.concatenate([rng.integers(0, n, 150), np.arange(n, n + 8)]).astype(np.uint32)
    flags = np.concatenate([rng.integers(1, 4, 150), np.full(8, 3)]).astype(np.uint32)
    return slots, flags


@functools.lru_cache(maxsize=None)
def scenario_expected():
    """The scenario and, per flush, the expected broadcast, sync collect and class counts (computed
    once on the restatement, shared and left unchanged by the tests)."""
    sc = SS.make(seed=21, n=600, flushes=4)
    n = sc["n"]
    exp = []

    def on_flush(i, g):
        slots, flags = scenario_messages(i, n)
        cast = expected_cast(g, slots, flags)
        drawn = [g.by_slot[int(s)] for s in slots[:150]]
        stats = {
            "outside": sum(1 for e in drawn if not e.aoi),
            "no_client": sum(1 for e in drawn if e.cid is None),
            "deaf_neighbours": sum(1 for e, f in zip(drawn, flags) if f & NEIGHBORS
                                   for b in e.By if g.by_slot[b].cid is None),
            "repeated": 150 - len(set(slots[:150].tolist())),
            "gates": sorted(cast),
            "records": sum(len(v) for v in cast.values()),
        }
        exp.append({"cast": cast, "sync": g.collect(), "stats": stats})

    SS.run_oracle(sc, on_flush)
    return sc, exp


def test_scenario_covers_every_class_of_message():
    """Checked on the restatement (no GPU): at every flush the draw has sources outside any AOI
    space, sources without a client, neighbours without a client, repeated sources and all four
    gates, so a scenario change cannot hollow the GPU tests out."""
    sc, exp = scenario_expected()
    assert len(exp) == len(sc["flushes"]) + 1
    for e in exp:
        st = e["stats"]
        print(st)
        assert st["outside"] > 0 and st["no_client"] > 0 and st["deaf_neighbours"] > 0 and st["repeated"] > 0
        assert st["gates"] == sorted(SS.GATES) and st["records"] > 0


def _d2h(ptr: int, nbytes: int) -> bytes:
    """Device memory to host through the HIP runtime this process already loaded."""
    import ctypes
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line)
    hip = ctypes.CDLL(path)
    out = ctypes.create_string_buffer(max(nbytes, 1))
    assert hip.hipMemcpy(out, ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return out.raw[:nbytes]


def device_cast(w, slots, flags):
    """collect_broadcast_device on torch tensors -> {gate: sorted records}, read back from the pointer."""
    import torch
    ds = torch.from_numpy(np.ascontiguousarray(slots, np.uint32).view(np.int32).copy()).to("cuda:0")
    df = torch.from_numpy(np.ascontiguousarray(flags, np.uint32).view(np.int32).copy()).to("cuda:0") \
        if flags is not None else None
    torch.cuda.synchronize()
    ids, off, ptr = w.collect_broadcast_device(ds.data_ptr(), df.data_ptr() if df is not None else 0, ds.numel())
    raw = _d2h(ptr, off[-1] * 32)
    out = {}
    for k, g in enumerate(ids):
        rows = sorted(raw[32 * j:32 * j + 32] for j in range(off[k], off[k + 1]))
        if rows:
            out[int(g)] = rows
    return out


def run_scenario(cast):
    """Drive the scenario on the GPU; after every flush broadcast (cast(w, slots, flags) ->
    {gate: sorted records}) BEFORE the sync collect, twice, and compare all three with the restatement."""
    from goworld_amd import World
    sc, exp = scenario_expected()
    n = sc["n"]
    seen = []

    def on_flush(i, w, ent=None, lev=None):
        slots, flags = scenario_messages(i, n)
        got = cast(w, slots, flags)
        assert got == exp[i]["cast"], f"flush {i}: broadcast records"
        assert cast(w, slots, flags) == got, f"flush {i}: a second broadcast differs"
        # the broadcast left the sync flags (and positions, and the relation) alone
        assert records_by_gate(w.collect_sync_infos()) == exp[i]["sync"], f"flush {i}: sync records after a broadcast"
        seen.append(sum(len(v) for v in got.values()))

    with World(n + 8, max_spaces=4, device=0) as w:
        SS.run_gpu(sc, w, on_flush)
    assert seen == [e["stats"]["records"] for e in exp] and min(seen) > 0


@pytest.mark.gpu
def test_broadcast_scenario_matches_oracle():
    run_scenario(lambda w, s, f: records_by_gate(w.collect_broadcast(s, f)))


@pytest.mark.gpu
def test_broadcast_device_form_matches_oracle():
    run_scenario(device_cast)


@pytest.mark.gpu
def test_broadcast_dense_crowd_regrows_output():
    """Everyone in everyone's window (a 60 x 60 square): per-source InterestedBy of ~287, so the
    window rows are longer than one 64-lane step.  A 1-message call, then every slot once plus 64
    copies of one in-space slot (~110k records): the write pass, queued behind the count pass with
    the small call's output, writes nothing; the host regrows the output and relaunches it, and
    many waves take positions from one gate's cursor."""
    from goworld_amd import World
    sc = SS.make(seed=23, n=600, n_outside=20, flushes=2, L=60.0)
    n = sc["n"]
    left = {op[1] for ops in sc["flushes"] for op in ops if op[0] == "leave"}
    hot = next(op[1] for op in sc["setup"] if op[0] == "enter" and op[1] not in left)  # in a space throughout
    slots = np.concatenate([np.arange(n), np.full(64, hot)]).astype(np.uint32)
    flags = np.full(slots.size, 3, np.uint32)
    exp = []

    def oracle_flush(i, g):
        exp.append((expected_cast(g, slots[:1], flags[:1]), expected_cast(g, slots, flags),
                    max(len(e.By) for e in g.by_slot.values())))

    SS.run_oracle(sc, oracle_flush)
    assert all(e[2] > 256 for e in exp) and all(sum(len(v) for v in e[1].values()) > 100_000 for e in exp)

    def on_flush(i, w, ent=None, lev=None):
        if i == 0:
            assert records_by_gate(w.collect_broadcast(slots[:1], flags[:1])) == exp[0][0]
        assert records_by_gate(w.collect_broadcast(slots, flags)) == exp[i][1], f"flush {i}"

    with World(n, max_spaces=4, device=0) as w:
        SS.run_gpu(sc, w, on_flush)


@pytest.mark.gpu
def test_broadcast_window_bounds_and_ownership():
    """One space with D = 0.1f and 64 entities on a lattice of pitch D around x = z = 1024, where
    fl32(w - D) / fl32(w + D) decide membership and depend on which entity owns the window
    (the later seq): moved in a seeded order so that owners differ.  The receivers of every source
    are exactly the restatement's neighbours with a client, and the library's own gwaoi_neighbors."""
    from goworld_amd import CAST_DTYPE, World
    from oracle.oracle import SpacesOracle
    D = np.float32(0.1)
    n = 64
    xs = (np.float32(1024.0) + D * np.arange(8, dtype=np.float32)).astype(np.float32)
    x = np.repeat(xs, 8)
    z = np.tile(xs, 8)
    rng = np.random.default_rng(5)
    has = rng.random(n) < 0.75
    order = rng.permutation(n)
    ora = SpacesOracle({0: float(D)}, n)
    with World(n, device=0) as w:
        sp = w.space_create(float(D))
        w.entity_bind(list(range(n)), [bytes([s]) * 16 for s in range(n)])
        for s in np.nonzero(has)[0]:
            w.entity_set_client(int(s), 1 + int(s) % 3, bytes([128 + int(s)]) * 16)
        for s in range(n):
            w.enter(sp, s, x[s], z[s])
            ora.enter(0, s, x[s], z[s])
        w.tick()
        for s in order:  # same positions, new seqs: ownership of each pair follows this order
            w.moved(int(s), x[s], z[s])
            ora.moved(int(s), x[s], z[s])
        w.tick()
        got = w.collect_broadcast(np.arange(n), np.full(n, NEIGHBORS))
        recs = np.concatenate([a.reshape(-1).view(CAST_DTYPE) for a in got.values()])
        sizes = set()
        for s in range(n):
            mine = recs[recs["src"] == s]
            assert (mine["msg"] == s).all()
            nbr = ora.neighbors(s)
            want = sorted(int(b) for b in nbr if has[b])
            assert sorted(mine["dst"].tolist()) == want, f"source {s}"
            assert want == sorted(int(b) for b in w.neighbors(s) if has[b]), f"source {s}: gwaoi_neighbors"
            for r in mine:
                assert bytes(r["cid"]) == bytes([128 + int(r["dst"])]) * 16
            sizes.add(len(nbr))
        for g, a in got.items():
            assert all(1 + int(d) % 3 == g for d in a.reshape(-1).view(CAST_DTYPE)["dst"])
        assert len(sizes) > 1 and len(recs) > 0  # corner, edge and inner entities differ


@pytest.mark.gpu
def test_broadcast_default_flags_zero_flags_and_empty_batch():
    from goworld_amd import World
    sc, exp = scenario_expected()
    n = sc["n"]

    short = dict(sc, flushes=[])  # the setup flush only
    g = SS.run_oracle(short, lambda i, g: None)

    def on_flush(i, w, ent=None, lev=None):
        slots, _ = scenario_messages(0, n)
        both = records_by_gate(w.collect_broadcast(slots, np.full(slots.size, 3)))
        assert both == expected_cast(g, slots, np.full(slots.size, 3)) and both
        assert records_by_gate(w.collect_broadcast(slots)) == both  # flags=None: OWN | NEIGHBORS
        assert device_cast(w, slots, None) == both
        assert records_by_gate(w.collect_broadcast(slots, np.zeros(slots.size))) == {}
        assert w.collect_broadcast([]) == {}
        assert w.collect_broadcast([], []) == {}
        assert w.collect_broadcast_device(0, 0, 0)[1][-1] == 0

    with World(n + 8, max_spaces=4, device=0) as w:
        SS.run_gpu(short, w, on_flush)


@pytest.mark.gpu
def test_broadcast_errors_leave_the_world_usable():
    import ctypes as C

    import torch
    from goworld_amd import GwaoiError, World
    from goworld_amd._lib import GateRecords
    n = 16
    with World(n, device=0) as w:
        sp = w.space_create(100.0)
        w.entity_bind([0, 1, 2], EID[:3])
        w.entity_set_client(0, 1, CID[0])
        w.entity_set_client(1, 2, CID[1])
        for s in range(3):
            w.enter(sp, s, 10.0 * s, 0.0)
        with pytest.raises(GwaoiError) as ei:
            w.collect_broadcast([0])  # ops queued since the last flush
        assert ei.value.code == -3
        w.tick()
        good = {1: [cast_rec(CID[0], 0, 0, 0), cast_rec(CID[0], 1, 2, 0)],
                2: [cast_rec(CID[1], 0, 0, 1), cast_rec(CID[1], 1, 2, 1)]}
        assert records_by_gate(w.collect_broadcast([0, 2])) == good
        with pytest.raises(GwaoiError) as ei:
            w.collect_broadcast([0, n, 2])  # slot == max_slots
        assert ei.value.code == -2
        assert records_by_gate(w.collect_broadcast([0, 2])) == good
        with pytest.raises(GwaoiError) as ei:
            w.collect_broadcast([0, 2], [3, 4])  # a flag bit outside OWN | NEIGHBORS
        assert ei.value.code == -1
        # device form: the offending message is dropped and reported; the world is not poisoned
        ds = torch.tensor([0, n, 2], dtype=torch.int32, device="cuda:0")
        df = torch.tensor([3, 3, 4], dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(GwaoiError) as ei:
            w.collect_broadcast_device(ds.data_ptr(), 0, 3)
        assert ei.value.code == -2
        with pytest.raises(GwaoiError) as ei:
            w.collect_broadcast_device(ds.data_ptr() + 8, df.data_ptr() + 8, 1)
        assert ei.value.code == -1
        out = GateRecords()  # through the C ABI: the other messages are delivered with the error code
        assert w._L.gwaoi_collect_broadcast_device(w._w, ds.data_ptr(), None, 3, C.byref(out)) == -2
        assert out.n_gates == 2 and out.offsets[2] == 4
        raw = _d2h(out.records, 4 * 32)
        assert sorted(raw[32 * j:32 * j + 32] for j in range(4)) == sorted(
            cast_rec(CID[k], m, s, k) for m, s in ((0, 0), (2, 2)) for k in (0, 1))
        assert device_cast(w, [0, 2], [3, 3]) == good
        assert records_by_gate(w.collect_broadcast([0, 2])) == good
        w.moved(0, 1.0, 0.0)
        w.tick()  # flushes still run
        assert records_by_gate(w.collect_broadcast([0, 2])) == good
