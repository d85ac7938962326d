"""Server-driven movement on the GPU (include/gwaoi_sync.h, "server-driven movement"):
gwaoi_steer_batch(_device), the batched form of Monster.Tick's chase and FaceTo
(examples/unity_demo/Monster.go:80-102, Entity.go:1292-1304, Vector3.go:44-77).

The model is built here over the sequential restatement (oracle/entity_sync.py) driven by
tests/sync_scenario.py, in numpy float32 step by step: every message is computed from a snapshot
of the entities, then the applied ones are applied in message order (MOVE through
GameEntities.set_position_yaw(from_client=False), FACE alone sets yaw and both sync flags).

Comparisons.  out_applied, out_pos[:, 0:3] and everything downstream of positions (the movers'
rows after the flush, the flush's net events, the collect records' x, y, z) are exact, bit for
bit.  Yaw goes through a float64 acos that is not pinned to the reference's, so it is compared to
the model's as an angle modulo 360: |d| <= ulp32(model) + 1e-12 degrees.  (A float64 acos good to
4 ulp on either side differs by at most 3.6e-15 rad = 2e-13 degrees; the roundings of 2 pi - y,
/ pi, * 180 and the last subtraction add under 3e-13 degrees; 1e-12 covers twice that, and one
float32 ulp covers the final rounding falling on either side of a boundary.  Modulo 360 because
DirToYaw jumps from 0 to 360 at yaw = 90.)  Where the GPU's yaw differs from the model's within
that bound, the GPU's value replaces the model's in the records expected from the next collect,
which is then compared byte for byte as the other sync tests do.
"""
import functools
import struct

import numpy as np
import pytest

import sync_scenario as SS
from oracle import oracle
from oracle.entity_sync import GameEntities, records_by_gate
from test_broadcast import _d2h  # device memory to host through the HIP runtime the process loaded
from test_interest_query import nearest_model, scenario_tags

EID = [bytes([65 + i]) * 16 for i in range(16)]
CID = [bytes([97 + i]) * 16 for i in range(16)]
NO_SLOT = 0xFFFFFFFF
MOVE, FACE = 1, 2
F32 = np.float32
EINVAL, EBADSLOT, ESTATE, ENONFINITE = -1, -2, -3, -6


# --------------------------------------------------------------- the model ------

def normalize(x, y, z):
    """Vector3.Normalize as written (Vector3.go:64-72): the sum is X*X + Y + Y + Z*Z, left to right,
    every operand and result np.float32.  Returns (x, y, z, d)."""
    s = F32(F32(F32(F32(x * x) + y) + y) + F32(z * z))
    d = F32(np.sqrt(np.float64(s)))
    if d == 0:
        return x, y, z, d
    return F32(x / d), F32(y / d), F32(z / d), d


def dir_to_yaw(x, z):
    """Vector3.DirToYaw (Vector3.go:45-62) of a direction with Y = 0: float64, then float32."""
    nx, _, nz, _ = normalize(x, F32(0), z)
    yaw = np.arccos(np.float64(nx))
    if nz < 0:
        yaw = np.float64(np.pi * 2) - yaw
    yaw = yaw / np.float64(np.pi) * np.float64(180)
    yaw = np.float64(90) - yaw if yaw <= 90 else np.float64(90) + (np.float64(360) - yaw)
    return F32(yaw)


def steer_one(a, b, s, fl):
    """The mover's (x, y, z, yaw) after one message, from entity a toward entity b."""
    x, y, z, yaw = F32(a.x), F32(a.y), F32(a.z), F32(a.yaw)
    s = F32(s)
    if fl & MOVE:
        nx, ny, nz, _ = normalize(F32(b.x - x), F32(0), F32(b.z - z))
        x, y, z = F32(x + F32(nx * s)), F32(y + F32(ny * s)), F32(z + F32(nz * s))
    if fl & FACE:
        yaw = dir_to_yaw(F32(b.x - x), F32(b.z - z))
    return x, y, z, yaw


def steer_model(g, movers, targets, steps, flags=None, apply=True):
    """(applied, pos) of a batch on the restatement g: every message from the state before the
    call; then (apply=True) the applied ones in message order.  A message whose new x or z is not
    finite, or whose yaw is NaN, does not apply (the library drops it with GWAOI_ENONFINITE)."""
    n = len(movers)
    flags = np.full(n, MOVE | FACE, np.uint32) if flags is None else flags
    applied, pos = np.zeros(n, bool), np.zeros((n, 4), np.float32)
    with np.errstate(all="ignore"):
        for m in range(n):
            a = g.by_slot.get(int(movers[m]))
            if a is None or not flags[m] or int(targets[m]) not in a.In:  # IsInterestedIn
                continue
            out = steer_one(a, g.by_slot[int(targets[m])], steps[m], int(flags[m]))
            if np.isfinite(out[0]) and np.isfinite(out[2]) and not np.isnan(out[3]):
                applied[m], pos[m] = True, out
    if apply:
        for m in np.flatnonzero(applied):
            e = g.by_slot[int(movers[m])]
            if flags[m] & MOVE:
                assert e.aoi and g.set_position_yaw(e.slot, *pos[m], from_client=False)
            else:
                e.yaw = F32(pos[m, 3])
                e.flags |= 3
    return applied, pos


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def yaw_close(got, want):
    """|got - want| as an angle modulo 360 <= ulp32(want) + 1e-12 degrees, elementwise."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    d = np.minimum(d, np.abs(360.0 - d))
    return d <= np.spacing(np.abs(want)).astype(np.float64) + 1e-12


def check_answers(got, want, what, movers=None, yaw_fix=None, g_eids=None):
    """applied and x, y, z bit for bit; yaw within the bound, the GPU's kept for the records."""
    (ga, gp), (wa, wp) = got, want
    assert np.array_equal(ga, wa), f"{what}: applied"
    assert same_bits(gp[:, :3], wp[:, :3]), f"{what}: positions"
    ok = yaw_close(gp[:, 3], wp[:, 3])
    assert ok.all(), f"{what}: yaw {gp[~ok, 3]} against {wp[~ok, 3]}"
    if yaw_fix is not None:
        for m in np.flatnonzero(wa):
            eid = g_eids[int(movers[m])]
            yaw_fix.pop(eid, None)
            if gp[m, 3].tobytes() != wp[m, 3].tobytes():
                yaw_fix[eid] = (wp[m, 3].tobytes(), gp[m, 3].tobytes())


def with_gpu_yaw(expected, yaw_fix):
    """The expected collect records (left unchanged) with the model's yaw replaced by the GPU's
    for the entities in yaw_fix, while their record still carries that model yaw."""
    def fix(r):
        f = yaw_fix.get(r[16:32])
        return r[:44] + f[1] if f is not None and r[44:] == f[0] else r
    return {gate: sorted(fix(r) for r in recs) for gate, recs in expected.items()}


# ------------------------------------------------------------------ CPU ------

def test_library_entry_points_validate_without_a_gpu():
    from goworld_amd import _lib, build
    build.build()
    L = _lib.load()
    assert L.gwaoi_steer_batch(None, None, None, None, None, 0, None, None) == EINVAL
    assert L.gwaoi_steer_batch_device(None, None, None, None, None, 0, None, None) == EINVAL
    assert "gwaoi_steer_batch" in _lib.SYNC_EXPORTS and "gwaoi_steer_batch_device" in _lib.SYNC_EXPORTS
    from goworld_amd import STEER_FACE, STEER_MOVE, World
    assert (STEER_MOVE, STEER_FACE) == (MOVE, FACE) == (World.STEER_MOVE, World.STEER_FACE)


def axis_world():
    """Entity 0 at the origin (y = 2, yaw = 0.5) and one entity 10 away on each axis, D = 100."""
    g = GameEntities({0: 100.0}, 8)
    for i, (x, z) in enumerate([(0, 0), (10, 0), (0, 10), (-10, 0), (0, -10)]):
        g.create(EID[i], i, x, 2.0, z, 0.5)
        g.enter_space(i, 0, x, 2.0, z)
    g.create(EID[5], 5, 0.0, 2.0, 0.0, 0.5)  # coincident with entity 0
    g.enter_space(5, 0, 0.0, 2.0, 0.0)
    g.collect()
    return g


def test_expected_answers_on_the_axis_world():
    g = axis_world()
    one = lambda t, s, fl=MOVE | FACE: steer_model(g, [0], [t], [s], np.array([fl], np.uint32), apply=False)
    # FaceTo alone: +x is yaw 90, +z 0, -x 270, -z 180; the position is the mover's
    for t, yaw in ((1, 90.0), (2, 0.0), (3, 270.0), (4, 180.0)):
        a, p = one(t, 1.0, FACE)
        assert a.tolist() == [True] and p[0].tolist() == [0.0, 2.0, 0.0, yaw]
    # the chase: one unit toward the target, then facing it from there; MOVE alone keeps the yaw
    assert one(1, 1.0)[1][0].tolist() == [1.0, 2.0, 0.0, 90.0]
    assert one(4, 2.5)[1][0].tolist() == [0.0, 2.0, -2.5, 180.0]
    assert one(2, 1.0, MOVE)[1][0].tolist() == [0.0, 2.0, 1.0, 0.5]
    # a step larger than the distance overshoots and then faces back; a negative step moves away
    assert one(1, 25.0)[1][0].tolist() == [25.0, 2.0, 0.0, 270.0]
    assert one(1, -3.0)[1][0].tolist() == [-3.0, 2.0, 0.0, 90.0]
    # coincident: d == 0, the direction stays (0, 0, 0): position unchanged, acos(0) -> yaw 0
    a, p = one(5, 1.0)
    assert a.tolist() == [True] and p[0].tolist() == [0.0, 2.0, 0.0, 0.0]
    # not interested, itself, no flags, a slot that is no entity: nothing
    g.create(EID[6], 6, 500.0, 0.0, 500.0, 0.0)
    g.enter_space(6, 0, 500.0, 0.0, 500.0)
    a, p = steer_model(g, [0, 0, 0, 7, 0], [6, 0, 1, 0, NO_SLOT], [1.0] * 5, np.array([3, 3, 0, 3, 3], np.uint32),
                       apply=False)
    assert not a.any() and not p.any()
    # a diagonal, step by step: 45 degrees to within the float32 direction's rounding
    g.create(EID[7], 7, 3.0, 0.0, 3.0, 0.0)
    g.enter_space(7, 0, 3.0, 0.0, 3.0)
    a, p = one(7, 1.0)
    assert a.tolist() == [True] and abs(float(p[0, 3]) - 45.0) < 1e-5
    assert p[0, 0] == p[0, 2] == F32(F32(3.0) / F32(np.sqrt(18.0)))
    # applied in message order with both sync flags: the target that also moves is seen where it was
    a, p = steer_model(g, [1, 0], [0, 1], [1.0, 1.0])
    assert p.tolist() == [[9.0, 2.0, 0.0, 270.0], [1.0, 2.0, 0.0, 90.0]]
    assert (g.by_slot[0].x, g.by_slot[1].x, g.by_slot[0].flags, g.by_slot[1].flags) == (1.0, 9.0, 3, 3)
    assert yaw_close([360.0, 0.0, 90.0], [0.0, 360.0, 90.00001]).tolist() == [True, True, True]
    assert yaw_close([90.0, 1.0], [90.0001, 359.0]).tolist() == [False, False]


def edge_world():
    """Eight pairs 1000 apart from each other (D = 100), mover 2k -> target 2k + 1, and a step each:
    four axis-aligned pairs (X = +-1 exactly); a pair 1e-22 apart in x, whose square is a float32
    denormal; a pair 1e-23 apart, whose square is zero; y = -0.0 on a mover; coordinates of
    magnitude 1e6 with a step of 1e-3."""
    big = 1.0e6
    pairs = [((0, 1, 0), (10, 1, 0)), ((1000, 1, 0), (990, 1, 0)), ((2000, 1, 0), (2000, 1, 10)),
             ((3000, 1, 0), (3000, 1, -10)), ((0, 1, 4000), (1e-22, 1, 4000)), ((0, 1, 5000), (1e-23, 1, 5000)),
             ((6000, -0.0, 0), (6003, 5, 4)), ((big, 1, big), (big + 50, 1, big - 50))]
    mv, tg = np.arange(0, 16, 2, dtype=np.uint32), np.arange(1, 16, 2, dtype=np.uint32)
    return pairs, mv, tg, np.array([1, 1, 1, 1, 1, 0.5, 2.5, 1e-3], np.float32)


def test_model_at_the_arithmetic_edges():
    """What the model (and the reference) does at the edges the GPU test compares bit for bit."""
    pairs, mv, tg, steps = edge_world()
    g = GameEntities({0: 100.0}, 16)
    for k, (pa, pb) in enumerate(pairs):
        for s, (x, y, z) in ((2 * k, pa), (2 * k + 1, pb)):
            g.create(EID[s], s, x, y, z, 0.25)
            g.enter_space(s, 0, x, y, z)
    big = F32(1.0e6)
    dx22, dx23 = F32(1e-22), F32(1e-23)
    # 1e-22: the square is a denormal, kept: d != 0 (flushed, the mover would advance by dx * s)
    assert 0 < F32(dx22 * dx22) < F32(1.2e-38) and normalize(dx22, F32(0), F32(0))[3] > 0
    # 1e-23: the square is zero, d == 0 although dx != 0: the direction stays unnormalised
    assert F32(dx23 * dx23) == 0 and dx23 != 0 and normalize(dx23, F32(0), F32(0))[3] == 0
    a, p = steer_model(g, mv, tg, steps, apply=False)
    assert a.all()
    assert p[0].tolist() == [1.0, 1.0, 0.0, 90.0] and p[1].tolist() == [999.0, 1.0, 0.0, 270.0]
    assert p[2].tolist() == [2000.0, 1.0, 1.0, 0.0] and p[3].tolist() == [3000.0, 1.0, -1.0, 180.0]
    # the rounded denormal makes d < |dx|: X = 1.0097 > 1; after the move the target lies behind
    d22 = normalize(dx22, F32(0), F32(0))[3]
    assert p[4, 0] == F32(dx22 / d22) and 1.0 < p[4, 0] < 1.02 and p[4, 3] == 270.0
    assert p[5, 0] == F32(dx23 * F32(0.5)) != 0 and p[5, 2] == 5000.0
    # -0.0 + 0 * 2.5 = +0.0; with a negative step 0 * s = -0.0 and the sign stays
    assert p[6, :3].tolist() == [6001.5, 0.0, 2.0] and not np.signbit(p[6, 1])
    neg = steer_model(g, [12], [13], [-1.0], np.array([MOVE], np.uint32), apply=False)[1]
    assert np.signbit(neg[0, 1]) and neg[0, 1] == 0
    # the step is absorbed: x and z unchanged, a Moved is queued all the same
    assert p[7, 0] == big and p[7, 2] == big and abs(float(p[7, 3]) - 135.0) < 1e-4
    # FACE alone 1e-22 apart: acos(1.0097) is NaN in the reference; the message does not apply
    a, p = steer_model(g, mv[4:6], tg[4:6], steps[4:6], np.array([FACE, FACE], np.uint32), apply=False)
    assert a.tolist() == [False, True] and not p[0].any() and abs(float(p[1, 3])) < 1e-4


CLASSES = [("chase", 60), ("face", 20), ("move", 20), ("overshoot", 10), ("negative", 10), ("zero_step", 5),
           ("zero_flags", 5), ("unrelated", 30), ("cross", 10), ("self", 10), ("no_slot", 10), ("target_outside", 10),
           ("mover_outside", 10), ("unbound_mover", 1), ("unbound_target", 1)]
RELATED = ("chase", "face", "move", "overshoot", "negative", "zero_step", "zero_flags")


def scenario_messages(i, g, n):
    """The 212 distinct-mover messages drawn after flush i, by class, shuffled."""
    rng = np.random.default_rng(4000 + i)
    inside = [s for s in range(n) if g.by_slot[s].aoi]
    outside = [s for s in range(n) if not g.by_slot[s].aoi]
    pool = [int(s) for s in rng.permutation(inside)]
    social = [s for s in pool if g.by_slot[s].In]
    used = set()

    def take(src):
        s = next(s for s in src if s not in used)
        used.add(s)
        return s

    msgs = []
    for name, count in CLASSES:
        for _ in range(count):
            fl, step = MOVE | FACE, F32(rng.uniform(0, 3))
            if name in RELATED:
                a = take(social)
                b = int(rng.choice(sorted(g.by_slot[a].In)))
                if name == "chase" and rng.random() < 0.5:
                    step = F32(0.06)  # Monster.GetSpeed() * 30 / 1000
                fl = {"face": FACE, "move": MOVE, "zero_flags": 0}.get(name, fl)
                step = {"overshoot": F32(250.0), "negative": -step, "zero_step": F32(0)}.get(name, step)
            elif name == "unrelated":
                a = take(pool)
                ea = g.by_slot[a]
                b = int(rng.choice([s for s in inside if g.by_slot[s].space == ea.space and s != a and s not in ea.In]))
            elif name == "cross":
                a = take(pool)
                b = int(rng.choice([s for s in inside if g.by_slot[s].space != g.by_slot[a].space]))
            elif name == "self":
                a = b = take(pool)
            elif name == "no_slot":
                a, b = take(pool), NO_SLOT
            elif name == "target_outside":
                a, b = take(pool), int(rng.choice(outside))
            elif name == "mover_outside":
                a, b = take([int(s) for s in rng.permutation(outside)]), int(rng.choice(inside))
            elif name == "unbound_mover":
                a, b = n + 1, int(rng.choice(inside))
            else:
                a, b = take(pool), n + 2
            msgs.append((name, a, b, step, fl))
    order = rng.permutation(len(msgs))
    msgs = [msgs[k] for k in order]
    return ([m[0] for m in msgs], np.array([m[1] for m in msgs], np.uint32), np.array([m[2] for m in msgs], np.uint32),
            np.array([m[3] for m in msgs], np.float32), np.array([m[4] for m in msgs], np.uint32))


@functools.lru_cache(maxsize=None)
def scenario_expected():
    """The scenario and, per flush, the messages, the model's answers and what the steered flush
    must give: the movers' rows, the net events and the collect (computed once on the restatement,
    shared and left unchanged by the tests)."""
    sc = SS.make(seed=21, n=600, flushes=4)
    n = sc["n"]
    exp = []

    def on_flush(i, g):
        g.take_raw()  # (the scenario's own flush: tests/test_sync.py's ground)
        pre = g.collect()  # (its records are collected first: the next collect holds the steered moves' alone)
        names, mv, tg, st, fl = scenario_messages(i, g, n)
        applied, pos = steer_model(g, mv, tg, st, fl)
        raw = g.take_raw()
        ent, lev = oracle.net_events(*raw)
        rows = [sorted(g.by_slot[int(s)].In) if int(s) in g.by_slot else [] for s in mv]
        exp.append({"names": names, "msg": (mv, tg, st, fl), "answers": (applied, pos), "enter": ent, "leave": lev,
                    "rows": rows, "pre": pre, "sync": g.collect(), "callbacks": int(raw[0].size),
                    "targets_moving": int(np.isin(tg, mv).sum()), "nan": int(np.isnan(pos).sum())})

    g = SS.run_oracle(sc, on_flush)
    return sc, exp, {s: e.eid for s, e in g.by_slot.items()}


def test_scenario_covers_every_class_of_message():
    """Checked on the restatement (no GPU): after each of the 5 flushes the draw has 212 messages
    of every class with distinct movers, 125 of which apply (the seven related classes but the
    zero flags), targets that are themselves movers, moves that cross windows (enter and leave
    events) and collect records, and no NaN: a scenario change cannot hollow the GPU tests out."""
    sc, exp, _ = scenario_expected()
    assert len(exp) == len(sc["flushes"]) + 1 == 5
    for e in exp:
        mv, tg, st, fl = e["msg"]
        applied = e["answers"][0]
        count = {k: e["names"].count(k) for k, _ in CLASSES}
        print(count, int(applied.sum()), e["callbacks"], len(e["enter"]), len(e["leave"]),
              sum(len(v) for v in e["sync"].values()), e["targets_moving"])
        assert count == dict(CLASSES) and len(mv) == 212 == len(set(mv.tolist()))
        assert int(applied.sum()) == 125
        by = np.array(e["names"])
        assert applied[np.isin(by, RELATED[:-1])].all() and not applied[~np.isin(by, RELATED[:-1])].any()
        assert 69 <= e["targets_moving"] <= 88 and e["nan"] == 0
        assert 366 <= e["callbacks"] <= 566 and len(e["enter"]) > 0 and len(e["leave"]) > 0
        assert 1203 <= sum(len(v) for v in e["sync"].values()) <= 1327  # (the steered moves' records alone)
        assert {0.06, 250.0, 0.0} <= set(np.round(st.astype(np.float64), 6).tolist()) and (st < 0).any()


# ------------------------------------------------------------------ GPU ------

def _dev(a, dtype=np.uint32):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype).view(np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def device_steer(w, movers, targets, steps, flags=None, d_targets=None):
    """steer_batch_device on torch tensors -> (code, applied, pos); the outputs are read back
    whatever the code (the device form delivers the other messages with an error)."""
    import torch
    from goworld_amd import GwaoiError
    mv, st = _dev(movers), _dev(steps, np.float32)
    tg = _dev(targets) if d_targets is None else None
    fl = _dev(flags) if flags is not None else None
    n = mv.numel()
    oa = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda:0")
    op = torch.full((max(n, 1), 4), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    code = 0
    try:
        w.steer_batch_device(mv.data_ptr(), tg.data_ptr() if tg is not None else d_targets, st.data_ptr(),
                             fl.data_ptr() if fl is not None else 0, n, oa.data_ptr(), op.data_ptr())
    except GwaoiError as e:
        code = e.code
    return code, oa.cpu().numpy()[:n].astype(bool), op.cpu().numpy()[:n]


def host_steer(w, movers, targets, steps, flags=None):
    return (0,) + w.steer_batch(movers, targets, steps, flags)


def rows_of(w, slots):
    off, items = w.neighbors_batch(slots)
    return [sorted(items[off[m]:off[m + 1]].tolist()) for m in range(len(off) - 1)]


def scenario_run(steer):
    from goworld_amd import World, pair_keys
    sc, exp, eids = scenario_expected()
    n = sc["n"]
    yaw_fix = {}
    seen = []

    def on_flush(i, w, ent=None, lev=None):
        e = exp[i]
        mv, tg, st, fl = e["msg"]
        assert records_by_gate(w.collect_sync_infos()) == with_gpu_yaw(e["pre"], yaw_fix), f"flush {i}: the scenario's records"
        code, applied, pos = steer(w, mv, tg, st, fl)
        assert code == 0
        check_answers((applied, pos), e["answers"], f"flush {i}", mv, yaw_fix, eids)
        ent2, lev2 = w.tick()
        assert np.array_equal(pair_keys(ent2), e["enter"]), f"flush {i}: enter pairs of the steered moves"
        assert np.array_equal(pair_keys(lev2), e["leave"]), f"flush {i}: leave pairs of the steered moves"
        assert rows_of(w, mv) == e["rows"], f"flush {i}: the movers' rows"
        got = records_by_gate(w.collect_sync_infos())
        assert got == with_gpu_yaw(e["sync"], yaw_fix), f"flush {i}: sync records"
        seen.append(int(applied.sum()))

    with World(n + 8, max_spaces=4, device=0) as w:
        SS.run_gpu(sc, w, on_flush)
    assert seen == [125] * 5


@pytest.mark.gpu
def test_steer_scenario_host_form_matches_model():
    """After every flush of the scenario: 212 messages of every class, the answers against the
    model, then the flush: the movers' rows, the net events and the sync collect."""
    scenario_run(host_steer)


@pytest.mark.gpu
def test_steer_scenario_device_form_matches_model():
    """The same on a second world with every array in device memory."""
    scenario_run(device_steer)


@functools.lru_cache(maxsize=None)
def loop_expected():
    """The closed loop's chained models: nearest (tests/test_interest_query.py's) -> steer."""
    sc = SS.make(seed=22, n=600, flushes=2)
    n = sc["n"]
    tags = scenario_tags(n)
    monsters = np.flatnonzero((tags[:n] & 1) != 0).astype(np.uint32)  # "type" bit 1 chases "type" bit 2
    mask = np.full(monsters.size, 2, np.uint32)
    steps = np.full(monsters.size, 0.06, np.float32)
    exp = []

    def on_flush(i, g):
        near, dist, _ = nearest_model(g, tags, monsters, mask, mask)
        applied, pos = steer_model(g, monsters, near, steps)
        exp.append({"near": near, "answers": (applied, pos), "sync": g.collect()})

    g = SS.run_oracle(sc, on_flush)
    return sc, tags, monsters, mask, steps, exp, {s: e.eid for s, e in g.by_slot.items()}


@pytest.mark.gpu
def test_steer_closed_loop_on_the_device():
    """Monster.AI -> Monster.Tick without a position on the host: nearest_batch_device's output,
    GWAOI_NO_SLOT entries included, goes straight to steer_batch_device as the targets; then the
    flush and collect_sync_infos_device, against the chained models."""
    import torch
    from goworld_amd import World
    sc, tags, monsters, mask, steps, exp, eids = loop_expected()
    n = sc["n"]
    yaw_fix = {}
    assert all((e["near"] == NO_SLOT).any() and e["answers"][0].sum() > 50 for e in exp)

    def on_flush(i, w, ent=None, lev=None):
        e = exp[i]
        if i == 0:
            w.entity_set_tag(np.arange(n), tags[:n])
        dq, dm = _dev(monsters), _dev(mask)
        d_near = torch.zeros(monsters.size, dtype=torch.int32, device="cuda:0")
        d_dist = torch.zeros(monsters.size, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        w.nearest_batch_device(dq.data_ptr(), dm.data_ptr(), dm.data_ptr(), monsters.size, d_near.data_ptr(),
                               d_dist.data_ptr())
        code, applied, pos = device_steer(w, monsters, None, steps, d_targets=d_near.data_ptr())
        assert code == 0
        assert np.array_equal(d_near.cpu().numpy().view(np.uint32), e["near"])
        check_answers((applied, pos), e["answers"], f"flush {i}", monsters, yaw_fix, eids)
        w.tick()
        ids, off, ptr = w.collect_sync_infos_device()
        raw = np.frombuffer(_d2h(ptr, 48 * off[-1]), np.uint8).reshape(-1, 48)
        got = records_by_gate({g: raw[off[k]:off[k + 1]] for k, g in enumerate(ids)})
        assert got == with_gpu_yaw(e["sync"], yaw_fix), f"flush {i}: device sync records"

    with World(n, max_spaces=4, device=0) as w:
        SS.run_gpu(sc, w, on_flush)


def build_pairs(w, g, sp, pairs, D_key=0):
    """Entities 2k (mover) and 2k + 1 (target) of pairs[k] = ((x, y, z), (x, y, z)) in space sp / D_key."""
    for k, (pa, pb) in enumerate(pairs):
        for s, (x, y, z) in ((2 * k, pa), (2 * k + 1, pb)):
            w.entity_bind([s], [EID[s]])
            w.entity_set_client(s, 1, CID[s])
            w.entity_set_position_yaw(s, x, y, z, 0.25)
            w.enter(sp, s, x, z)
            g.create(EID[s], s, x, y, z, 0.25)
            g.set_client(s, 1, CID[s])
            g.enter_space(s, D_key, x, y, z)


@pytest.mark.gpu
def test_steer_arithmetic_edges():
    """The edge pairs (edge_world, checked on the model by test_model_at_the_arithmetic_edges) on
    the GPU, bit for bit: MOVE | FACE and MOVE alone for all eight, FACE alone without the 1e-22
    pair (its X exceeds 1: test_steer_errors_leave_the_world_usable), and a negative step on
    y = -0.0.  Every round is flushed, collected and compared, then everyone is put back."""
    from goworld_amd import World
    pairs, mv, tg, steps = edge_world()
    g = GameEntities({0: 100.0}, 16)
    keep = np.array([0, 1, 2, 3, 5, 6, 7])
    rounds = [(np.arange(8), steps, None), (np.arange(8), steps, np.full(8, MOVE, np.uint32)),
              (keep, steps[keep], np.full(7, FACE, np.uint32)),
              (np.array([6]), np.array([-1.0], np.float32), np.array([MOVE], np.uint32))]
    with World(16, device=0) as w:
        sp = w.space_create(100.0)
        build_pairs(w, g, sp, pairs)
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()
        for k, st, flags in rounds:
            want = steer_model(g, mv[k], tg[k], st, flags)
            got = w.steer_batch(mv[k], tg[k], st, flags)
            check_answers(got, want, f"flags {flags}")
            assert want[0].all()
            w.tick()
            assert records_by_gate(w.collect_sync_infos()) == g.collect()
            for q, (pa, pb) in enumerate(pairs):
                w.set_position_yaw(2 * q, *pa, 0.25)
                g.set_position_yaw(2 * q, *pa, 0.25)
            w.tick()
            assert records_by_gate(w.collect_sync_infos()) == g.collect()
        assert np.signbit(got[1][0, 1]) and got[1][0, 1] == 0  # (the last round: -0.0 + -0.0)


def packet(slot, x, y, z, yaw):
    return EID[slot] + struct.pack("<4f", x, y, z, yaw)


@pytest.mark.gpu
@pytest.mark.parametrize("later", ["set_position_yaw", "packet"])
def test_steer_ordering_and_claims(later):
    """Steer, then a host Moved of another entity and a later write of one of the movers (a host
    set_position_yaw, or a client packet), then one flush: the relation's ownership follows the
    sequential order and the later write wins for position and yaw alike, as the sequential calls
    of the model leave it."""
    from goworld_amd import World, pair_keys
    pairs = [((0, 1, 0), (30, 1, 0)), ((0, 2, 60), (40, 2, 60)), ((200, 3, 0), (200, 3, 90)), ((95, 4, 95), (60, 4, 60))]
    mv, tg = np.arange(0, 8, 2, dtype=np.uint32), np.arange(1, 8, 2, dtype=np.uint32)
    steps = np.array([5, 120, 2, 7], np.float32)
    g = GameEntities({0: 100.0}, 16)
    with World(16, device=0) as w:
        sp = w.space_create(100.0)
        build_pairs(w, g, sp, pairs)
        w.entity_set_syncing(2, True)
        g.set_syncing(2, True)
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()
        g.take_raw()
        want = steer_model(g, mv, tg, steps)
        check_answers(w.steer_batch(mv, tg, steps), want, later)
        assert want[0].all()
        # another entity moves after the steer (its seq is later: it owns its windows now) ...
        w.moved(5, 150.0, 60.0)
        g.set_position_yaw(5, 150.0, 0.0, 60.0, 0.25)
        g.by_slot[5].y, g.by_slot[5].flags = F32(3.0), 0  # (a bare Moved: no Position, no flag)
        # ... and mover 2 is written again: the later write wins for position and yaw
        if later == "set_position_yaw":
            w.set_position_yaw(2, 111.0, 7.0, 61.0, 33.0)
            g.set_position_yaw(2, 111.0, 7.0, 61.0, 33.0)
        else:
            w.sync_from_clients(packet(2, 111.0, 7.0, 61.0, 33.0))
            g.handle_sync_packet(packet(2, 111.0, 7.0, 61.0, 33.0))
        ent, lev = w.tick()
        e_ent, e_lev = oracle.net_events(*g.take_raw())
        assert np.array_equal(pair_keys(ent), e_ent) and np.array_equal(pair_keys(lev), e_lev)
        assert len(e_ent) + len(e_lev) > 0
        assert rows_of(w, np.arange(8)) == [sorted(g.by_slot[s].In) for s in range(8)]
        exp = g.collect()
        assert records_by_gate(w.collect_sync_infos()) == exp
        rec2 = CID[2] + EID[2] + struct.pack("<4f", 111.0, 7.0, 61.0, 33.0)
        assert rec2 in exp[1]
        # the steered position of mover 0 and the later write of mover 2 are what the next steer reads
        want = steer_model(g, [0, 2], [1, 5], [1.0, 1.0])
        check_answers(w.steer_batch([0, 2], [1, 5], [1.0, 1.0]), want, "the next steer")
        assert want[0][0]
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()


@pytest.mark.gpu
def test_steer_errors_leave_the_world_usable():
    """Every error is followed by a good call whose answers are checked."""
    import ctypes as C

    from goworld_amd import GwaoiError, World
    n = 16
    pairs = [((0, 1, 0), (30, 1, 0)), ((0, 2, 60), (40, 2, 60)), ((200, 3, 0), (200, 3, 90))]
    g = GameEntities({0: 100.0, 1: 1.0e36}, n)

    def good(w):
        """Movers 0 and 2 step 1 toward their targets; flush; the collect equals the model's."""
        want = steer_model(g, [0, 2], [1, 3], [1.0, 1.0])
        check_answers(w.steer_batch([0, 2], [1, 3], [1.0, 1.0]), want, "good call")
        assert want[0].all()
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()

    def raises(code, f, *args):
        with pytest.raises(GwaoiError) as ei:
            f(*args)
        assert ei.value.code == code
        return ei.value

    with World(n, max_spaces=2, device=0) as w:
        sp = w.space_create(100.0)
        huge = w.space_create(1.0e36)
        build_pairs(w, g, sp, pairs)
        # ops queued since the last flush (the enters), then a flush in flight
        raises(ESTATE, w.steer_batch, [0], [1], [1.0])
        assert device_steer(w, [0], [1], [1.0])[0] == ESTATE
        w.tick_begin()
        raises(ESTATE, w.steer_batch, [0], [1], [1.0])
        w.tick_end()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()
        good(w)
        # a second steer call before the flush; a read and a collect before it, too
        want = steer_model(g, [4], [5], [2.0])
        check_answers(w.steer_batch([4], [5], [2.0]), want, "first of two")
        raises(ESTATE, w.steer_batch, [0], [1], [1.0])
        raises(ESTATE, w.related_batch, [0], [1])
        raises(ESTATE, w.collect_sync_infos)
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()
        good(w)
        # host form: nothing happens on an error
        raises(EINVAL, w.steer_batch, [0, 2, 0], [1, 3, 1], [1.0, 1.0, 1.0])          # a repeated mover
        raises(EINVAL, w.steer_batch, [0, 2], [1, 3], [1.0, 1.0], [3, 4])             # a bad flag bit
        raises(EBADSLOT, w.steer_batch, [0, n], [1, 3], [1.0, 1.0])
        raises(EBADSLOT, w.steer_batch, [0, 2], [1, n], [1.0, 1.0])
        raises(EBADSLOT, w.steer_batch, [0, 2], [1, 0xFFFFFFFE], [1.0, 1.0], [3, 4])  # (precedence)
        raises(ENONFINITE, w.steer_batch, [0, 2], [1, 3], [1.0, np.inf])
        raises(ENONFINITE, w.steer_batch, [0, 2], [1, 3], [np.nan, 1.0])
        raises(EINVAL, w.steer_batch, [0, 0], [1, 1], [np.nan, 1.0])                  # (precedence)
        assert w.steer_batch([0], [NO_SLOT], [1.0])[0].tolist() == [False]            # GWAOI_NO_SLOT is no error
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect() == {}
        good(w)
        # null arguments with n > 0
        L, h = w._L, w._w
        q = np.zeros(4, np.uint32)
        qp = q.ctypes.data_as(C.c_void_p)
        for k in (1, 2, 3, 6, 7):
            args = [h, qp, qp, qp, None, 1, qp, qp]
            args[k] = None
            assert L.gwaoi_steer_batch(*args) == EINVAL and L.gwaoi_steer_batch_device(*args) == EINVAL
        good(w)
        # n == 0: nothing, in either form, and not a queued op
        a, p = w.steer_batch([], [], [])
        assert a.size == 0 and p.shape == (0, 4)
        w.steer_batch_device(0, 0, 0, 0, 0, 0, 0)
        assert w.related_batch([0], [1]).tolist() == [True]
        good(w)
        # device form: the offending message is dropped, the others are delivered with the code
        for code, mv, tg, st, fl in (
                (EBADSLOT, [0, n, 2], [1, 3, 3], [1.0, 1.0, 1.0], None),
                (EBADSLOT, [0, 4, 2], [1, n + 5, 3], [1.0, 1.0, 1.0], [3, 4, 3]),
                (EINVAL, [0, 4, 2], [1, 5, 3], [1.0, np.inf, 1.0], [3, 8, 3]),
                (ENONFINITE, [0, 4, 2], [1, 5, 3], [1.0, np.inf, 1.0], None),
                (ENONFINITE, [0, 4, 2], [1, 5, 3], [1.0, np.nan, 1.0], None)):
            keep = [0, 2]
            want = steer_model(g, [0, 2], [1, 3], [1.0, 1.0])
            got = device_steer(w, mv, tg, st, fl)
            assert got[0] == code and got[1].tolist() == [True, False, True] and not got[2][1].any()
            check_answers((got[1][keep], got[2][keep]), want, f"device form, {code}")
            w.tick()
            assert records_by_gate(w.collect_sync_infos()) == g.collect()
        good(w)
        # a repeated mover in the device form: exactly one of its messages applies, the call
        # returns EINVAL and the state equals the model run with that one message
        mv, tg, st = [0, 2, 0, 0], [1, 3, 1, 1], [1.0, 1.0, 2.0, 3.0]
        code, applied, pos = device_steer(w, mv, tg, st)
        assert code == EINVAL and applied[1] and applied[[0, 2, 3]].sum() == 1
        won = [1, int(np.flatnonzero(applied & (np.array(mv) == 0))[0])]
        want = steer_model(g, [mv[k] for k in won], [tg[k] for k in won], [st[k] for k in won])
        check_answers((applied[won], pos[won]), want, "repeated mover")
        assert not pos[~applied].any()
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()
        good(w)
        # coordinates near 3.3e38 in a space with D = 1e36, 5e35 apart: dx * dx overflows, d = +inf
        # and the direction becomes (0, 0, 0): the message applies, the position stays, acos(0) gives
        # yaw 0.  No step makes x' overflow there: |nx| <= 1 needs dx * dx finite, so |x| < 3e26.
        x0 = F32(3.3e38)
        for s, x in ((8, x0), (9, F32(3.305e38))):
            w.entity_bind([s], [EID[s]])
            w.entity_set_client(s, 1, CID[s])
            w.entity_set_position_yaw(s, x, 1.0, 0.0, 0.25)
            w.enter(huge, s, x, 0.0)
            g.create(EID[s], s, x, 1.0, 0.0, 0.25)
            g.set_client(s, 1, CID[s])
            g.enter_space(s, 1, x, 1.0, 0.0)
        # 1e-22 apart: fl(dx * dx) is a denormal rounded down, so d < |dx| and X = 1.0097 > 1
        for s, x in ((12, 0.0), (13, 1e-22)):
            w.entity_bind([s], [EID[s]])
            w.entity_set_client(s, 1, CID[s])
            w.entity_set_position_yaw(s, x, 1.0, 900.0, 0.25)
            w.enter(sp, s, x, 900.0)
            g.create(EID[s], s, x, 1.0, 900.0, 0.25)
            g.set_client(s, 1, CID[s])
            g.enter_space(s, 0, x, 1.0, 900.0)
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()
        want = steer_model(g, [8], [9], [2.0e37])
        assert want[0].tolist() == [True] and want[1][0].tolist() == [x0, 1.0, 0.0, 0.0]
        check_answers(w.steer_batch([8], [9], [2.0e37]), want, "squares overflow")
        w.tick()
        assert records_by_gate(w.collect_sync_infos()) == g.collect()
        # overflow to inf: X = 1.0097 times the largest float32 step.  Dropped with ENONFINITE in both
        # forms, the sync record unchanged (no flag, no record of mover 12 in the next collect), the
        # other message of the call delivered.  The same with FACE alone: the reference's acos(X > 1)
        # is NaN, and a NaN yaw is refused like a non-finite position.
        big = np.finfo(np.float32).max
        for form, fl in (("host", None), ("device", None), ("host", np.array([FACE, FACE], np.uint32)),
                         ("device", np.array([FACE, FACE], np.uint32))):
            mv, tg, st = [12, 0], [13, 1], [big, 1.0]
            with np.errstate(all="ignore"):
                assert not np.isfinite(steer_one(g.by_slot[12], g.by_slot[13], big, MOVE)[0])
                assert np.isnan(steer_one(g.by_slot[12], g.by_slot[13], big, FACE)[3])
            want = steer_model(g, mv, tg, st, fl)
            assert want[0].tolist() == [False, True]
            if form == "host":
                got = raises(ENONFINITE, w.steer_batch, mv, tg, st, fl).result
            else:
                code, *got = device_steer(w, mv, tg, st, fl)
                assert code == ENONFINITE
            check_answers(got, want, f"overflow, {form} form, flags {fl}")
            w.tick()
            exp = g.collect()
            assert records_by_gate(w.collect_sync_infos()) == exp
            assert not any(r[16:32] == EID[12] for r in exp.get(1, [])) and any(r[16:32] == EID[0] for r in exp[1])
        good(w)
