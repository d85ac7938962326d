"""Time gwaoi_steer_batch (Monster.Tick's chase and FaceTo on the GPU) on the cfg3 world.

    python tools/steer_bench.py [--n N] [--reps 40] [--warmup 5] [--out profiles/steer_bench.json]

Builds the cfg3 world (1M entities in one space), flushes once, then for 1 / 64 / 4,096 / 65,536
messages (distinct movers, targets taken from a prior nearest_batch, a step of 0.06) times, per
repetition and alternating call by call:

  device form   movers, targets, steps and the answers in HBM: HIP events on the world's stream
                around the call plus a host clock around it (the call ends in a stream
                synchronise), then its tick (host clock);
  host form     numpy in, numpy out through the binding (host clock), then its tick;
  baseline      the path the call replaces, through the same binding: `related_batch` for the
                gate, the reference's arithmetic in vectorised numpy float32 on positions held by
                the host, then one `set_position_yaw` per applied mover; then its tick.  Its three
                parts are reported separately: the per-call ctypes cost of the third is one a cgo
                adapter would not pay in full.

Every path starts from the state the previous one left (the host's positions are refreshed from
the answers outside the timed windows), and every tick is followed by an untimed
`collect_sync_infos_device`, as a game's loop does: the library uploads pending host writes with the
next sync call, so without it the 40 B per `set_position_yaw` of the baseline would be uploaded
inside the steer call that follows and be charged to the new path.  That upload is charged to
nobody here.  On the last repetition the baseline's arithmetic is run
on the host form's snapshot and compared with its answers: positions bit for bit, yaw to within
one float32 ulp modulo 360.  Per size: warm-up repetitions first, then the median and p99 of
`--reps`.  `beats_baseline_by_more_than_its_spread` is
(baseline median - new median) > (baseline max - baseline min) of that session.

Algorithmic bytes per message, from the shapes (BYTES_PER_MESSAGE below), over the call time = a
whole-call rate (not a kernel's share of peak).

Needs a GPU: there is no CPU path.  Prints one JSON document (and writes --out).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.broadcast_bench import stats  # noqa: E402

SIZES = (1, 64, 4096, 65536)
NO_SLOT = 0xFFFFFFFF
STEP = np.float32(2 * 30 / 1000.0)  # Monster.GetSpeed() * 30 / 1000
F32 = np.float32

# what one message moves, from the shapes of k_steer and k_steer_apply
BYTES_PER_MESSAGE = {
    "message (mover, target, step, flags) read": 16,
    "two ranks read": 2 * 4,
    "two frame entries (slot, space) read": 2 * 8,
    "two frame records (x, z, seq) read": 2 * 16,
    "slot record read (space, y, yaw; flags in the apply)": 16,
    "slot record written (Position, yaw, flags)": 20,
    "claims written and compared": 16 + 8,
    "batch entry (slot, x, z, space, mover) written, mover read": 20 + 4,
    "outputs (applied, x, y, z, yaw) written, the position read by the apply": 17 + 16,
}


def host_arithmetic(ax, ay, az, bx, bz, s):
    """The reference's MOVE then FACE in vectorised numpy float32, step by step (the baseline's
    second part): new x, y, z and yaw of every mover."""
    def normalize(x, y, z):
        d = np.sqrt((((x * x + y) + y) + z * z).astype(np.float64)).astype(np.float32)
        ok = d != 0
        dd = np.where(ok, d, F32(1))
        return np.where(ok, x / dd, x), np.where(ok, y / dd, y), np.where(ok, z / dd, z)

    zero = np.zeros_like(ax)
    nx, ny, nz = normalize(bx - ax, zero, bz - az)
    x, y, z = ax + nx * s, ay + ny * s, az + nz * s
    fx, _, fz = normalize(bx - x, zero, bz - z)
    yaw = np.arccos(fx.astype(np.float64))
    yaw = np.where(fz < 0, np.pi * 2 - yaw, yaw)
    yaw = yaw / np.pi * 180.0
    yaw = np.where(yaw <= 90, 90 - yaw, 90 + (360 - yaw))
    return x, y, z, yaw.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=0, help="entities (0: cfg3's 1M)")
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions per size (>= 30)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed repetitions per size first")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("steer_bench needs a GPU (no CPU path)")
    from goworld_amd import World
    from goworld_amd.workload import make_workload

    wl = make_workload("cfg3", n=args.n or None)
    n = wl.n
    rng = np.random.default_rng(0x57EE)
    np.seterr(all="ignore")  # (acos of the reference's X > 1 corner is NaN by design)
    w = World(n, device=0)
    sp = w.space_create(float(wl.D))
    slots, x0, z0, _ = wl.initial()
    # the host's copy of the positions: what the baseline needs and the new path does not
    px, py, pz, pyaw = (np.zeros(n, np.float32) for _ in range(4))
    px[slots], pz[slots] = x0, z0
    w.enter_batch(sp, slots, x0, z0)
    w.tick_device()
    w.collect_sync_infos_device()
    w.sync()
    stream = torch.cuda.ExternalStream(w.stream())
    per_msg = sum(BYTES_PER_MESSAGE.values())
    out = {"tool": "tools/steer_bench.py", "workload": "cfg3", "n": n, "D": float(wl.D), "step": float(STEP),
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "bytes_per_message": dict(BYTES_PER_MESSAGE, total=per_msg), "sizes": []}

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a = time.perf_counter()
        e0.record(stream)
        r = f()
        e1.record(stream)
        e1.synchronize()
        b = time.perf_counter()
        return e0.elapsed_time(e1), (b - a) * 1e3, r

    def walled(f):
        a = time.perf_counter()
        r = f()
        return (time.perf_counter() - a) * 1e3, r

    def refresh(mv, applied, pos):
        m = mv[applied]
        px[m], py[m], pz[m], pyaw[m] = pos[applied, 0], pos[applied, 1], pos[applied, 2], pos[applied, 3]

    for k in SIZES:
        if k > n:
            continue
        mv = rng.choice(n, k, replace=False).astype(np.uint32)
        tg, _ = w.nearest_batch(mv)
        steps = np.full(k, STEP, np.float32)
        d_mv = torch.from_numpy(mv.view(np.int32).copy()).to("cuda:0")
        d_tg = torch.from_numpy(tg.view(np.int32).copy()).to("cuda:0")
        d_st = torch.from_numpy(steps).to("cuda:0")
        d_ap = torch.zeros(k, dtype=torch.uint8, device="cuda:0")
        d_pos = torch.zeros((k, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        T = {key: [] for key in ("dev_events", "dev_wall", "dev_tick", "host_wall", "host_tick", "base_related",
                                 "base_arith", "base_set", "base_tick")}
        has = tg != NO_SLOT
        tgc = np.where(has, tg, 0)
        applied_counts = []
        checked = False

        def baseline_compute():
            t_rel, rel = walled(lambda: w.related_batch(mv[has], tg[has]))
            on = np.zeros(k, bool)
            on[has] = rel
            t_ar, new = walled(lambda: host_arithmetic(px[mv], py[mv], pz[mv], px[tgc], pz[tgc], steps))
            return t_rel, t_ar, on, new

        for rep in range(args.warmup + args.reps):
            rec = rep >= args.warmup
            # device form, then its tick
            e, t, _ = timed(lambda: w.steer_batch_device(d_mv.data_ptr(), d_tg.data_ptr(), d_st.data_ptr(), 0, k,
                                                         d_ap.data_ptr(), d_pos.data_ptr()))
            tt, _ = walled(w.tick_device)
            w.collect_sync_infos_device()
            refresh(mv, d_ap.cpu().numpy().astype(bool), d_pos.cpu().numpy())
            if rec:
                T["dev_events"].append(e)
                T["dev_wall"].append(t)
                T["dev_tick"].append(tt)
            # host form, then its tick; on the last repetition the baseline's arithmetic on the same snapshot
            last = rep == args.warmup + args.reps - 1
            if last:
                _, _, b_on, b_new = baseline_compute()
            t, (applied, pos) = walled(lambda: w.steer_batch(mv, tg, steps))
            tt, _ = walled(w.tick_device)
            w.collect_sync_infos_device()
            if last:
                assert np.array_equal(applied, b_on), "baseline and steer_batch disagree on the gate"
                for c in range(3):
                    assert np.array_equal(pos[applied, c].view(np.uint32), b_new[c][applied].view(np.uint32)), \
                        "baseline and steer_batch disagree on a position"
                d = np.abs(pos[applied, 3].astype(np.float64) - b_new[3][applied].astype(np.float64))
                d = np.minimum(d, np.abs(360.0 - d))
                assert (d <= np.spacing(np.abs(b_new[3][applied])).astype(np.float64) + 1e-12).all(), "yaw"
                checked = True
            refresh(mv, applied, pos)
            applied_counts.append(int(applied.sum()))
            if rec:
                T["host_wall"].append(t)
                T["host_tick"].append(tt)
            # the baseline: gate, arithmetic on the host's positions, one call per applied mover, then its tick
            t_rel, t_ar, on, new = baseline_compute()
            bx, by, bz, byaw = new

            def set_all():
                for m in np.flatnonzero(on):
                    w.set_position_yaw(int(mv[m]), bx[m], by[m], bz[m], byaw[m])
            t_set, _ = walled(set_all)
            tt, _ = walled(w.tick_device)
            w.collect_sync_infos_device()  # (uploads the set_position_yaw writes: see the head comment)
            refresh(mv, on, np.stack(new, axis=1))
            if rec:
                T["base_related"].append(t_rel)
                T["base_arith"].append(t_ar)
                T["base_set"].append(t_set)
                T["base_tick"].append(tt)
        A = {key: np.asarray(v) for key, v in T.items()}
        base_call = A["base_related"] + A["base_arith"] + A["base_set"]
        sb, sbt = stats(base_call), stats(base_call + A["base_tick"])
        spread, spread_t = sb["max_ms"] - sb["min_ms"], sbt["max_ms"] - sbt["min_ms"]
        sd, sdt = stats(A["dev_wall"]), stats(A["dev_wall"] + A["dev_tick"])
        sh, sht = stats(A["host_wall"]), stats(A["host_wall"] + A["host_tick"])
        row = {
            "messages": k, "targets_found": int(has.sum()), "applied_min": min(applied_counts),
            "applied_max": max(applied_counts), "answers_equal_baseline": checked,
            "algorithmic_bytes": k * per_msg,
            "device_form": {"events": stats(A["dev_events"]), "wall": sd, "wall_with_tick": sdt,
                            "whole_call_GBps_events": k * per_msg / (stats(A["dev_events"])["median_ms"] * 1e-3) / 1e9},
            "host_form": {"wall": sh, "wall_with_tick": sht},
            "baseline": {"path": "related_batch + numpy float32 on host positions + set_position_yaw per applied mover (ctypes)",
                         "related_batch": stats(A["base_related"]), "arithmetic": stats(A["base_arith"]),
                         "set_position_yaw": stats(A["base_set"]), "wall": sb, "wall_with_tick": sbt,
                         "spread_ms": spread, "spread_with_tick_ms": spread_t},
            "ratio_median": {"device_form": sb["median_ms"] / sd["median_ms"], "host_form": sb["median_ms"] / sh["median_ms"],
                             "device_form_with_tick": sbt["median_ms"] / sdt["median_ms"],
                             "host_form_with_tick": sbt["median_ms"] / sht["median_ms"]},
            "beats_baseline_by_more_than_its_spread": {
                "device_form": bool(sb["median_ms"] - sd["median_ms"] > spread),
                "host_form": bool(sb["median_ms"] - sh["median_ms"] > spread),
                "device_form_with_tick": bool(sbt["median_ms"] - sdt["median_ms"] > spread_t),
                "host_form_with_tick": bool(sbt["median_ms"] - sht["median_ms"] > spread_t)},
        }
        out["sizes"].append(row)
        print(f"{k} messages done", file=sys.stderr, flush=True)
    out["note"] = ("wall = host clock around the call (it ends in a stream synchronise); events = HIP events on the "
                   "world's stream around the device-form call; *_with_tick adds the tick that follows, call by call; "
                   "the baseline's three parts are timed separately and summed; GB/s is a whole-call rate over "
                   "algorithmic bytes, not a kernel's share of peak")
    w.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
