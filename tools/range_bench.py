"""Time the range reads (gwaoi_range_batch, host and device forms) on the cfg3 world.

    python tools/range_bench.py [--n N] [--reps 30] [--warmup 3] [--out profiles/range_bench.json]

Builds the cfg3 world (1M entities in one space), flushes once, then for 1 / 64 / 4,096 / 65,536
queries, radii 3, 25, D and 3 D, slot-centred and about points (GWAOI_RANGE_POINT; the points are
positions of drawn entities shifted by a drawn offset below 1, so both kinds see the same density)
times the call.  Device form (queries already in HBM, rows left in HBM): HIP events on the world's
stream around the call plus a host clock around it (the call ends in a host wait).  Host form (numpy
in, numpy out through the binding): the host clock.  Per case: warm-up calls first, then the median
and p99 of `--reps` calls; the paths alternate call by call in one process.

Baseline: the path a game has without the call, from positions it holds on the host.
    slot-centred, r <= D   gwaoi_neighbors_batch (the InterestedIn rows) plus the numpy DistanceTo
                           filter over the host positions, at every query count
    points, or r > D       a numpy bounding-box mask over a host snapshot of all positions, then the
                           same distance, per query: at 1 and 64 queries only (it is a pass over
                           every entity per query)
Its answers are compared with the call's (sets and distances bit for bit).  There is no threshold:
`loses_to_baseline` says where the call's median is the larger one, and the baseline's own spread
(max - min) stands beside its median.

`items` is exact (the call's item count).  Rates are whole-call rates (items per second), not a
kernel's share of peak.  Needs a GPU: there is no CPU path.  Prints one JSON document (and writes --out).
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
BOX_BASELINE_SIZES = (1, 64)
F32 = np.float32


def dist(dx, dz):
    """Vector3.DistanceTo with every y equal to 0, float32 step by step."""
    d2 = (dx * dx + F32(0)) + dz * dz
    return np.sqrt(d2.astype(np.float64)).astype(np.float32)


def canon(off, items, dists):
    """Rows sorted by slot: comparable whatever the order within a row."""
    rid = np.repeat(np.arange(off.size - 1), np.diff(off.astype(np.int64)))
    o = np.lexsort((items, rid))
    return off.tolist(), items[o], dists[o].view(np.uint32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=0, help="entities (0: cfg3's 1M)")
    ap.add_argument("--reps", type=int, default=30, help="timed calls per case")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls per case first")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("range_bench needs a GPU (no CPU path)")
    from goworld_amd import World
    from goworld_amd.workload import make_workload

    wl = make_workload("cfg3", n=args.n or None)
    n, D = wl.n, float(wl.D)
    rng = np.random.default_rng(0x5A11)
    w = World(n, device=0)
    sp = w.space_create(D)
    slots, x0, z0, _ = wl.initial()
    px, pz = np.zeros(n, np.float32), np.zeros(n, np.float32)  # the host snapshot
    px[slots], pz[slots] = x0, z0
    w.entity_set_tag([0], [0])  # (the sync layer, before the flush)
    w.enter_batch(sp, slots, x0, z0)
    w.tick_device()
    w.sync()
    stream = torch.cuda.ExternalStream(w.stream())
    out = {"tool": "tools/range_bench.py", "workload": "cfg3", "n": n, "D": D, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "cases": []}

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

    def base_rows(src, r):
        """InterestedIn rows, then the distance filter (slot-centred, r <= D)."""
        off, items = w.neighbors_batch(src)
        rid = np.repeat(np.arange(src.size), np.diff(off.astype(np.int64)))
        d = dist(px[items] - px[src][rid], pz[items] - pz[src][rid])
        keep = d <= F32(r)
        cnt = np.bincount(rid[keep], minlength=src.size)
        o = np.zeros(src.size + 1, np.uint32)
        o[1:] = np.cumsum(cnt)
        return o, items[keep], d[keep]

    def base_box(cx, cz, r, me):
        """A bounding-box mask over the snapshot, then the distance, per query."""
        o = np.zeros(cx.size + 1, np.uint32)
        its, ds = [], []
        for m in range(cx.size):
            idx = np.flatnonzero((np.abs(px - cx[m]) <= r) & (np.abs(pz - cz[m]) <= r))
            if me is not None:
                idx = idx[idx != me[m]]
            d = dist(px[idx] - cx[m], pz[idx] - cz[m])
            keep = d <= F32(r)
            its.append(idx[keep].astype(np.uint32))
            ds.append(d[keep])
            o[m + 1] = o[m] + int(keep.sum())
        return o, np.concatenate(its), np.concatenate(ds)

    for k in SIZES:
        if k > n:
            continue
        src = rng.integers(0, n, k).astype(np.uint32)
        shift = rng.uniform(-1, 1, (k, 2)).astype(np.float32)
        pts = np.stack([px[src] + shift[:, 0], np.zeros(k, np.float32), pz[src] + shift[:, 1]], 1).astype(np.float32)
        for r in (3.0, 25.0, D, 3.0 * D):
            for kind in ("slot", "point"):
                q = World.range_queries(src, r) if kind == "slot" else World.range_queries(np.full(k, sp), r, points=pts)
                d_q = torch.from_numpy(q.view(np.uint8).copy()).to("cuda:0")
                torch.cuda.synchronize()
                if kind == "slot" and r <= D:
                    base, base_path = (lambda: base_rows(src, r)), "gwaoi_neighbors_batch + numpy DistanceTo filter"
                elif k in BOX_BASELINE_SIZES:
                    cx, cz = (px[src], pz[src]) if kind == "slot" else (pts[:, 0], pts[:, 2])
                    base = (lambda cx=cx, cz=cz: base_box(cx, cz, F32(r), src if kind == "slot" else None))
                    base_path = "numpy bounding-box mask over the host snapshot + DistanceTo, per query"
                else:
                    base, base_path = None, None
                dev = (lambda: w.range_batch_device(d_q.data_ptr(), k))
                host = (lambda: w.range_batch(q))
                for _ in range(args.warmup):
                    timed(dev)
                    host()
                    if base:
                        base()
                T = {"events": [], "wall": [], "host_form_wall": [], "baseline": []}
                got = gb = None
                for _ in range(args.reps):  # alternating: the paths see the same machine state
                    e, t, _ = timed(dev)
                    T["events"].append(e)
                    T["wall"].append(t)
                    t, got = walled(host)
                    T["host_form_wall"].append(t)
                    if base:
                        t, gb = walled(base)
                        T["baseline"].append(t)
                items = int(got[0][-1])
                se, sw, sh = stats(T["events"]), stats(T["wall"]), stats(T["host_form_wall"])
                row = {"queries": k, "radius": r, "centre": kind, "items": items, "events": se, "wall": sw,
                       "host_form_wall": sh, "items_per_s_device_form": items / (sw["median_ms"] * 1e-3),
                       "items_per_s_host_form": items / (sh["median_ms"] * 1e-3)}
                if base:
                    a, b = canon(*got), canon(*gb)
                    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (k, r, kind)
                    sb = stats(T["baseline"])
                    row["baseline"] = {"path": base_path, "wall": sb, "spread_ms": sb["max_ms"] - sb["min_ms"],
                                       "answers_equal": True,
                                       "speedup_median_device_form": sb["median_ms"] / sw["median_ms"],
                                       "speedup_median_host_form": sb["median_ms"] / sh["median_ms"],
                                       "loses_to_baseline": {"device_form": bool(sw["median_ms"] > sb["median_ms"]),
                                                             "host_form": bool(sh["median_ms"] > sb["median_ms"])}}
                out["cases"].append(row)
                print(f"{k} queries, r = {r}, {kind}: {items} items, device {sw['median_ms']:.3f} ms, host "
                      f"{sh['median_ms']:.3f} ms" + (f", baseline {row['baseline']['wall']['median_ms']:.3f} ms" if base else ""),
                      file=sys.stderr, flush=True)
    out["note"] = ("wall = host clock around the device-form call (it ends in a host wait); events = HIP events on the "
                   "world's stream around it; host_form_wall = host clock around the host-form call; rates are "
                   "whole-call rates, not a kernel's share of peak")
    w.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
