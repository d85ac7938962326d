"""Time the interest-set reads (gwaoi_neighbors_batch, gwaoi_related_batch, gwaoi_nearest_batch)
on the cfg3 world.

    python tools/interest_query_bench.py [--n N] [--reps 40] [--warmup 5] [--out profiles/interest_query_bench.json]

Builds the cfg3 world (1M entities in one space), tags a seeded half of the entities with bit 1,
flushes once, then for 1 / 64 / 4,096 / 65,536 queries times the three reads.  Device forms
(queries already in HBM, answers left in HBM): HIP events on the world's stream around the call
plus a host clock around the call, which ends in a stream synchronise.  Host forms (numpy in,
numpy out through the binding): the host clock.  Per size: warm-up calls first, then the median
and p99 of `--reps` calls.

Baseline: the only path the library offered before is one `gwaoi_neighbors` call per source plus
a host-side filter, through the same binding: the row itself; `b in row` for membership; the tag
filter and the float32 distance minimum in numpy for the nearest.  It runs in the same process,
alternating with the new path call by call, at 1 and 64 sources, and its answers are compared
with the new path's.  `beats_baseline_by_more_than_its_spread` is
(baseline median - new median) > (baseline max - baseline min) of that session.

Algorithmic bytes, from the counts printed here (`hits` is exact: the rows call's item count):
    rows        2 passes x candidates x 16 B + hits x (8 + 4) B + queries x 44 B
    membership  pairs x 65 B  (2 x 4 in, 2 x 4 rank, 2 x 8 slot/space, 2 x 16 record, 1 out)
    nearest     candidates x 16 B + hits x (8 + 4 + 4) B + queries x 48 B
over the call time = a whole-call rate (not a kernel's share of peak).  `candidates` is an
estimate (the grid origin is internal): the entities in each source's window widened to whole
cells of size D / cells_per_dist anchored at the frame's bounding box.

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

from tools.broadcast_bench import stats, window_candidates  # noqa: E402

SIZES = (1, 64, 4096, 65536)
BASELINE_SIZES = (1, 64)
NO_SLOT = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=0, help="entities (0: cfg3's 1M)")
    ap.add_argument("--reps", type=int, default=40, help="timed calls per size (>= 30)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed calls per size first")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("interest_query_bench needs a GPU (no CPU path)")
    from goworld_amd import World
    from goworld_amd.workload import make_workload

    wl = make_workload("cfg3", n=args.n or None)
    n = wl.n
    rng = np.random.default_rng(0x1A7E)
    tags = (rng.random(n) < 0.5).astype(np.uint32)
    w = World(n, device=0)
    sp = w.space_create(float(wl.D))
    slots, x0, z0, _ = wl.initial()
    px, pz = np.zeros(n, np.float32), np.zeros(n, np.float32)
    px[slots], pz[slots] = x0, z0
    w.entity_set_tag(np.arange(n), tags)
    w.enter_batch(sp, slots, x0, z0)
    w.tick_device()
    w.sync()
    cpd = w.debug_counters()["cells_per_dist"]
    stream = torch.cuda.ExternalStream(w.stream())
    out = {"tool": "tools/interest_query_bench.py", "workload": "cfg3", "n": n, "tagged": int(tags.sum()),
           "D": float(wl.D), "cells_per_dist": int(cpd), "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "sizes": []}

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

    # the parent's path: one gwaoi_neighbors per source, then the host filter
    def base_rows(src):
        return [w.neighbors(int(s)) for s in src]

    def base_related(a, b):
        return np.array([int(q) in w.neighbors(int(p)).tolist() for p, q in zip(a, b)], bool)

    def base_nearest(src):
        bs, bd = np.full(src.size, NO_SLOT, np.uint32), np.full(src.size, np.inf, np.float32)
        for m, s in enumerate(src):
            nb = w.neighbors(int(s))
            nb = nb[(tags[nb] & 1) == 1]
            if nb.size:
                dx, dz = px[nb] - px[s], pz[nb] - pz[s]
                d2 = (dx * dx + np.float32(0)) + dz * dz  # float32 step by step; every y is 0 here
                k = np.flatnonzero(d2 == d2.min())[0]     # (nb is sorted: the smallest slot of a tie)
                bs[m], bd[m] = nb[k], np.float32(np.sqrt(np.float64(d2[k])))
        return bs, bd

    for k in SIZES:
        if k > n:
            continue
        src = rng.integers(0, n, k).astype(np.uint32)
        # membership pairs: every second one a source and one of its neighbours (if it has any), the others random
        oth = rng.integers(0, n, k).astype(np.uint32)
        off, items = w.neighbors_batch(src)
        some = np.flatnonzero((off[1:] > off[:-1]) & (np.arange(k) % 2 == 0))
        oth[some] = items[off[:-1][some]]
        ones = np.ones(k, np.uint32)
        d_src = torch.from_numpy(src.view(np.int32).copy()).to("cuda:0")
        d_oth = torch.from_numpy(oth.view(np.int32).copy()).to("cuda:0")
        d_one = torch.from_numpy(ones.view(np.int32).copy()).to("cuda:0")
        d_rel = torch.zeros(k, dtype=torch.uint8, device="cuda:0")
        d_ns = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        d_nd = torch.zeros(k, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        calls = {
            "rows": (lambda: w.neighbors_batch_device(d_src.data_ptr(), k), lambda: w.neighbors_batch(src),
                     lambda: base_rows(src)),
            "membership": (lambda: w.related_batch_device(d_src.data_ptr(), d_oth.data_ptr(), k, d_rel.data_ptr()),
                           lambda: w.related_batch(src, oth), lambda: base_related(src, oth)),
            "nearest": (lambda: w.nearest_batch_device(d_src.data_ptr(), d_one.data_ptr(), d_one.data_ptr(), k,
                                                       d_ns.data_ptr(), d_nd.data_ptr()),
                        lambda: w.nearest_batch(src, ones, ones), lambda: base_nearest(src)),
        }
        with_base = k in BASELINE_SIZES
        for _ in range(args.warmup):
            for dev, host, base in calls.values():
                timed(dev)
                host()
                if with_base:
                    base()
        T = {name: {"events": [], "wall": [], "host_form_wall": [], "baseline": []} for name in calls}
        last = {}
        for _ in range(args.reps):  # alternating: the paths see the same machine state
            for name, (dev, host, base) in calls.items():
                e, t, _ = timed(dev)
                T[name]["events"].append(e)
                T[name]["wall"].append(t)
                t, r = walled(host)
                T[name]["host_form_wall"].append(t)
                last[name] = r
                if with_base:
                    t, rb = walled(base)
                    T[name]["baseline"].append(t)
                    last[name + "_base"] = rb
        off, items = last["rows"]
        hits = int(off[-1])
        if with_base:  # the two paths agree
            assert [np.sort(items[off[m]:off[m + 1]]).tolist() for m in range(k)] == [r.tolist() for r in last["rows_base"]]
            assert np.array_equal(last["membership"], last["membership_base"])
            assert np.array_equal(last["nearest"][0], last["nearest_base"][0])
            assert np.array_equal(last["nearest"][1].view(np.uint32), last["nearest_base"][1].view(np.uint32))
        cand = window_candidates(x0, z0, src, float(wl.D), cpd)
        nbytes = {"rows": 2 * cand * 16 + hits * 12 + k * 44, "membership": k * 65,
                  "nearest": cand * 16 + hits * 16 + k * 48}
        row = {"queries": k, "hits": hits, "candidates_estimate": cand, "related_true": int(last["membership"].sum()),
               "nearest_found": int((last["nearest"][0] != NO_SLOT).sum())}
        for name in calls:
            se, sw, sh = stats(T[name]["events"]), stats(T[name]["wall"]), stats(T[name]["host_form_wall"])
            r = {"events": se, "wall": sw, "host_form_wall": sh, "algorithmic_bytes": nbytes[name],
                 "whole_call_GBps_wall": nbytes[name] / (sw["median_ms"] * 1e-3) / 1e9,
                 "whole_call_GBps_events": nbytes[name] / (se["median_ms"] * 1e-3) / 1e9}
            if with_base:
                sb = stats(T[name]["baseline"])
                spread = sb["max_ms"] - sb["min_ms"]
                r["baseline"] = {"path": "gwaoi_neighbors per source + host filter (ctypes)", "wall": sb,
                                 "per_source_ms": sb["median_ms"] / k, "spread_ms": spread,
                                 "speedup_median_device_form": sb["median_ms"] / sw["median_ms"],
                                 "speedup_median_host_form": sb["median_ms"] / sh["median_ms"],
                                 "beats_baseline_by_more_than_its_spread": {
                                     "device_form": bool(sb["median_ms"] - sw["median_ms"] > spread),
                                     "host_form": bool(sb["median_ms"] - sh["median_ms"] > spread)}}
            row[name] = r
        out["sizes"].append(row)
        print(f"{k} queries done", file=sys.stderr, flush=True)
    out["note"] = ("wall = host clock around the device-form call (it ends in a stream synchronise); events = HIP events "
                   "on the world's stream around it; host_form_wall = host clock around the host-form call; GB/s are "
                   "whole-call rates over algorithmic bytes, not a kernel's share of peak")
    w.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
