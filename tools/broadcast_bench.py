"""Time the broadcast fan-out (gwaoi_collect_broadcast_device) on the cfg3 world.

    python tools/broadcast_bench.py [--n N] [--reps 40] [--warmup 5] [--out profiles/broadcast_bench.json]

Builds the cfg3 world (1M entities in one space, about half with a client on one
of 4 gates), flushes once, then for 1 / 64 / 4,096 / 65,536 messages times
`collect_broadcast_device` (messages already in HBM, records left in HBM): HIP
events on the world's stream around the call plus a host clock around the call,
which ends in a stream synchronise.  Per size: warm-up calls first, then the
median and p99 of `--reps` calls.

Baseline: the only path the library offered before is one `gwaoi_neighbors` call
per source plus a host-side client lookup.  It runs in the same process,
alternating with the new path call by call, at 1 and 64 sources (more sources
only repeat the same launch + two host waits per source; the figure quoted for
larger batches is an extrapolation and is labelled so).

Floor: algorithmic bytes from the counts printed here,
    2 passes x candidates x 16 B + hits x (8 + 16) B + records x 32 B,
over the call time = a whole-call rate (not a kernel's share of peak: that
needs kernel times from a separate `rocprofv3 --kernel-trace --stats` run).
`candidates` is an estimate (the grid origin is internal): the entities in each
source's window widened to whole cells of size D / cells_per_dist anchored at
the frame's bounding box.  `hits` is exact where the baseline ran (it lists
every neighbour) and otherwise the neighbour records over the client share.

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

SIZES = (1, 64, 4096, 65536)
BASELINE_SIZES = (1, 64)
GATES = (1, 2, 3, 4)


def entity_ids(prefix: bytes, slots: np.ndarray) -> np.ndarray:
    ids = np.char.add(prefix, np.char.zfill(slots.astype(np.int64).astype("S15"), 15))
    return np.frombuffer(ids.astype("S16").tobytes(), np.uint8).reshape(-1, 16)


def window_candidates(x, z, src, D, cpd):
    """Entities in each source's window widened to whole cells (cell = D / cpd, anchored at the bbox)."""
    c = float(D) / max(1, int(cpd))
    x0, z0 = float(x.min()), float(z.min())
    cx = np.floor((x - x0) / c).astype(np.int64)
    cz = np.floor((z - z0) / c).astype(np.int64)
    gx, gz = int(cx.max()) + 1, int(cz.max()) + 1
    H = np.bincount(cz * gx + cx, minlength=gx * gz).reshape(gz, gx)
    S = np.zeros((gz + 1, gx + 1), np.int64)
    S[1:, 1:] = H.cumsum(0).cumsum(1)
    lo_x = np.clip(np.floor((x[src] - D - x0) / c).astype(np.int64), 0, gx - 1)
    hi_x = np.clip(np.floor((x[src] + D - x0) / c).astype(np.int64), 0, gx - 1) + 1
    lo_z = np.clip(np.floor((z[src] - D - z0) / c).astype(np.int64), 0, gz - 1)
    hi_z = np.clip(np.floor((z[src] + D - z0) / c).astype(np.int64), 0, gz - 1) + 1
    return int((S[hi_z, hi_x] - S[lo_z, hi_x] - S[hi_z, lo_x] + S[lo_z, lo_x]).sum())


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": float(np.median(a)), "p99_ms": float(a[min(a.size - 1, int(np.ceil(0.99 * a.size)) - 1)]),
            "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=0, help="entities (0: cfg3's 1M)")
    ap.add_argument("--reps", type=int, default=40, help="timed calls per size (>= 30)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed calls per size first")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("broadcast_bench needs a GPU (no CPU path)")
    from goworld_amd import World
    from goworld_amd.workload import make_workload

    wl = make_workload("cfg3", n=args.n or None)
    n = wl.n
    rng = np.random.default_rng(0xCA57)
    has = rng.random(n) < 0.5
    gate = np.asarray(GATES, np.uint16)[np.arange(n) % len(GATES)]
    w = World(n, device=0)
    sp = w.space_create(float(wl.D))
    slots, x0, z0, _ = wl.initial()
    w.entity_bind(slots, entity_ids(b"E", slots))
    cids = entity_ids(b"C", slots)
    for s in np.nonzero(has)[0]:
        w.entity_set_client(int(s), int(gate[s]), cids[s])
    w.enter_batch(sp, slots, x0, z0)
    w.tick_device()
    w.sync()
    cpd = w.debug_counters()["cells_per_dist"]
    stream = torch.cuda.ExternalStream(w.stream())
    out = {"tool": "tools/broadcast_bench.py", "workload": "cfg3", "n": n, "clients": int(has.sum()),
           "gates": len(GATES), "D": float(wl.D), "cells_per_dist": int(cpd), "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "sizes": [], "baseline": []}

    def timed_new(ds, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a = time.perf_counter()
        e0.record(stream)
        ids, off, _ = w.collect_broadcast_device(ds.data_ptr(), 0, k)
        e1.record(stream)
        e1.synchronize()
        b = time.perf_counter()
        return e0.elapsed_time(e1), (b - a) * 1e3, off[-1]

    def baseline(src):
        """gwaoi_neighbors per source + the host client lookup -> (receiver slot, gate) lists."""
        recs = hits = 0
        for s in src:
            nb = w.neighbors(int(s))
            hits += nb.size
            to = nb[has[nb]]
            _ = gate[to]
            recs += to.size + int(has[s])
        return recs, hits

    for k in SIZES:
        if k > n:
            continue
        src = rng.integers(0, n, k).astype(np.uint32)
        ds = torch.from_numpy(src.view(np.int32).copy()).to("cuda:0")
        torch.cuda.synchronize()
        for _ in range(args.warmup):
            timed_new(ds, k)
            if k in BASELINE_SIZES:
                baseline(src)
        ev, wall, base, records, hits = [], [], [], 0, None
        for _ in range(args.reps):  # alternating: the two paths see the same machine state
            e, t, records = timed_new(ds, k)
            ev.append(e)
            wall.append(t)
            if k in BASELINE_SIZES:
                a = time.perf_counter()
                brec, hits = baseline(src)
                base.append((time.perf_counter() - a) * 1e3)
                assert brec == records, (brec, records)
        own = int(has[src].sum())
        hits_kind = "exact (gwaoi_neighbors)"
        if hits is None:
            hits, hits_kind = int(round((records - own) / (has.sum() / n))), "estimate: neighbour records / client share"
        cand = window_candidates(x0, z0, src, float(wl.D), cpd)
        terms = {"candidates_2_passes_x_16B": 2 * cand * 16, "hits_x_24B": int(hits) * 24, "records_x_32B": int(records) * 32}
        tot_b = sum(terms.values())
        se, sw = stats(ev), stats(wall)
        row = {"messages": k, "records": int(records), "own_records": own, "hits": int(hits), "hits_kind": hits_kind,
               "candidates_estimate": cand, "events": se, "wall": sw,
               "records_per_s_wall": records / (sw["median_ms"] * 1e-3),
               "algorithmic_bytes": tot_b, "bytes_terms": terms, "dominant_term": max(terms, key=terms.get),
               "whole_call_GBps_wall": tot_b / (sw["median_ms"] * 1e-3) / 1e9,
               "whole_call_GBps_events": tot_b / (se["median_ms"] * 1e-3) / 1e9}
        out["sizes"].append(row)
        if base:
            sb = stats(base)
            out["baseline"].append({"sources": k, "path": "gwaoi_neighbors per source + host client lookup (ctypes)",
                                    "wall": sb, "per_source_ms": sb["median_ms"] / k,
                                    "speedup_median": sb["median_ms"] / sw["median_ms"]})
    if out["baseline"]:
        per = out["baseline"][-1]["per_source_ms"]
        out["baseline_extrapolated"] = [
            {"sources": r["messages"], "ms": per * r["messages"], "vs_new_median": per * r["messages"] / r["wall"]["median_ms"],
             "note": "EXTRAPOLATION: per-source cost at 64 sources x the source count, not measured"}
            for r in out["sizes"] if r["messages"] not in BASELINE_SIZES]
    out["note"] = ("wall = host clock around the call (it ends in a stream synchronise); events = HIP events on the "
                   "world's stream around the call; GB/s are whole-call rates over algorithmic bytes, not a kernel's "
                   "share of peak")
    w.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
