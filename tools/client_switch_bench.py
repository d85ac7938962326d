"""Time batched client switches (gwaoi_collect_client_switch) on the cfg3 world.

    python tools/client_switch_bench.py [--n N] [--reps 40] [--warmup 5] [--out profiles/client_switch_bench.json]

Builds the cfg3 world of tools/broadcast_bench.py (1M entities in one space, about
half with a client on one of 4 gates), flushes once, then for 1 / 64 / 4,096 /
65,536 switches times one `gwaoi_collect_client_switch` call through the C ABI
(arrays prepared beforehand; a host clock around the call, which ends in a stream
synchronise with both record lists in host memory).  A batch has distinct slots:
half attaches (entities without a client get one) and half client-to-client swaps
(a new ClientID on another gate).  Every timed call is followed by an untimed call
that puts the old clients back, so each timed call sees the same world.  Per
size: warm-up calls first, then the median and p99 of `--reps` calls.

Replaced path: before this call the library offered one `gwaoi_neighbors` per
switched entity (a launch and two copies each; the caller then builds the records
from its own tables) plus one `gwaoi_entity_set_client`.  It runs in the same
process, alternating with the new call, at 1 and 64 switches; its time does not
include building the records.

Needs a GPU: there is no CPU path.  Prints one JSON document (and writes --out,
keeping a "broadcast_walk" entry the file already has).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.broadcast_bench import GATES, entity_ids, stats  # noqa: E402

SIZES = (1, 64, 4096, 65536)
BASELINE_SIZES = (1, 64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=0, help="entities (0: cfg3's 1M)")
    ap.add_argument("--reps", type=int, default=40, help="timed calls per size (>= 30)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed calls per size first")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("client_switch_bench needs a GPU (no CPU path)")
    from goworld_amd import World
    from goworld_amd._lib import GateRecords
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
    L, W = w._L, w._w
    out = {"tool": "tools/client_switch_bench.py", "workload": "cfg3", "n": n, "clients": int(has.sum()),
           "gates": len(GATES), "D": float(wl.D), "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "sizes": [], "baseline": []}

    def p(a, t=C.c_void_p):
        return a.ctypes.data_as(t)

    def switch(sl, gt, ci):
        """One call through the C ABI -> (ms, create records, destroy records)."""
        c, d = GateRecords(), GateRecords()
        a = time.perf_counter()
        rc = L.gwaoi_collect_client_switch(W, p(sl), p(gt), p(ci) if ci is not None else None, sl.size, C.byref(c), C.byref(d))
        b = time.perf_counter()
        assert rc == 0, rc
        return (b - a) * 1e3, int(c.offsets[c.n_gates]), int(d.offsets[d.n_gates])

    free, taken = np.nonzero(~has)[0], np.nonzero(has)[0]
    for k in SIZES:
        if k > n:
            continue
        # half attaches, half swaps (1 switch: an attach), distinct slots
        att = rng.choice(free, (k + 1) // 2, replace=False).astype(np.uint32)
        swp = rng.choice(taken, k // 2, replace=False).astype(np.uint32)
        sl = np.ascontiguousarray(np.concatenate([att, swp]))
        gt = np.ascontiguousarray(np.concatenate([gate[att], np.asarray(GATES, np.uint16)[(swp + 1) % len(GATES)]]))
        ci = np.ascontiguousarray(entity_ids(b"N", sl))
        # the way back: the attached lose their client, the swapped get theirs again
        gt0 = np.ascontiguousarray(gate[sl])
        ci0 = np.ascontiguousarray(np.concatenate([np.zeros((att.size, 16), np.uint8), cids[swp]]))

        def replaced():
            """gwaoi_neighbors + gwaoi_entity_set_client per switch -> (ms, neighbours listed)."""
            hits = 0
            a = time.perf_counter()
            for m in range(k):
                hits += w.neighbors(int(sl[m])).size
                w.entity_set_client(int(sl[m]), int(gt[m]), ci[m])
            return (time.perf_counter() - a) * 1e3, hits

        for _ in range(args.warmup):
            switch(sl, gt, ci)
            switch(sl, gt0, ci0)
            if k in BASELINE_SIZES:
                replaced()
                switch(sl, gt0, ci0)
        wall, base, nc, nd, hits = [], [], 0, 0, None
        for _ in range(args.reps):  # alternating: the two paths see the same machine state
            t, nc, nd = switch(sl, gt, ci)
            wall.append(t)
            _, bc, bd = switch(sl, gt0, ci0)
            assert (bc, bd) == (nd, nc), "the way back lists the same neighbours"
            if k in BASELINE_SIZES:
                t, hits = replaced()
                base.append(t)
                assert hits == nc, (hits, nc)  # every switch lists its neighbours as creates (the swaps also as destroys)
                switch(sl, gt0, ci0)
        sw = stats(wall)
        out["sizes"].append({"switches": k, "attaches": int(att.size), "swaps": int(swp.size), "create_records": nc,
                             "destroy_records": nd, "wall": sw, "records_per_s_wall": (nc + nd) / (sw["median_ms"] * 1e-3),
                             "record_bytes": nc * 48 + nd * 32})
        if base:
            sb = stats(base)
            out["baseline"].append({"switches": k, "path": "gwaoi_neighbors + gwaoi_entity_set_client per switch (ctypes); "
                                    "building the records on the host is not included", "neighbours_listed": hits,
                                    "wall": sb, "per_switch_ms": sb["median_ms"] / k,
                                    "speedup_median": sb["median_ms"] / sw["median_ms"]})
    out["note"] = ("wall = host clock around one C-ABI call, which ends in a stream synchronise with both record lists "
                   "in host memory; every timed call is followed by an untimed one that restores the old clients")
    w.close()
    if args.out and os.path.exists(args.out):
        try:
            old = json.load(open(args.out))
            if "broadcast_walk" in old:
                out["broadcast_walk"] = old["broadcast_walk"]
        except ValueError:
            pass
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
