"""ctypes binding of libgwaoi.so (include/gwaoi.h).

The shared library is built in-tree (goworld_amd/lib/libgwaoi.so) by
``goworld_amd.build``.  There is no fallback: if the library is missing,
``load()`` raises.  PyTorch, when installed, is imported first so that the
process holds exactly one HIP runtime (torch bundles its own libamdhip64, and
libgwaoi then binds to that copy by soname).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# GWAOI_LIB: an alternative in-tree build (tools/variants.sh, A/B tuning runs)
LIB_PATH = os.environ.get("GWAOI_LIB") or os.path.join(HERE, "lib", "libgwaoi.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "gwaoi.h")

GWAOI_F_TIMING = 1
GWAOI_F_NO_SPARSE = 2  # never the sparse flush (include/gwaoi.h)
GWAOI_F_BATCH_READY = 4  # accepted and ignored since ABI 5
GWAOI_F_UNIQUE_MOVES = 8  # a flush's Moved batches never repeat a slot: no last-op claims (checked on device)
# test and diagnostics flags (include/gwaoi.h): a slower or failing path, to compare with the default one
GWAOI_F_TEST_FORCE_RADIX = 0x100
GWAOI_F_TEST_FORCE_COPY = 0x200
GWAOI_F_TEST_BUCKETED = 0x400
GWAOI_F_TEST_REGROW_FAIL = 0x800
GWAOI_F_TEST_SPARSE_SEQUENCE = 0x1000
GWAOI_F_TEST_SPARSE_SCR2 = 0x2000
GWAOI_F_TEST_CHECK_STAGES = 0x4000

STATUS = {
    0: "GWAOI_OK", -1: "GWAOI_EINVAL", -2: "GWAOI_EBADSLOT", -3: "GWAOI_ESTATE", -4: "GWAOI_ENOMEM",
    -5: "GWAOI_EDEVICE", -6: "GWAOI_ENONFINITE", -7: "GWAOI_EBADSPACE", -8: "GWAOI_EBUSY",
    -9: "GWAOI_ECAPACITY",
}

# every function include/gwaoi.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "gwaoi_world_create", "gwaoi_world_destroy", "gwaoi_space_create", "gwaoi_space_destroy",
    "gwaoi_enter", "gwaoi_leave", "gwaoi_moved", "gwaoi_enter_batch", "gwaoi_leave_batch",
    "gwaoi_moved_batch", "gwaoi_moved_batch_device", "gwaoi_tick", "gwaoi_tick_device",
    "gwaoi_events_device", "gwaoi_neighbors", "gwaoi_world_info", "gwaoi_stage_times",
    "gwaoi_reset_stage_times", "gwaoi_set_stage_timing", "gwaoi_sync", "gwaoi_stream", "gwaoi_stream_after", "gwaoi_stream_before", "gwaoi_strerror", "gwaoi_last_error",
    "gwaoi_abi_version", "gwaoi_enter_seq", "gwaoi_moved_seq", "gwaoi_moved_batch_device_seq",
    "gwaoi_snapshot", "gwaoi_restore", "gwaoi_debug_counters", "gwaoi_tick_begin", "gwaoi_tick_finish",
    "gwaoi_events_csr", "gwaoi_events_csr_device",
    "gwaoi_enter_batch_device", "gwaoi_leave_batch_device", "gwaoi_moved_batch_stage",
    "gwaoi_moved_batch_commit", "gwaoi_moved_batch_pinned", "gwaoi_pinned_alloc", "gwaoi_pinned_free",
    "gwaoi_events_host", "gwaoi_pairs_host",
]

# gwaoi_tick_finish modes
GWAOI_END_NEXT, GWAOI_END_HOST, GWAOI_END_PAIRS = 1, 2, 4

# every function include/gwaoi_strips.h declares
STRIP_EXPORTS = [
    "gwaoi_strips_create", "gwaoi_strips_destroy", "gwaoi_strips_halo", "gwaoi_strips_route",
    "gwaoi_strips_route_scatter", "gwaoi_strips_tick", "gwaoi_strips_events_device", "gwaoi_strips_events",
    "gwaoi_strips_last_error", "gwaoi_strips_route_kinds", "gwaoi_strips_tick_async", "gwaoi_strips_wait",
    "gwaoi_strips_host_waits", "gwaoi_strips_route_row_words", "gwaoi_strips_route_begin", "gwaoi_strips_route_end",
]

# every function include/gwaoi_sync.h declares
SYNC_EXPORTS = [
    "gwaoi_entity_bind", "gwaoi_entity_bind_batch", "gwaoi_entity_unbind", "gwaoi_entity_set_client",
    "gwaoi_entity_set_syncing", "gwaoi_entity_set_position_yaw", "gwaoi_set_position_yaw",
    "gwaoi_sync_from_clients", "gwaoi_sync_from_clients_device", "gwaoi_collect_sync_infos",
    "gwaoi_collect_sync_infos_device", "gwaoi_collect_client_events", "gwaoi_entity_enter_plain",
    "gwaoi_entity_leave_plain", "gwaoi_collect_broadcast", "gwaoi_collect_broadcast_device",
    "gwaoi_collect_client_switch", "gwaoi_neighbors_batch", "gwaoi_neighbors_batch_device",
    "gwaoi_related_batch", "gwaoi_related_batch_device", "gwaoi_entity_set_tag", "gwaoi_entity_set_tag_batch",
    "gwaoi_nearest_batch", "gwaoi_nearest_batch_device", "gwaoi_steer_batch", "gwaoi_steer_batch_device",
    "gwaoi_range_batch", "gwaoi_range_batch_device", "gwaoi_range_count_batch", "gwaoi_range_count_batch_device",
]

# every function include/gwaoi_wire.h declares
WIRE_EXPORTS = [
    "gwaoi_wire_create", "gwaoi_wire_destroy", "gwaoi_wire_last_error", "gwaoi_wire_set_entity_games",
    "gwaoi_wire_remove_entities", "gwaoi_wire_set_clients", "gwaoi_wire_remove_clients",
    "gwaoi_wire_gate_from_clients", "gwaoi_wire_gate_from_clients_device", "gwaoi_wire_dispatcher_to_games",
    "gwaoi_wire_dispatcher_to_games_device", "gwaoi_wire_gate_to_clients", "gwaoi_wire_gate_to_clients_device",
]

SYNC_OUT_REC = 48  # ClientID[16] + EntityID[16] + x,y,z,yaw float32 (Entity.go:1233-1251)
DESTROY_REC = 32   # ClientID[16] + EntityID[16]
SIF_OWN_CLIENT, SIF_NEIGHBOR_CLIENTS = 1, 2
CAST_REC = 32      # ClientID[16] + msg, src slot, dst slot, 0 (uint32 little-endian): gwaoi_collect_broadcast
CAST_OWN, CAST_NEIGHBORS = 1, 2
NO_SLOT = 0xFFFFFFFF  # gwaoi_nearest_batch: no neighbour passes the filter (GWAOI_NO_SLOT)
STEER_MOVE, STEER_FACE = 1, 2  # gwaoi_steer_batch flags (GWAOI_STEER_MOVE / GWAOI_STEER_FACE)
RANGE_POINT, RANGE_PLANAR = 1, 2  # gwaoi_range_query flags (GWAOI_RANGE_POINT / GWAOI_RANGE_PLANAR)
# gwaoi_range_query, 32 B
RANGE_QUERY = np.dtype([("center", "<u4"), ("flags", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                        ("radius", "<f4"), ("mask", "<u4"), ("want", "<u4")])
CAST_DTYPE = np.dtype([("cid", np.uint8, (16,)), ("msg", "<u4"), ("src", "<u4"), ("dst", "<u4"), ("pad", "<u4")])


class Config(C.Structure):
    _fields_ = [("max_slots", C.c_uint32), ("max_spaces", C.c_uint32), ("device", C.c_int32),
                ("flags", C.c_uint32), ("event_capacity", C.c_uint64), ("cells_per_dist", C.c_float)]


class Events(C.Structure):
    _fields_ = [("n_enter", C.c_uint64), ("n_leave", C.c_uint64),
                ("enter", C.POINTER(C.c_uint32)), ("leave", C.POINTER(C.c_uint32))]


class Info(C.Structure):
    _fields_ = [("ticks", C.c_uint64), ("next_seq", C.c_uint64), ("live", C.c_uint32),
                ("spaces", C.c_uint32), ("total_cells", C.c_uint32), ("pending_ops", C.c_uint32),
                ("event_capacity", C.c_uint64), ("max_slots", C.c_uint32), ("max_spaces", C.c_uint32)]


class StripsConfig(C.Structure):
    _fields_ = [("n_strips", C.c_uint32), ("rank", C.c_uint32), ("edges", C.c_void_p),
                ("aoi_distance", C.c_float), ("teleport", C.c_float)]


class GateRecords(C.Structure):
    _fields_ = [("n_gates", C.c_uint32), ("gate_ids", C.POINTER(C.c_uint16)),
                ("offsets", C.POINTER(C.c_uint64)), ("records", C.c_void_p)]


class SlotRows(C.Structure):
    _fields_ = [("n", C.c_uint32), ("offsets", C.c_void_p), ("items", C.c_void_p)]


class RangeRows(C.Structure):
    _fields_ = [("n", C.c_uint32), ("offsets", C.c_void_p), ("items", C.c_void_p), ("dists", C.c_void_p)]


class WireGroups(C.Structure):
    _fields_ = [("n_groups", C.c_uint32), ("keys", C.POINTER(C.c_uint32)), ("offsets", C.POINTER(C.c_uint64)),
                ("records", C.c_void_p), ("rec_bytes", C.c_uint32), ("n_dropped", C.c_uint64)]


class Debug(C.Structure):
    _fields_ = [("flushes", C.c_uint64), ("combined_replays", C.c_uint64), ("combined_queue_drains", C.c_uint64),
                ("special_global", C.c_uint64), ("event_regrows", C.c_uint64), ("speculative_launches", C.c_uint64),
                ("cell_size_switches", C.c_uint64), ("cells_per_dist", C.c_uint32), ("pad", C.c_uint32),
                ("incremental_sorts", C.c_uint64), ("sparse_flushes", C.c_uint64), ("sparse_declined", C.c_uint64),
                ("premarked_runs", C.c_uint64), ("sparse_unfused", C.c_uint64),
                ("unique_flushes", C.c_uint64), ("overlapped_flushes", C.c_uint64)]


class StageTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("ms", C.c_double), ("calls", C.c_uint64)]


class GwaoiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code
        self.events = None  # tick(): the committed flush's (enter, leave) pairs, still to replay
        self.result = None  # steer_batch(): (applied, pos) when messages were dropped on the device (overflow)


_lib = None


def load():
    """Load libgwaoi.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:  # one HIP runtime per process: bind to torch's copy when torch is present
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, f, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t
    P = C.POINTER
    sigs = {
        "gwaoi_world_create": ([P(Config), P(vp)], C.c_int),
        "gwaoi_world_destroy": ([vp], C.c_int),
        "gwaoi_space_create": ([vp, f, P(u32)], C.c_int),
        "gwaoi_space_destroy": ([vp, u32], C.c_int),
        "gwaoi_enter": ([vp, u32, u32, f, f], C.c_int),
        "gwaoi_leave": ([vp, u32], C.c_int),
        "gwaoi_moved": ([vp, u32, f, f], C.c_int),
        "gwaoi_enter_batch": ([vp, u32, vp, vp, vp, sz], C.c_int),
        "gwaoi_leave_batch": ([vp, vp, sz], C.c_int),
        "gwaoi_moved_batch": ([vp, vp, vp, vp, sz], C.c_int),
        "gwaoi_moved_batch_device": ([vp, vp, vp, vp, sz], C.c_int),
        "gwaoi_tick": ([vp, P(Events)], C.c_int),
        "gwaoi_tick_device": ([vp, P(u64), P(u64)], C.c_int),
        "gwaoi_tick_begin": ([vp], C.c_int),
        "gwaoi_events_csr": ([vp, P(vp), P(vp), P(u64)], C.c_int),
        "gwaoi_events_csr_device": ([vp, P(vp), P(vp), P(u64)], C.c_int),
        "gwaoi_tick_finish": ([vp, C.c_uint32, P(u64), P(u64)], C.c_int),
        "gwaoi_events_host": ([vp, P(Events)], C.c_int),
        "gwaoi_pairs_host": ([vp, P(Events)], C.c_int),
        "gwaoi_moved_batch_stage": ([vp, sz, P(vp), P(vp), P(vp)], C.c_int),
        "gwaoi_moved_batch_commit": ([vp, sz], C.c_int),
        "gwaoi_moved_batch_pinned": ([vp, vp, vp, vp, sz], C.c_int),
        "gwaoi_pinned_alloc": ([vp, sz, P(vp)], C.c_int),
        "gwaoi_pinned_free": ([vp, vp], C.c_int),
        "gwaoi_events_device": ([vp, P(vp), P(vp)], C.c_int),
        "gwaoi_neighbors": ([vp, u32, vp, sz, P(sz)], C.c_int),
        "gwaoi_world_info": ([vp, P(Info)], C.c_int),
        "gwaoi_debug_counters": ([vp, P(Debug)], C.c_int),
        "gwaoi_stage_times": ([vp, P(StageTime), sz, P(sz)], C.c_int),
        "gwaoi_reset_stage_times": ([vp], C.c_int),
        "gwaoi_set_stage_timing": ([vp, C.c_uint32], C.c_int),
        "gwaoi_sync": ([vp], C.c_int),
        "gwaoi_stream": ([vp], vp),
        "gwaoi_stream_after": ([vp, vp], C.c_int),
        "gwaoi_stream_before": ([vp, vp], C.c_int),
        "gwaoi_strerror": ([C.c_int], C.c_char_p),
        "gwaoi_last_error": ([vp], C.c_char_p),
        "gwaoi_abi_version": ([], C.c_int),
        "gwaoi_enter_seq": ([vp, u32, u32, f, f, u64], C.c_int),
        "gwaoi_moved_seq": ([vp, u32, f, f, u64], C.c_int),
        "gwaoi_moved_batch_device_seq": ([vp, vp, vp, vp, vp, sz], C.c_int),
        "gwaoi_enter_batch_device": ([vp, u32, vp, vp, vp, vp, sz, vp], C.c_int),
        "gwaoi_leave_batch_device": ([vp, u32, vp, sz], C.c_int),
        "gwaoi_strips_create": ([vp, u32, P(StripsConfig), P(vp)], C.c_int),
        "gwaoi_strips_destroy": ([vp], C.c_int),
        "gwaoi_strips_halo": ([vp, P(f)], C.c_int),
        "gwaoi_strips_route": ([vp, vp, sz, P(u64)], C.c_int),
        "gwaoi_strips_route_row_words": ([vp, P(u32)], C.c_int),
        "gwaoi_strips_route_begin": ([vp, vp, sz, vp], C.c_int),
        "gwaoi_strips_route_end": ([vp, vp, P(vp), P(u64)], C.c_int),
        "gwaoi_strips_route_scatter": ([vp, vp, vp], C.c_int),
        "gwaoi_strips_tick": ([vp, vp, sz, vp, sz, vp, sz, P(u64), P(u64)], C.c_int),
        "gwaoi_strips_route_kinds": ([vp, vp, vp, vp], C.c_int),
        "gwaoi_strips_tick_async": ([vp, vp, sz, vp, sz, vp, sz, u64, u64, vp], C.c_int),
        "gwaoi_strips_wait": ([vp, P(u64), P(u64)], C.c_int),
        "gwaoi_strips_host_waits": ([vp, P(u64)], C.c_int),
        "gwaoi_strips_events_device": ([vp, P(vp), P(vp)], C.c_int),
        "gwaoi_strips_events": ([vp, P(Events)], C.c_int),
        "gwaoi_strips_last_error": ([vp], C.c_char_p),
        "gwaoi_snapshot": ([vp, vp, vp, vp, vp, vp, sz, P(sz)], C.c_int),
        "gwaoi_restore": ([vp, vp, vp, vp, vp, vp, sz], C.c_int),
        "gwaoi_entity_bind": ([vp, u32, vp], C.c_int),
        "gwaoi_entity_bind_batch": ([vp, vp, vp, sz], C.c_int),
        "gwaoi_entity_unbind": ([vp, u32], C.c_int),
        "gwaoi_entity_set_client": ([vp, u32, C.c_uint16, vp], C.c_int),
        "gwaoi_entity_set_syncing": ([vp, u32, C.c_int], C.c_int),
        "gwaoi_entity_set_position_yaw": ([vp, u32, f, f, f, f], C.c_int),
        "gwaoi_set_position_yaw": ([vp, u32, f, f, f, f], C.c_int),
        "gwaoi_entity_enter_plain": ([vp, u32, f, f, f], C.c_int),
        "gwaoi_entity_leave_plain": ([vp, u32], C.c_int),
        "gwaoi_sync_from_clients": ([vp, vp, sz], C.c_int),
        "gwaoi_sync_from_clients_device": ([vp, vp, sz], C.c_int),
        "gwaoi_collect_sync_infos": ([vp, P(GateRecords)], C.c_int),
        "gwaoi_collect_sync_infos_device": ([vp, P(GateRecords)], C.c_int),
        "gwaoi_collect_client_events": ([vp, P(GateRecords), P(GateRecords)], C.c_int),
        "gwaoi_collect_broadcast": ([vp, vp, vp, sz, P(GateRecords)], C.c_int),
        "gwaoi_collect_broadcast_device": ([vp, vp, vp, sz, P(GateRecords)], C.c_int),
        "gwaoi_collect_client_switch": ([vp, vp, vp, vp, sz, P(GateRecords), P(GateRecords)], C.c_int),
        "gwaoi_neighbors_batch": ([vp, vp, sz, P(SlotRows)], C.c_int),
        "gwaoi_neighbors_batch_device": ([vp, vp, sz, P(SlotRows)], C.c_int),
        "gwaoi_related_batch": ([vp, vp, vp, sz, vp], C.c_int),
        "gwaoi_related_batch_device": ([vp, vp, vp, sz, vp], C.c_int),
        "gwaoi_entity_set_tag": ([vp, u32, u32], C.c_int),
        "gwaoi_entity_set_tag_batch": ([vp, vp, vp, sz], C.c_int),
        "gwaoi_nearest_batch": ([vp, vp, vp, vp, sz, vp, vp], C.c_int),
        "gwaoi_nearest_batch_device": ([vp, vp, vp, vp, sz, vp, vp], C.c_int),
        "gwaoi_steer_batch": ([vp, vp, vp, vp, vp, sz, vp, vp], C.c_int),
        "gwaoi_steer_batch_device": ([vp, vp, vp, vp, vp, sz, vp, vp], C.c_int),
        "gwaoi_range_batch": ([vp, vp, sz, P(RangeRows)], C.c_int),
        "gwaoi_range_batch_device": ([vp, vp, sz, P(RangeRows)], C.c_int),
        "gwaoi_range_count_batch": ([vp, vp, sz, vp], C.c_int),
        "gwaoi_range_count_batch_device": ([vp, vp, sz, vp], C.c_int),
        "gwaoi_wire_create": ([C.c_int, P(vp)], C.c_int),
        "gwaoi_wire_destroy": ([vp], None),
        "gwaoi_wire_last_error": ([vp], C.c_char_p),
        "gwaoi_wire_set_entity_games": ([vp, vp, vp, sz], C.c_int),
        "gwaoi_wire_remove_entities": ([vp, vp, sz], C.c_int),
        "gwaoi_wire_set_clients": ([vp, vp, vp, sz], C.c_int),
        "gwaoi_wire_remove_clients": ([vp, vp, sz], C.c_int),
        "gwaoi_wire_gate_from_clients": ([vp, vp, sz, u32, P(WireGroups)], C.c_int),
        "gwaoi_wire_gate_from_clients_device": ([vp, vp, sz, u32, P(WireGroups)], C.c_int),
        "gwaoi_wire_dispatcher_to_games": ([vp, vp, sz, P(WireGroups)], C.c_int),
        "gwaoi_wire_dispatcher_to_games_device": ([vp, vp, sz, P(WireGroups)], C.c_int),
        "gwaoi_wire_gate_to_clients": ([vp, vp, sz, P(WireGroups)], C.c_int),
        "gwaoi_wire_gate_to_clients_device": ([vp, vp, sz, P(WireGroups)], C.c_int),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class World:
    """One GPU AOI world: many spaces, one HIP stream (include/gwaoi.h)."""

    def __init__(self, max_slots: int, max_spaces: int = 1, device: int = -1, timing: bool = False,
                 event_capacity: int = 0, cells_per_dist: float = 0.0, sparse: bool = True,
                 unique_moves: bool = False, test_flags: int = 0):
        """test_flags: an OR of GWAOI_F_TEST_* (tests comparing a slower path with the default one)."""
        self._L = load()
        flags = ((GWAOI_F_TIMING if timing else 0) | (0 if sparse else GWAOI_F_NO_SPARSE) |
                 (GWAOI_F_UNIQUE_MOVES if unique_moves else 0) | int(test_flags))
        cfg = Config(max_slots, max_spaces, device, flags, event_capacity, cells_per_dist)
        h = C.c_void_p()
        self._check(self._L.gwaoi_world_create(C.byref(cfg), C.byref(h)), world=False)
        self._w = h
        self.max_slots = max_slots

    def close(self):
        if getattr(self, "_w", None):
            self._L.gwaoi_world_destroy(self._w)
            self._w = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, world=True):
        if rc != 0:
            msg = self._L.gwaoi_strerror(rc).decode()
            if world and getattr(self, "_w", None):
                last = self._L.gwaoi_last_error(self._w).decode()
                if last:
                    msg += f" ({last})"
            raise GwaoiError(rc, msg)
        return rc

    # ---- spaces / AOIManager calls
    def space_create(self, aoi_distance) -> int:
        s = C.c_uint32()
        self._check(self._L.gwaoi_space_create(self._w, C.c_float(aoi_distance), C.byref(s)))
        return s.value

    def space_destroy(self, space):
        self._check(self._L.gwaoi_space_destroy(self._w, space))

    def enter(self, space, slot, x, z, seq=None):
        if seq is None:
            self._check(self._L.gwaoi_enter(self._w, space, slot, C.c_float(x), C.c_float(z)))
        else:
            self._check(self._L.gwaoi_enter_seq(self._w, space, slot, C.c_float(x), C.c_float(z), int(seq)))

    def leave(self, slot):
        self._check(self._L.gwaoi_leave(self._w, slot))

    def moved(self, slot, x, z, seq=None):
        if seq is None:
            self._check(self._L.gwaoi_moved(self._w, slot, C.c_float(x), C.c_float(z)))
        else:
            self._check(self._L.gwaoi_moved_seq(self._w, slot, C.c_float(x), C.c_float(z), int(seq)))

    def enter_batch(self, space, slots, x, z):
        s = np.ascontiguousarray(slots, np.uint32)
        x = np.ascontiguousarray(x, np.float32)
        z = np.ascontiguousarray(z, np.float32)
        self._check(self._L.gwaoi_enter_batch(self._w, space, _p(s), _p(x), _p(z), s.size))

    def leave_batch(self, slots):
        s = np.ascontiguousarray(slots, np.uint32)
        self._check(self._L.gwaoi_leave_batch(self._w, _p(s), s.size))

    def moved_batch(self, slots, x, z):
        s = np.ascontiguousarray(slots, np.uint32)
        x = np.ascontiguousarray(x, np.float32)
        z = np.ascontiguousarray(z, np.float32)
        self._check(self._L.gwaoi_moved_batch(self._w, _p(s), _p(x), _p(z), s.size))

    def stage_moves(self, n: int):
        """gwaoi_moved_batch_stage: (slots, x, z) numpy views of n moves in the world's pinned
        staging memory, to be filled by the caller and queued with commit_moves(k)."""
        ps, px, pz = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._L.gwaoi_moved_batch_stage(self._w, n, C.byref(ps), C.byref(px), C.byref(pz)))
        u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        return (np.ctypeslib.as_array(C.cast(ps, u32), shape=(n,)), np.ctypeslib.as_array(C.cast(px, f32), shape=(n,)),
                np.ctypeslib.as_array(C.cast(pz, f32), shape=(n,)))

    def commit_moves(self, k: int):
        """gwaoi_moved_batch_commit: queue the first k staged moves (one H2D, checked on the device)."""
        self._check(self._L.gwaoi_moved_batch_commit(self._w, k))

    def pinned_batch(self, n: int):
        """A move batch buffer in pinned host memory (gwaoi_pinned_alloc): (slots, x, z) numpy
        arrays of n moves; free with free_pinned_batch.  Queue a filled prefix with moved_batch_pinned."""
        p = C.c_void_p()
        self._check(self._L.gwaoi_pinned_alloc(self._w, 12 * n, C.byref(p)))
        buf = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(3 * n,))
        return p.value, (buf[:n], buf[n:2 * n].view(np.float32), buf[2 * n:].view(np.float32))

    def free_pinned_batch(self, ptr: int):
        self._check(self._L.gwaoi_pinned_free(self._w, C.c_void_p(ptr)))

    def moved_batch_pinned(self, views, k: int):
        """gwaoi_moved_batch_pinned: the first k moves of a pinned_batch (read in place by the H2D)."""
        s, x, z = views
        self._check(self._L.gwaoi_moved_batch_pinned(self._w, _p(s), _p(x), _p(z), k))

    def moved_batch_device(self, d_slots: int, d_x: int, d_z: int, n: int, d_seq: int | None = None):
        if d_seq is None:
            self._check(self._L.gwaoi_moved_batch_device(self._w, C.c_void_p(d_slots), C.c_void_p(d_x),
                                                         C.c_void_p(d_z), n))
        else:
            self._check(self._L.gwaoi_moved_batch_device_seq(self._w, C.c_void_p(d_slots), C.c_void_p(d_x),
                                                             C.c_void_p(d_z), C.c_void_p(d_seq), n))

    def enter_batch_device(self, space, d_slots: int, d_x: int, d_z: int, n: int, d_seq: int | None = None,
                           box=None):
        """gwaoi_enter_batch_device: Enter calls whose arrays live in device memory (slots
        not live; box = (x0, z0, x1, z1) around the positions, or None)."""
        b = np.ascontiguousarray(box, np.float32) if box is not None else None
        self._check(self._L.gwaoi_enter_batch_device(self._w, space, C.c_void_p(d_slots), C.c_void_p(d_x),
                                                     C.c_void_p(d_z), C.c_void_p(d_seq) if d_seq else None, n,
                                                     _p(b) if b is not None else None))

    def leave_batch_device(self, space, d_slots: int, n: int):
        self._check(self._L.gwaoi_leave_batch_device(self._w, space, C.c_void_p(d_slots), n))

    # ---- flush
    def tick(self, copy: bool = True):
        """Flush; returns (enter_pairs, leave_pairs) as (n,2) uint32 arrays [a, b].

        When the flush committed but the device reported a problem in the queued
        ops (a dropped move: ESTATE / ENONFINITE / EINVAL), the GwaoiError carries
        the flush's events as ``.events``: they must still be replayed.
        copy=False: views of the world's pinned buffer, valid until the next flush."""
        ev = Events()
        return self._events(self._L.gwaoi_tick(self._w, C.byref(ev)), ev, copy)

    def tick_begin(self):
        """Start the flush (gwaoi_tick_begin); AOIManager calls made before tick_end
        are queued for the next flush."""
        self._check(self._L.gwaoi_tick_begin(self._w))

    def finish(self, mode: int = 0):
        """gwaoi_tick_finish(mode): commit the flush in flight; mode is an OR of GWAOI_END_NEXT
        (begin the next flush), GWAOI_END_HOST (events to host memory: events_host) and
        GWAOI_END_PAIRS (one event per mirrored pair: pairs_host).  Returns the finished flush's
        (n_enter, n_leave); on a committed flush with a device-reported problem the GwaoiError
        carries them as ``.counts``."""
        ne, nl = C.c_uint64(), C.c_uint64()
        rc = self._L.gwaoi_tick_finish(self._w, mode, C.byref(ne), C.byref(nl))
        if rc != 0:
            try:
                self._check(rc)
            except GwaoiError as e:
                e.counts = (ne.value, nl.value)
                raise
        return ne.value, nl.value

    def _finish_events(self, mode, copy):
        # the flush's host events with its status: a committed flush with a device-reported
        # problem raises with them as ``.events`` (events_host describes the copy this call made,
        # empty when the flush did not commit)
        err = None
        try:
            self.finish(mode)
        except GwaoiError as e:
            err = e
        ev = Events()
        ok = self._L.gwaoi_events_host(self._w, C.byref(ev)) == 0
        ent, lev = self._events(0, ev, copy) if ok else (None, None)
        if err is not None:
            err.events = (ent, lev) if ok else None
            raise err
        return ent, lev

    def tick_end(self, copy: bool = True):
        """Finish the flush started by tick_begin: (enter_pairs, leave_pairs) as tick()
        (gwaoi_tick_finish(GWAOI_END_HOST))."""
        return self._finish_events(GWAOI_END_HOST, copy)

    def tick_end_device(self):
        """gwaoi_tick_finish(0): events stay in HBM."""
        return self.finish(0)

    def tick_end_begin_device(self):
        """gwaoi_tick_finish(GWAOI_END_NEXT): finish the flush in flight and begin the next one
        (queued on the GPU before this one's commit when only device Moved batches were
        queued).  Returns the finished flush's (n_enter, n_leave); its events stay
        readable through events_device() while the next flush runs."""
        return self.finish(GWAOI_END_NEXT)

    def tick_end_begin(self, copy: bool = True):
        """gwaoi_tick_finish(GWAOI_END_NEXT | GWAOI_END_HOST) + events_host: finish the flush in
        flight (its events copied to host memory beside the next flush) and begin the next one."""
        return self._finish_events(GWAOI_END_NEXT | GWAOI_END_HOST, copy)

    def tick_end_begin_async(self):
        """gwaoi_tick_finish(GWAOI_END_NEXT | GWAOI_END_HOST): the events' copy to host memory is
        left running; returns (n_enter, n_leave).  events_host() waits for it."""
        return self.finish(GWAOI_END_NEXT | GWAOI_END_HOST)

    def tick_end_begin_pairs_async(self):
        """gwaoi_tick_finish(GWAOI_END_NEXT | GWAOI_END_PAIRS): one event per mirrored pair copied
        out; returns the directed (n_enter, n_leave).  pairs_host() waits for them."""
        return self.finish(GWAOI_END_NEXT | GWAOI_END_PAIRS)

    def pairs_host(self, copy: bool = True):
        """gwaoi_pairs_host: (enter pairs, leave pairs) as (n,2) arrays; (a,b) stands for (a,b) and (b,a)."""
        ev = Events()
        return self._events(self._L.gwaoi_pairs_host(self._w, C.byref(ev)), ev, copy)

    def events_host(self, copy: bool = True):
        """gwaoi_events_host: the events of the last tick_end_begin_async in host memory."""
        ev = Events()
        return self._events(self._L.gwaoi_events_host(self._w, C.byref(ev)), ev, copy)

    def _events(self, rc, ev, copy):
        ne, nl = ev.n_enter, ev.n_leave
        cp = (lambda a: a.copy()) if copy else (lambda a: a)
        ent = cp(np.ctypeslib.as_array(ev.enter, shape=(2 * ne,)).reshape(ne, 2)) if ne else np.empty((0, 2), np.uint32)
        lev = cp(np.ctypeslib.as_array(ev.leave, shape=(2 * nl,)).reshape(nl, 2)) if nl else np.empty((0, 2), np.uint32)
        if rc != 0:
            try:
                self._check(rc)
            except GwaoiError as e:
                e.events = (ent, lev) if (ev.enter or ev.leave) else None
                raise
        return ent, lev

    def tick_device(self):
        """Flush; events stay in HBM.  Returns (n_enter, n_leave); on a committed flush
        with a device-reported problem the GwaoiError carries them as ``.counts``."""
        ne, nl = C.c_uint64(), C.c_uint64()
        rc = self._L.gwaoi_tick_device(self._w, C.byref(ne), C.byref(nl))
        if rc != 0:
            try:
                self._check(rc)
            except GwaoiError as e:
                e.counts = (ne.value, nl.value)
                raise
        return ne.value, nl.value

    def events_csr(self):
        """The last flush's events by entity (gwaoi_events_csr): (offsets[max_slots+1], items)
        uint32 copies; item = b | 0x80000000 for an enter (s, b), b for a leave."""
        o, it, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self._L.gwaoi_events_csr(self._w, C.byref(o), C.byref(it), C.byref(n)))
        off = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint32)), shape=(self.max_slots + 1,)).copy()
        items = (np.ctypeslib.as_array(C.cast(it, C.POINTER(C.c_uint32)), shape=(n.value,)).copy() if n.value
                 else np.empty(0, np.uint32))
        return off, items

    def events_device(self):
        e, l = C.c_void_p(), C.c_void_p()
        self._check(self._L.gwaoi_events_device(self._w, C.byref(e), C.byref(l)))
        return e.value, l.value

    # ---- queries
    def neighbors(self, slot, cap=4096):
        while True:
            out = np.empty(cap, np.uint32)
            n = C.c_size_t()
            self._check(self._L.gwaoi_neighbors(self._w, slot, _p(out), cap, C.byref(n)))
            if n.value <= cap:
                return np.sort(out[:n.value])
            cap = n.value

    def info(self) -> dict:
        i = Info()
        self._check(self._L.gwaoi_world_info(self._w, C.byref(i)))
        return {k: getattr(i, k) for k, _ in Info._fields_}

    def debug_counters(self) -> dict:
        """Rare-path counters summed over flushes (gwaoi_debug_counters)."""
        d = Debug()
        self._check(self._L.gwaoi_debug_counters(self._w, C.byref(d)))
        return {k: getattr(d, k) for k, _ in Debug._fields_}

    def stage_times(self) -> dict:
        arr = (StageTime * 32)()
        n = C.c_size_t()
        self._check(self._L.gwaoi_stage_times(self._w, arr, 32, C.byref(n)))
        return {arr[i].name.decode(): (arr[i].ms, arr[i].calls) for i in range(min(n.value, 32))}

    def stage_names(self) -> list:
        arr = (StageTime * 32)()
        n = C.c_size_t()
        self._check(self._L.gwaoi_stage_times(self._w, arr, 32, C.byref(n)))
        return [arr[i].name.decode() for i in range(min(n.value, 32))]

    def set_stage_timing(self, stages=None):
        """Time the named stages with HIP events (None = all, [] = none)."""
        names = getattr(self, "_stage_names", None) or self.stage_names()
        self._stage_names = names
        mask = (1 << len(names)) - 1 if stages is None else sum(1 << names.index(s) for s in stages)
        self._check(self._L.gwaoi_set_stage_timing(self._w, mask))

    def reset_stage_times(self):
        self._check(self._L.gwaoi_reset_stage_times(self._w))

    def sync(self):
        self._check(self._L.gwaoi_sync(self._w))

    def stream(self) -> int:
        return self._L.gwaoi_stream(self._w) or 0

    def stream_after(self, other: int):
        """The world's stream runs what it is given next after everything queued on `other` (a hipStream_t)."""
        self._check(self._L.gwaoi_stream_after(self._w, C.c_void_p(other)))

    def stream_before(self, other: int):
        """`other` runs what it is given next after everything queued on the world's stream."""
        self._check(self._L.gwaoi_stream_before(self._w, C.c_void_p(other)))

    # ---- freeze / restore
    def snapshot(self) -> dict:
        """AOI state of the last flush in frame order: slot, space, x, z, seq arrays."""
        n = C.c_size_t()
        self._check(self._L.gwaoi_snapshot(self._w, None, None, None, None, None, 0, C.byref(n)))
        k = n.value
        out = {"slot": np.empty(k, np.uint32), "space": np.empty(k, np.uint32), "x": np.empty(k, np.float32),
               "z": np.empty(k, np.float32), "seq": np.empty(k, np.uint64)}
        if k:
            self._check(self._L.gwaoi_snapshot(self._w, _p(out["slot"]), _p(out["space"]), _p(out["x"]),
                                               _p(out["z"]), _p(out["seq"]), k, C.byref(n)))
        return out

    def restore(self, snap: dict):
        a = {k: np.ascontiguousarray(snap[k], t) for k, t in
             (("slot", np.uint32), ("space", np.uint32), ("x", np.float32), ("z", np.float32), ("seq", np.uint64))}
        self._check(self._L.gwaoi_restore(self._w, _p(a["slot"]), _p(a["space"]), _p(a["x"]), _p(a["z"]),
                                          _p(a["seq"]), a["slot"].size))

    # ---- entity position sync (include/gwaoi_sync.h)
    def entity_bind(self, slots, eids):
        """Bind slots to 16-byte entity ids: eids is (n,16) uint8 or a list of 16-byte bytes."""
        s = np.ascontiguousarray(np.atleast_1d(slots), np.uint32)
        e = _ids(eids, s.size)
        self._check(self._L.gwaoi_entity_bind_batch(self._w, _p(s), _p(e), s.size))

    def entity_unbind(self, slot):
        self._check(self._L.gwaoi_entity_unbind(self._w, slot))

    def entity_set_client(self, slot, gate_id=0, clientid=None):
        if clientid is None:
            self._check(self._L.gwaoi_entity_set_client(self._w, slot, 0, None))
        else:
            c = _ids([clientid], 1)
            self._check(self._L.gwaoi_entity_set_client(self._w, slot, gate_id, _p(c)))

    def entity_set_syncing(self, slot, syncing=True):
        self._check(self._L.gwaoi_entity_set_syncing(self._w, slot, 1 if syncing else 0))

    def entity_set_position_yaw(self, slot, x, y, z, yaw):
        self._check(self._L.gwaoi_entity_set_position_yaw(self._w, slot, C.c_float(x), C.c_float(y),
                                                          C.c_float(z), C.c_float(yaw)))

    def entity_enter_plain(self, slot, x, y, z):
        """Space.enter of a space without AOI (or an entity type without AOI)."""
        self._check(self._L.gwaoi_entity_enter_plain(self._w, slot, C.c_float(x), C.c_float(y), C.c_float(z)))

    def entity_leave_plain(self, slot):
        self._check(self._L.gwaoi_entity_leave_plain(self._w, slot))

    def set_position_yaw(self, slot, x, y, z, yaw):
        self._check(self._L.gwaoi_set_position_yaw(self._w, slot, C.c_float(x), C.c_float(y), C.c_float(z),
                                                   C.c_float(yaw)))

    def sync_from_clients(self, payload):
        """Decode a HandleSyncPositionYawFromClient payload (bytes / uint8 array, 32 B per record)."""
        b = np.frombuffer(bytes(payload), np.uint8) if not isinstance(payload, np.ndarray) else \
            np.ascontiguousarray(payload, np.uint8).reshape(-1)
        if b.size % 32:
            raise ValueError("payload is not a whole number of 32-byte records")
        self._check(self._L.gwaoi_sync_from_clients(self._w, _p(b), b.size // 32))

    def sync_from_clients_device(self, d_payload: int, n_rec: int):
        self._check(self._L.gwaoi_sync_from_clients_device(self._w, C.c_void_p(d_payload), n_rec))

    def collect_sync_infos(self) -> dict:
        """CollectEntitySyncInfos: {gate_id: (n,48) uint8 records}."""
        g = GateRecords()
        self._check(self._L.gwaoi_collect_sync_infos(self._w, C.byref(g)))
        return _gate_dict(g, SYNC_OUT_REC)

    def collect_sync_infos_device(self):
        """Records stay in HBM: (gate_ids, offsets (records), device pointer)."""
        g = GateRecords()
        self._check(self._L.gwaoi_collect_sync_infos_device(self._w, C.byref(g)))
        ids = [g.gate_ids[i] for i in range(g.n_gates)]
        off = [g.offsets[i] for i in range(g.n_gates + 1)] if g.n_gates else [0]
        return ids, off, g.records or 0

    def collect_client_events(self):
        """Events routed to clients: ({gate: (n,48) create records}, {gate: (n,32) destroy records})."""
        c, d = GateRecords(), GateRecords()
        self._check(self._L.gwaoi_collect_client_events(self._w, C.byref(c), C.byref(d)))
        return _gate_dict(c, SYNC_OUT_REC), _gate_dict(d, DESTROY_REC)

    def collect_broadcast(self, slots, flags=None) -> dict:
        """AllClients delivery of a batch of messages (gwaoi_collect_broadcast): message m comes
        from entity slots[m] with flags[m] (CAST_OWN | CAST_NEIGHBORS; None: both for every
        message).  Returns {gate_id: (n,32) uint8 records} of the gates that receive any (an empty
        batch gives {}); view a gate's array as CAST_DTYPE."""
        s = np.ascontiguousarray(np.atleast_1d(slots), np.uint32).reshape(-1)
        f = None
        if flags is not None:
            f = np.ascontiguousarray(np.atleast_1d(flags), np.uint32).reshape(-1)
            if f.size != s.size:
                raise ValueError(f"{s.size} slots but {f.size} flags")
        g = GateRecords()
        self._check(self._L.gwaoi_collect_broadcast(self._w, _p(s) if s.size else None,
                                                    _p(f) if f is not None and f.size else None, s.size, C.byref(g)))
        return {k: a for k, a in _gate_dict(g, CAST_REC).items() if len(a)}

    def collect_broadcast_device(self, d_slots: int, d_flags: int, n: int):
        """Messages in device memory (d_flags 0: both flags for every message), records stay in
        HBM: (gate_ids, offsets (records), device pointer), valid until the next broadcast."""
        g = GateRecords()
        self._check(self._L.gwaoi_collect_broadcast_device(self._w, C.c_void_p(d_slots) if d_slots else None,
                                                           C.c_void_p(d_flags) if d_flags else None, n, C.byref(g)))
        ids = [g.gate_ids[i] for i in range(g.n_gates)]
        off = [g.offsets[i] for i in range(g.n_gates + 1)] if g.n_gates else [0]
        return ids, off, g.records or 0

    def collect_client_switch(self, slots, gates, clientids):
        """Entity.SetClient for a batch (gwaoi_collect_client_switch): message m sets the client of
        slots[m] to (gates[m], clientids[m]); clientids[m] is 16 bytes, or None for no client.
        Returns ({gate_id: (n,48) create records}, {gate_id: (n,32) destroy records}) of the gates
        that receive any, for the entities in each source's InterestedBy, and switches the clients."""
        s = np.ascontiguousarray(np.atleast_1d(slots), np.uint32).reshape(-1)
        gt = np.ascontiguousarray(np.atleast_1d(gates), np.uint16).reshape(-1)
        cl = list(clientids)
        if gt.size != s.size or len(cl) != s.size:
            raise ValueError(f"{s.size} slots but {gt.size} gates and {len(cl)} client ids")
        ids = None
        if any(c is not None for c in cl):
            ids = _ids([bytes(16) if c is None else c for c in cl], s.size)
        c, d = GateRecords(), GateRecords()
        self._check(self._L.gwaoi_collect_client_switch(self._w, _p(s) if s.size else None, _p(gt) if s.size else None,
                                                        _p(ids) if ids is not None else None, s.size,
                                                        C.byref(c), C.byref(d)))
        return ({k: a for k, a in _gate_dict(c, SYNC_OUT_REC).items() if len(a)},
                {k: a for k, a in _gate_dict(d, DESTROY_REC).items() if len(a)})

    # ---- interest-set reads (include/gwaoi_sync.h)
    NO_SLOT = NO_SLOT

    def neighbors_batch(self, slots):
        """InterestedIn of every slots[m] on the relation of the last flush (gwaoi_neighbors_batch):
        (offsets[n + 1], items) uint32 copies, row m = items[offsets[m]:offsets[m + 1]] in an
        unspecified order.  A slot outside every AOI space gives an empty row."""
        s = np.ascontiguousarray(np.atleast_1d(slots), np.uint32).reshape(-1)
        r = SlotRows()
        self._check(self._L.gwaoi_neighbors_batch(self._w, _p(s) if s.size else None, s.size, C.byref(r)))
        off = np.ctypeslib.as_array(C.cast(r.offsets, C.POINTER(C.c_uint32)), shape=(r.n + 1,)).copy()
        items = (np.ctypeslib.as_array(C.cast(r.items, C.POINTER(C.c_uint32)), shape=(int(off[-1]),)).copy()
                 if off[-1] else np.empty(0, np.uint32))
        return off, items

    def neighbors_batch_device(self, d_slots: int, n: int):
        """Slots in device memory, rows stay in HBM: (offsets pointer, items pointer, n_items), valid
        until the next rows call.  n_items is offsets[n], read back from the device."""
        r = SlotRows()
        self._check(self._L.gwaoi_neighbors_batch_device(self._w, C.c_void_p(d_slots) if d_slots else None, n,
                                                         C.byref(r)))
        return r.offsets or 0, r.items or 0, _device_u32((r.offsets or 0) + 4 * r.n)

    def related_batch(self, a, b) -> np.ndarray:
        """a[m].IsInterestedIn(b[m]) on the relation of the last flush (gwaoi_related_batch): a bool array."""
        qa = np.ascontiguousarray(np.atleast_1d(a), np.uint32).reshape(-1)
        qb = np.ascontiguousarray(np.atleast_1d(b), np.uint32).reshape(-1)
        if qa.size != qb.size:
            raise ValueError(f"{qa.size} slots a but {qb.size} slots b")
        out = np.zeros(qa.size, np.uint8)
        self._check(self._L.gwaoi_related_batch(self._w, _p(qa) if qa.size else None, _p(qb) if qa.size else None,
                                                qa.size, _p(out) if qa.size else None))
        return out.astype(bool)

    def related_batch_device(self, d_a: int, d_b: int, n: int, d_out: int):
        """Pairs and the n answer bytes in device memory."""
        self._check(self._L.gwaoi_related_batch_device(self._w, C.c_void_p(d_a) if d_a else None,
                                                       C.c_void_p(d_b) if d_b else None, n,
                                                       C.c_void_p(d_out) if d_out else None))

    def entity_set_tag(self, slots, tags):
        """32 caller-defined bits per slot, read by nearest_batch's filter (gwaoi_entity_set_tag_batch)."""
        s = np.ascontiguousarray(np.atleast_1d(slots), np.uint32).reshape(-1)
        t = np.ascontiguousarray(np.atleast_1d(tags), np.uint32).reshape(-1)
        if s.size != t.size:
            raise ValueError(f"{s.size} slots but {t.size} tags")
        self._check(self._L.gwaoi_entity_set_tag_batch(self._w, _p(s) if s.size else None, _p(t) if s.size else None,
                                                       s.size))

    def nearest_batch(self, slots, masks=None, wants=None):
        """For every slots[m], the neighbour b with (tag[b] & masks[m]) == wants[m] of the smallest
        DistanceTo, ties to the smallest slot (gwaoi_nearest_batch): (slots uint32, distances
        float32); NO_SLOT and +inf where there is none.  masks=None: every neighbour."""
        s = np.ascontiguousarray(np.atleast_1d(slots), np.uint32).reshape(-1)
        mk = wt = None
        if masks is not None:
            mk = np.ascontiguousarray(np.atleast_1d(masks), np.uint32).reshape(-1)
            wt = np.ascontiguousarray(np.atleast_1d(wants), np.uint32).reshape(-1)
            if mk.size != s.size or wt.size != s.size:
                raise ValueError(f"{s.size} slots but {mk.size} masks and {wt.size} wants")
        out_s, out_d = np.empty(s.size, np.uint32), np.empty(s.size, np.float32)
        some = s.size > 0
        self._check(self._L.gwaoi_nearest_batch(self._w, _p(s) if some else None, _p(mk) if some and mk is not None else None,
                                                _p(wt) if some and wt is not None else None, s.size,
                                                _p(out_s) if some else None, _p(out_d) if some else None))
        return out_s, out_d

    def nearest_batch_device(self, d_slots: int, d_masks: int, d_wants: int, n: int, d_out_slot: int, d_out_dist: int):
        """Every array in device memory (d_masks 0: every neighbour)."""
        q = [C.c_void_p(p) if p else None for p in (d_slots, d_masks, d_wants)]
        self._check(self._L.gwaoi_nearest_batch_device(self._w, q[0], q[1], q[2], n,
                                                       C.c_void_p(d_out_slot) if d_out_slot else None,
                                                       C.c_void_p(d_out_dist) if d_out_dist else None))

    # ---- range reads (include/gwaoi_sync.h)
    RANGE_POINT, RANGE_PLANAR = RANGE_POINT, RANGE_PLANAR

    @staticmethod
    def range_queries(centers, radii, masks=None, wants=None, points=None, planar=False) -> np.ndarray:
        """A RANGE_QUERY array: query m asks for the entities within radii[m] of slot centers[m], or,
        with points (n x 3: x, y, z) given, of points[m] in space centers[m].  radii, masks, wants and
        planar broadcast over the queries; masks=None: everyone ((tag & mask) == want otherwise)."""
        c = np.ascontiguousarray(np.atleast_1d(centers), np.uint32).reshape(-1)
        q = np.zeros(c.size, RANGE_QUERY)
        q["center"] = c
        q["radius"] = np.broadcast_to(np.asarray(radii, np.float32), c.shape)
        q["flags"] = np.where(np.broadcast_to(np.asarray(planar, bool), c.shape), RANGE_PLANAR, 0)
        if points is not None:
            pt = np.asarray(points, np.float32).reshape(-1, 3)
            if pt.shape[0] != c.size:
                raise ValueError(f"{c.size} spaces but {pt.shape[0]} points")
            q["flags"] |= RANGE_POINT
            q["x"], q["y"], q["z"] = pt[:, 0], pt[:, 1], pt[:, 2]
        if masks is not None:
            q["mask"] = np.broadcast_to(np.asarray(masks, np.uint32), c.shape)
            q["want"] = np.broadcast_to(np.asarray(masks if wants is None else wants, np.uint32), c.shape)
        return q

    def range_batch(self, q):
        """The entities within each query's radius on the frame of the last flush (gwaoi_range_batch):
        (offsets[n + 1] uint32, items uint32, dists float32) copies; row m =
        items[offsets[m]:offsets[m + 1]] in an unspecified order, dists parallel to items."""
        a = np.ascontiguousarray(q, RANGE_QUERY).reshape(-1)
        r = RangeRows()
        self._check(self._L.gwaoi_range_batch(self._w, _p(a) if a.size else None, a.size, C.byref(r)))
        off = np.ctypeslib.as_array(C.cast(r.offsets, C.POINTER(C.c_uint32)), shape=(r.n + 1,)).copy()
        k = int(off[-1])
        if not k:
            return off, np.empty(0, np.uint32), np.empty(0, np.float32)
        return (off, np.ctypeslib.as_array(C.cast(r.items, C.POINTER(C.c_uint32)), shape=(k,)).copy(),
                np.ctypeslib.as_array(C.cast(r.dists, C.POINTER(C.c_float)), shape=(k,)).copy())

    def range_count_batch(self, q) -> np.ndarray:
        """The length of each query's row (gwaoi_range_count_batch): the count pass alone."""
        a = np.ascontiguousarray(q, RANGE_QUERY).reshape(-1)
        out = np.zeros(a.size, np.uint32)
        self._check(self._L.gwaoi_range_count_batch(self._w, _p(a) if a.size else None, a.size,
                                                    _p(out) if a.size else None))
        return out

    def range_batch_device(self, d_q: int, n: int):
        """Queries in device memory (16-B aligned), rows stay in HBM: (offsets pointer, items pointer,
        dists pointer, n_items), valid until the next range call.  n_items is offsets[n], read back."""
        r = RangeRows()
        self._check(self._L.gwaoi_range_batch_device(self._w, C.c_void_p(d_q) if d_q else None, n, C.byref(r)))
        return r.offsets or 0, r.items or 0, r.dists or 0, _device_u32((r.offsets or 0) + 4 * r.n)

    def range_count_batch_device(self, d_q: int, n: int, d_out: int):
        """Queries and the n uint32 counts in device memory."""
        self._check(self._L.gwaoi_range_count_batch_device(self._w, C.c_void_p(d_q) if d_q else None, n,
                                                           C.c_void_p(d_out) if d_out else None))

    # ---- server-driven movement (include/gwaoi_sync.h)
    STEER_MOVE, STEER_FACE = STEER_MOVE, STEER_FACE

    def steer_batch(self, movers, targets, steps, flags=None):
        """Monster.Tick's chase and FaceTo for a batch (gwaoi_steer_batch): mover m steps steps[m]
        toward targets[m] (STEER_MOVE) and faces it (STEER_FACE) if it is interested in it on the
        relation of the last flush; flags=None: both for every message.  Returns (applied bool[n],
        pos float32[n, 4]: the movers' x, y, z, yaw after their message, zeros where none applied).
        The moves are queued: tick before the next read or collect.  When the device drops a message
        whose new position overflows, the GwaoiError raised carries the answers in .result."""
        mv = np.ascontiguousarray(np.atleast_1d(movers), np.uint32).reshape(-1)
        tg = np.ascontiguousarray(np.atleast_1d(targets), np.uint32).reshape(-1)
        st = np.ascontiguousarray(np.atleast_1d(steps), np.float32).reshape(-1)
        fl = None
        if flags is not None:
            fl = np.ascontiguousarray(np.atleast_1d(flags), np.uint32).reshape(-1)
        if tg.size != mv.size or st.size != mv.size or (fl is not None and fl.size != mv.size):
            raise ValueError(f"{mv.size} movers but {tg.size} targets, {st.size} steps and "
                             f"{'no' if fl is None else fl.size} flags")
        applied, pos = np.zeros(mv.size, np.uint8), np.zeros((mv.size, 4), np.float32)
        some = mv.size > 0
        rc = self._L.gwaoi_steer_batch(self._w, _p(mv) if some else None, _p(tg) if some else None,
                                       _p(st) if some else None, _p(fl) if some and fl is not None else None,
                                       mv.size, _p(applied) if some else None, _p(pos) if some else None)
        try:
            self._check(rc)
        except GwaoiError as e:
            e.result = (applied.astype(bool), pos)
            raise
        return applied.astype(bool), pos

    def steer_batch_device(self, d_movers: int, d_targets: int, d_steps: int, d_flags: int, n: int,
                           d_out_applied: int, d_out_pos: int):
        """Every array in device memory (d_flags 0: MOVE | FACE for every message); d_targets may be
        nearest_batch_device's output as it is.  The outputs (n bytes, 4n floats) are complete on
        return, also when a GwaoiError reports dropped messages."""
        q = [C.c_void_p(p) if p else None for p in (d_movers, d_targets, d_steps, d_flags, d_out_applied, d_out_pos)]
        self._check(self._L.gwaoi_steer_batch_device(self._w, q[0], q[1], q[2], q[3], n, q[4], q[5]))


_hip = None


def _device_u32(ptr: int) -> int:
    """One uint32 of device memory, through the HIP runtime this process already loaded."""
    global _hip
    if _hip is None:
        _hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line))
    v = C.c_uint32()
    rc = _hip.hipMemcpy(C.byref(v), C.c_void_p(ptr), C.c_size_t(4), 2)  # hipMemcpyDeviceToHost
    if rc != 0:
        raise GwaoiError(-5, f"hipMemcpy: {rc}")
    return v.value


def _ids(ids, n) -> np.ndarray:
    if isinstance(ids, np.ndarray):
        a = np.ascontiguousarray(ids, np.uint8).reshape(-1, 16)
    else:
        a = np.frombuffer(b"".join(bytes(i) for i in ids), np.uint8).reshape(-1, 16)
    if a.shape[0] != n:
        raise ValueError(f"expected {n} ids of 16 bytes")
    return np.ascontiguousarray(a)


def _gate_dict(g: GateRecords, rec: int) -> dict:
    out = {}
    if not g.n_gates:
        return out
    total = g.offsets[g.n_gates]
    buf = np.ctypeslib.as_array(C.cast(g.records, C.POINTER(C.c_uint8)), shape=(total * rec,)).copy() \
        if total else np.empty(0, np.uint8)
    for i in range(g.n_gates):
        a, b = g.offsets[i], g.offsets[i + 1]
        out[g.gate_ids[i]] = buf[a * rec:b * rec].reshape(-1, rec)
    return out


def pair_keys(pairs: np.ndarray) -> np.ndarray:
    """(n,2) uint32 pairs -> sorted uint64 keys a<<32|b."""
    if pairs.size == 0:
        return np.empty(0, np.uint64)
    k = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
    return np.sort(k)


class Wire:
    """The position-sync wire regroups of a gate or a dispatcher on the GPU
    (include/gwaoi_wire.h): GateService.handleSyncPositionYawFromClient +
    tryFlushPendingSyncPackets, DispatcherService.handleSyncPositionYawFromClient
    + sendEntitySyncInfosToGames, GateService.handleSyncPositionYawOnClients.
    Each regroup returns ``{destination key: bytes}`` (host) in key order."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = C.c_void_p()
        rc = self._L.gwaoi_wire_create(device, C.byref(h))
        if rc != 0:
            raise GwaoiError(rc, self._L.gwaoi_strerror(rc).decode())
        self._w = h

    def close(self):
        if getattr(self, "_w", None):
            self._L.gwaoi_wire_destroy(self._w)
            self._w = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise GwaoiError(rc, self._L.gwaoi_strerror(rc).decode() + " (" +
                             self._L.gwaoi_wire_last_error(self._w).decode() + ")")

    @staticmethod
    def _ids(ids) -> np.ndarray:
        a = np.ascontiguousarray(np.frombuffer(b"".join(ids), np.uint8) if isinstance(ids, (list, tuple))
                                 else np.asarray(ids, np.uint8))
        assert a.size % 16 == 0
        return a

    def set_entity_games(self, ids, games):
        a, g = self._ids(ids), np.ascontiguousarray(games, np.uint16)
        if a.size // 16 != g.size:
            raise ValueError(f"{a.size // 16} ids but {g.size} games")
        self._check(self._L.gwaoi_wire_set_entity_games(self._w, _p(a), _p(g), g.size))

    def remove_entities(self, ids):
        a = self._ids(ids)
        self._check(self._L.gwaoi_wire_remove_entities(self._w, _p(a), a.size // 16))

    def set_clients(self, ids, index):
        a, x = self._ids(ids), np.ascontiguousarray(index, np.uint32)
        if a.size // 16 != x.size:
            raise ValueError(f"{a.size // 16} ids but {x.size} client indices")
        self._check(self._L.gwaoi_wire_set_clients(self._w, _p(a), _p(x), x.size))

    def remove_clients(self, ids):
        a = self._ids(ids)
        self._check(self._L.gwaoi_wire_remove_clients(self._w, _p(a), a.size // 16))

    @staticmethod
    def _groups(g: WireGroups, on_device: bool):
        n = g.n_groups
        keys = np.ctypeslib.as_array(g.keys, shape=(n,)).copy() if n else np.empty(0, np.uint32)
        off = np.ctypeslib.as_array(g.offsets, shape=(n + 1,)).copy()
        if on_device:
            return keys, off, g.records, int(g.n_dropped)
        total = int(off[-1]) * g.rec_bytes
        buf = C.string_at(g.records, total) if total else b""
        return {int(k): buf[int(off[i]) * g.rec_bytes:int(off[i + 1]) * g.rec_bytes] for i, k in enumerate(keys)}, \
            int(g.n_dropped)

    def _call(self, fn, data, *extra, rec=32):
        buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
        assert buf.size % rec == 0
        g = WireGroups()
        self._check(fn(self._w, _p(buf) if buf.size else None, buf.size // rec, *extra, C.byref(g)))
        return self._groups(g, False)

    def gate_from_clients(self, records: bytes, n_dispatchers: int):
        return self._call(self._L.gwaoi_wire_gate_from_clients, records, n_dispatchers)

    def dispatcher_to_games(self, records: bytes):
        return self._call(self._L.gwaoi_wire_dispatcher_to_games, records)

    def gate_to_clients(self, records: bytes):
        return self._call(self._L.gwaoi_wire_gate_to_clients, records, rec=48)

    def _call_device(self, fn, d_ptr: int, n: int, *extra):
        g = WireGroups()
        self._check(fn(self._w, C.c_void_p(d_ptr) if n else None, n, *extra, C.byref(g)))
        return self._groups(g, True)

    def gate_from_clients_device(self, d_ptr: int, n: int, n_dispatchers: int):
        """(keys, offsets, device records pointer, n_dropped)."""
        return self._call_device(self._L.gwaoi_wire_gate_from_clients_device, d_ptr, n, n_dispatchers)

    def dispatcher_to_games_device(self, d_ptr: int, n: int):
        return self._call_device(self._L.gwaoi_wire_dispatcher_to_games_device, d_ptr, n)

    def gate_to_clients_device(self, d_ptr: int, n: int):
        return self._call_device(self._L.gwaoi_wire_gate_to_clients_device, d_ptr, n)
