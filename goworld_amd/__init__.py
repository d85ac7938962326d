"""goworld_amd -- MI355X-native AOI (area-of-interest) engine for GoWorld.

The one hot path accelerated here is go-aoi's XZListAOIManager as GoWorld's
engine/entity.Space drives it (Space.go:105,211,221,243,259).  The product is
the C-ABI library libgwaoi.so (include/gwaoi.h, HIP kernels for gfx950);
this package holds its ctypes binding (``_lib``), the host-side mirror of the
go-aoi interface (``aoi``), the seeded workloads (``workload``) and the
in-tree build (``build``).
"""
from ._lib import (CAST_DTYPE, CAST_NEIGHBORS, CAST_OWN, CAST_REC, NO_SLOT, RANGE_PLANAR, RANGE_POINT, RANGE_QUERY,  # noqa: F401
                   STEER_FACE, STEER_MOVE, GwaoiError, Wire, World, load, pair_keys)

__all__ = ["World", "Wire", "GwaoiError", "load", "pair_keys", "CAST_REC", "CAST_DTYPE", "CAST_OWN",
           "CAST_NEIGHBORS", "NO_SLOT", "STEER_MOVE", "STEER_FACE", "RANGE_QUERY", "RANGE_POINT", "RANGE_PLANAR"]
