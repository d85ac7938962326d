// The grid's cell function and the arithmetic of a range read (gwaoi_range_batch): the distance,
// the hit predicate and the cell window that is certain to hold every hit.  Plain values in, plain
// values out, __host__ __device__ under hipcc and ordinary inline functions without it, so
// tests/cpp/range_test.cpp checks window against predicate on the host (build with
// -ffp-contract=off, as the library is).  DESIGN.md §3l has the argument.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GW_HD __host__ __device__ __forceinline__
#else
#define GW_HD inline
#endif

namespace gw {

// Monotone non-decreasing in v (IEEE sub/mul round monotonically; clamp is
// monotone).  keygen and every query use this one function.
GW_HD int cell_of(float v, float o, float inv, uint32_t g) {
    float t = (v - o) * inv;
    t = fmaxf(t, 0.0f);
    t = fminf(t, (float)(g - 1));
    return (int)t;
}

// Vector3.DistanceTo's sum (Vector3.go:22-28), float32 step by step; planar leaves the dy term out.
GW_HD float range_d2(float dx, float dy, float dz, bool planar) {
    return planar ? dx * dx + dz * dz : (dx * dx + dy * dy) + dz * dz;
}
GW_HD float range_dist(float d2) { return (float)sqrt((double)d2); }

// Candidate b against centre c and radius r: its DistanceTo, and `dist <= r` in float32.
GW_HD bool range_hit(float cx, float cy, float cz, float bx, float by, float bz, bool planar, float r, float *dist) {
    *dist = range_dist(range_d2(bx - cx, by - cy, bz - cz, planar));
    return *dist <= r;
}

// What the window reaches past c -+ r on one axis.  A hit has |b - c| <= r (1 + 2^-21) + 2.6e-23
// (DESIGN §3l): the relative term covers the roundings of the distance and of the bounds
// themselves, the absolute one the squares that underflow.
GW_HD float range_margin(float c, float r) { return (fabsf(c) + r) * 0x1p-20f + 1e-18f; }

struct RangeWindow {
    int cx0, cx1, cz0, cz1;  // cells [cx0, cx1] x [cz0, cz1] of the grid, clamped to it
};

// The cells of grid (ox, oz, 1 / cell size, gx x gz) that hold every hit of centre (cx, cz),
// radius r >= 0 (finite).  A bound that overflows is +-inf, which cell_of clamps.
GW_HD RangeWindow range_window(float cx, float cz, float r, float ox, float oz, float inv, uint32_t gx, uint32_t gz) {
    const float mx = range_margin(cx, r), mz = range_margin(cz, r);
    RangeWindow W;
    W.cx0 = cell_of(cx - r - mx, ox, inv, gx);
    W.cx1 = cell_of(cx + r + mx, ox, inv, gx);
    W.cz0 = cell_of(cz - r - mz, oz, inv, gz);
    W.cz1 = cell_of(cz + r + mz, oz, inv, gz);
    return W;
}

}  // namespace gw
