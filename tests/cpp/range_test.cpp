// Stand-alone test of csrc/gwaoi_range.h: whenever a range read's hit predicate holds for a
// candidate, the candidate's cell lies inside the query's cell window (range_window), for drawn
// grids, centres, radii and candidates and for the adversarial ones: centre +- r +- 0..3 ulps,
// offsets of 1e-23 .. 1e-19 at r = 0 and r > 0, a centre at 0, a centre on a cell boundary, points
// beyond the grid on every side, r larger than the grid, r = 0.  It also counts how often a window
// without the margin (cell_of(c - r) .. cell_of(c + r)) would have lost a hit: the cases bite.
// Prints "ok <cases> <hits>".
#include "gwaoi_range.h"

#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>

using gw::cell_of;
using gw::range_hit;
using gw::range_window;
using gw::RangeWindow;

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static inline uint64_t rnd() {  // xorshift64*
    g_s ^= g_s >> 12;
    g_s ^= g_s << 25;
    g_s ^= g_s >> 27;
    return g_s * 0x2545F4914F6CDD1Dull;
}
static inline uint32_t rndn(uint32_t n) { return (uint32_t)((rnd() >> 32) * (uint64_t)n >> 32); }
static inline float uni(float a, float b) { return a + (b - a) * (float)((rnd() >> 40) * (1.0 / 16777216.0)); }
static inline float sgn() { return (rnd() & 1) ? 1.0f : -1.0f; }

static float ulps(float v, int k) {  // k steps of nextafter
    const float to = k > 0 ? INFINITY : -INFINITY;
    for (int i = 0; i < (k < 0 ? -k : k); ++i) v = std::nextafterf(v, to);
    return v;
}

struct Grid {
    float ox, oz, inv, C;
    uint32_t gx, gz;
};

enum Cls { C_ULP, C_TINY, C_IN, C_OUT, C_SAME, C_N };
static uint64_t g_cases[C_N], g_hits[C_N], g_fail, g_bare_miss;

static void check(const Grid &g, float cx, float cy, float cz, float r, float bx, float by, float bz, bool planar, Cls cls) {
    const RangeWindow W = range_window(cx, cz, r, g.ox, g.oz, g.inv, g.gx, g.gz);
    float d;
    ++g_cases[cls];
    if (!range_hit(cx, cy, cz, bx, by, bz, planar, r, &d)) return;
    ++g_hits[cls];
    const int kx = cell_of(bx, g.ox, g.inv, g.gx), kz = cell_of(bz, g.oz, g.inv, g.gz);
    if (kx < W.cx0 || kx > W.cx1 || kz < W.cz0 || kz > W.cz1) {
        if (g_fail++ < 10)
            std::printf("hit outside the window: c=(%a,%a,%a) r=%a b=(%a,%a,%a) planar=%d grid o=(%a,%a) inv=%a %ux%u "
                        "cell (%d,%d) window [%d,%d]x[%d,%d]\n",
                        cx, cy, cz, r, bx, by, bz, (int)planar, g.ox, g.oz, g.inv, g.gx, g.gz, kx, kz, W.cx0, W.cx1, W.cz0, W.cz1);
    }
    // the same hit against the window without a margin
    if (kx < cell_of(cx - r, g.ox, g.inv, g.gx) || kx > cell_of(cx + r, g.ox, g.inv, g.gx) ||
        kz < cell_of(cz - r, g.oz, g.inv, g.gz) || kz > cell_of(cz + r, g.oz, g.inv, g.gz))
        ++g_bare_miss;
}

int main() {
    const float tiny[] = {1e-23f, 3e-23f, 1e-22f, 1e-21f, 1e-20f, 1e-19f};
    const int GROUPS = 560000, PER = 20;  // 1.12e7 cases
    for (int it = 0; it < GROUPS; ++it) {
        // ---- a grid: origin, cell size (sometimes a power of two, so that bounds fall on cells exactly), extent
        Grid g;
        const uint32_t gm = rndn(4);
        g.C = gm == 0 ? std::ldexp(1.0f, (int)rndn(8) - 2) : uni(0.3f, 120.0f);
        g.inv = (float)(1.0 / (double)g.C);
        g.gx = 1 + rndn(gm == 1 ? 3 : 300);
        g.gz = 1 + rndn(gm == 1 ? 3 : 300);
        const float span_x = g.C * (float)g.gx, span_z = g.C * (float)g.gz;
        g.ox = gm == 0 ? std::floor(uni(-2000.f, 2000.f)) : (gm == 2 ? 0.0f : uni(-5000.f, 5000.f));
        g.oz = gm == 0 ? std::floor(uni(-2000.f, 2000.f)) : (gm == 2 ? 0.0f : uni(-5000.f, 5000.f));
        // ---- a centre
        float cx, cz;
        switch (rndn(6)) {
        case 0: cx = 0.0f; cz = rndn(2) ? 0.0f : uni(g.oz, g.oz + span_z); break;             // at 0
        case 1: cx = g.ox + g.C * (float)rndn(g.gx + 1); cz = g.oz + g.C * (float)rndn(g.gz + 1); break;  // on a cell boundary
        case 2: cx = g.ox + (rndn(2) ? -1.0f : 1.0f + span_x / 1e6f) * 1e6f; cz = uni(g.oz, g.oz + span_z); break;  // beyond, x
        case 3: cx = uni(g.ox, g.ox + span_x); cz = g.oz + (rndn(2) ? -1e6f : span_z + 1e6f); break;      // beyond, z
        default: cx = uni(g.ox, g.ox + span_x); cz = uni(g.oz, g.oz + span_z); break;
        }
        const float cy = rndn(3) ? uni(-10.f, 10.f) : 0.0f;
        // ---- a radius
        float r;
        switch (rndn(8)) {
        case 0: r = 0.0f; break;
        case 1: r = tiny[rndn(6)]; break;
        case 2: r = g.C * (float)(1 + rndn(4)); break;            // whole cells
        case 3: r = 4.0f * (span_x + span_z) + 1.0f; break;       // larger than the grid
        case 4: r = rndn(2) ? 3e38f : 3e6f; break;
        case 5: r = uni(0.f, 3.0f); break;
        default: r = uni(0.f, 2.5f * g.C + 50.f); break;
        }
        for (int k = 0; k < PER; ++k) {
            const bool planar = rnd() & 1;
            float bx = cx, bz = cz, by = cy;
            Cls cls;
            const uint32_t m = rndn(10);
            if (m < 4) {  // on the rim: c +- r +- 0..3 ulps on one axis, the other axis equal, tiny or free
                cls = C_ULP;
                const int k1 = (int)rndn(7) - 3;
                float &a = (rnd() & 1) ? bx : bz;
                float &o = (&a == &bx) ? bz : bx;
                a = ulps(a + sgn() * r, k1);
                const uint32_t om = rndn(4);
                if (om == 1) o = o + sgn() * tiny[rndn(6)];
                if (om == 2) o = ulps(o, (int)rndn(7) - 3);
                if (om == 3 && r > 0) {  // a diagonal on the rim
                    const float t = uni(0.f, 6.2831853f);
                    bx = ulps(cx + r * std::cos(t), (int)rndn(7) - 3);
                    bz = ulps(cz + r * std::sin(t), (int)rndn(7) - 3);
                }
                if (!planar && rndn(2)) by = cy + sgn() * tiny[rndn(6)];
            } else if (m < 6) {  // offsets whose squares underflow
                cls = C_TINY;
                if (rndn(3)) bx = cx + sgn() * tiny[rndn(6)];
                if (rndn(3)) bz = cz + sgn() * tiny[rndn(6)];
                if (rndn(3)) by = cy + sgn() * tiny[rndn(6)];
                if (r > 0 && rndn(2)) bx = bx + sgn() * r;
            } else if (m < 8) {  // anywhere in the grid, or within r of the centre
                cls = C_IN;
                if (rndn(2)) {
                    bx = uni(g.ox, g.ox + span_x);
                    bz = uni(g.oz, g.oz + span_z);
                } else {
                    const float rr = r < 1e30f ? r : 1e6f;
                    bx = cx + uni(-rr, rr);
                    bz = cz + uni(-rr, rr);
                }
                by = cy + uni(-3.f, 3.f);
            } else if (m < 9) {  // beyond the grid on one side
                cls = C_OUT;
                const float far = rndn(2) ? 1e6f : uni(0.f, 2.0f * g.C);
                switch (rndn(4)) {
                case 0: bx = g.ox - far; bz = uni(g.oz, g.oz + span_z); break;
                case 1: bx = g.ox + span_x + far; bz = uni(g.oz, g.oz + span_z); break;
                case 2: bz = g.oz - far; bx = uni(g.ox, g.ox + span_x); break;
                default: bz = g.oz + span_z + far; bx = uni(g.ox, g.ox + span_x); break;
                }
            } else {
                cls = C_SAME;  // on the centre: a hit at every r
            }
            check(g, cx, cy, cz, r, bx, by, bz, planar, cls);
        }
    }
    uint64_t cases = 0, hits = 0;
    for (int c = 0; c < C_N; ++c) {
        cases += g_cases[c];
        hits += g_hits[c];
        // every class both hits and misses, so the predicate is exercised on both sides
        if (g_hits[c] == 0 || (c != C_SAME && g_hits[c] == g_cases[c])) {
            std::printf("class %d: %" PRIu64 " hits of %" PRIu64 " cases\n", c, g_hits[c], g_cases[c]);
            ++g_fail;
        }
    }
    if (g_hits[C_SAME] != g_cases[C_SAME]) {
        std::printf("a candidate on the centre missed\n");
        ++g_fail;
    }
    if (cases < 10000000ull) {
        std::printf("only %" PRIu64 " cases\n", cases);
        ++g_fail;
    }
    if (g_bare_miss == 0) {
        std::printf("no case needed the margin: the draw has lost its teeth\n");
        ++g_fail;
    }
    if (g_fail) {
        std::printf("%" PRIu64 " failures (rim %" PRIu64 "/%" PRIu64 ", tiny %" PRIu64 "/%" PRIu64 ")\n", g_fail, g_hits[C_ULP],
                    g_cases[C_ULP], g_hits[C_TINY], g_cases[C_TINY]);
        return 1;
    }
    std::printf("ok %" PRIu64 " %" PRIu64 " margin-needed %" PRIu64 "\n", cases, hits, g_bare_miss);
    return 0;
}
