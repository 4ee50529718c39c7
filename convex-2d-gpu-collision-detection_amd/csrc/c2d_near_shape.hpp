// c2d_near_shape.hpp — the margin policy of the pipeline of c2d_broad.hpp, stated once for the two translation units
// that search under a margin: c2d_near_broad.hip (every pair within a distance) and c2d_clearance_grid.hip (the nearest polygon within
// a distance).  The margin rides in Set and Obj: collide sees only the two objects.
//
// The policy:
//   box      the hull of two boxes, in float, rounded outward.  (1) §5.10's own-axes box (poly_broad_box): disjoint boxes give a
//            computed miss of the pairwise test.  (2) The exact float box of the live vertices, widened on every side by the
//            half-margin h = near_half_margin(r, C), C the polygon's largest |coordinate|: if the widened boxes of two regular
//            polygons are disjoint, every usable candidate (edge, vertex) of the pair has sqrtf(d2) > r.
//   wild     what §5.10 calls wild (a non-finite real vertex or a |coordinate| >= 2^60, fewer than three vertices, no usable edge
//            pair, a box that is not finite, and, in the pipeline, a box that spans more than two cells), plus a largest |coordinate|
//            below 2^-100 (outside the domain of c2d_clearance_bound.hpp's proof): tested against everything.
//   absent   a vertex count outside 1..rows: in no pair, not counted, reported through the ctx's asynchronous error word.
//   collide  the pairwise test of the contact and distance kernels (poly_collide), or the pick of c2d_distance_rule.hpp over both
//            sides with a usable candidate and sqrtf(best) <= r: the record's own dist, compared as the contract compares it.  One
//            pair per lane; the lanes of a wave hold unrelated candidates: nothing here is wave-uniform.
// Padded vertex slots (index >= the count) are never read.
#pragma once

#include "c2d_broad.hpp"
#include "c2d_distance_rule.hpp"
#include "c2d_poly_broad_box.hpp"
#include "c2d_poly_pair.hpp"

namespace c2d {

constexpr float kNearMaxDist = 0x1p60f;   // max_dist stays below it
constexpr float kNearCMin = 0x1p-100f;    // the domain of c2d_clearance_bound.hpp's proof begins here (kClearanceCMin)

// The half-margin of a polygon with largest |coordinate| C under the margin r (DESIGN.md §5.20 part 2): two of them pay
//   r (1 + 2^-19) + [r < 2^-60: r] + 2^-72   the margin itself through the square / square-root pair at the end of the chain (a margin
//                                            below 2^-60 is doubled: its square is subnormal or underflows),
//   2^-20 (C_A + C_B)                        c2d_clearance_bound.hpp's 8 u max(C_A, C_B) and the roundings of the float gap and of L.
C2D_DEV double near_half_margin(double r, double C) { return 0.5 * (r * (1.0 + 0x1p-19) + (r < 0x1p-60 ? r : 0.0) + 0x1p-72) + 0x1p-20 * C; }

struct PolyNearSet {
    PolySetDev set;
    float r;               // max_dist (finite, 0 <= r < 2^60, never -0)
    uint32_t* async_err;   // the ctx's asynchronous error word (pinned host memory)
};

struct PolyNearObj : PolyObj {
    float r;
};

// The conservative box of polygon P under its margin, or false: wild.  Padding repeats vertex 0, so the loop over all 16 slots sees
// the live vertices' values only.
C2D_DEV bool poly_near_box(const PolyNearObj& P, float4& box)
{
    float4 own;
    if (!poly_broad_box(P, own)) return false;   // (finite live vertices with every |coordinate| < 2^60 from here on)
    float cmax = 0.0f, xlo = P.x[0], xhi = P.x[0], ylo = P.y[0], yhi = P.y[0];
#pragma unroll
    for (int v = 0; v < C2D_POLY_KMAX; v++) {
        cmax = __builtin_fmaxf(cmax, __builtin_fmaxf(__builtin_fabsf(P.x[v]), __builtin_fabsf(P.y[v])));
        xlo = __builtin_fminf(xlo, P.x[v]);
        xhi = __builtin_fmaxf(xhi, P.x[v]);
        ylo = __builtin_fminf(ylo, P.y[v]);
        yhi = __builtin_fmaxf(yhi, P.y[v]);
    }
    if (!(cmax >= kNearCMin)) return false;
    const double h = near_half_margin((double)P.r, (double)cmax);
    // a float bound plus or minus h is one double rounding; round_down / round_up then leave the exact sum inside the box only if
    // that rounding went outward, so 2^-52 of the sum is added first
    const double x0 = (double)xlo - h, y0 = (double)ylo - h, x1 = (double)xhi + h, y1 = (double)yhi + h;
    const float wx0 = round_down(x0 - 0x1p-52 * __builtin_fabs(x0)), wy0 = round_down(y0 - 0x1p-52 * __builtin_fabs(y0));
    const float wx1 = round_up(x1 + 0x1p-52 * __builtin_fabs(x1)), wy1 = round_up(y1 + 0x1p-52 * __builtin_fabs(y1));
    box = make_float4(__builtin_fminf(own.x, wx0), __builtin_fminf(own.y, wy0), __builtin_fmaxf(own.z, wx1), __builtin_fmaxf(own.w, wy1));
    return __builtin_isfinite(box.x) && __builtin_isfinite(box.y) && __builtin_isfinite(box.z) && __builtin_isfinite(box.w);
}

// the margin policy of the pipeline (c2d_broad.hpp)
struct PolyNearShape {
    using Set = PolyNearSet;
    using Obj = PolyNearObj;
    static C2D_DEV void load(const Set& X, size_t i, Obj& o)
    {
        poly_load(X.set, i, o);
        o.r = X.r;
    }
    static C2D_DEV int box(const Set& X, size_t i, float4& b)
    {
        int k;
        if (!poly_count(X.set, i, k)) {
            __hip_atomic_fetch_or(X.async_err, C2D_ASYNC_ERR_POLY_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return kBroadAbsent;
        }
        Obj p;
        load(X, i, p);
        return poly_near_box(p, b) ? kBroadRegular : kBroadWild;
    }
    // hit || dist <= r of the pair's distance record (DistanceWork::pair, c2d_distance.hip) without its wave-uniform shortcut
    static C2D_DEV bool collide(const Obj& a, const Obj& b)
    {
        if (poly_collide(a, b)) return true;
        PolyObj p = a, q = b;   // distance_side turns its edge polygon
        DistancePick pick;
        distance_side<C2D_POLY_KMAX>(p.x, p.y, p.k, q.x, q.y, q.k, 0u, pick);
        distance_side<C2D_POLY_KMAX>(q.x, q.y, q.k, p.x, p.y, p.k, kDistanceSide1, pick);
        return pick.code != kDistanceNone && __builtin_sqrtf(pick.best) <= a.r;
    }
};

}  // namespace c2d
