// c2d_sweep_shape.hpp — the moving-polygon policy of the pipeline of c2d_broad.hpp, stated once for the two
// translation units that search on swept boxes: c2d_sweep_broad.hip (every pair that touches in a step) and c2d_cast_grid.hip (the
// polygon each moving polygon touches first).  The motion rides in Set and Obj: collide sees only the two objects.
//
// The policy:
//   box      the hull of the box of §5.10's parallelogram U (two of the polygon's OWN test axes, chosen as poly_broad_box chooses
//            them) at t = 0 and of the same box displaced by the polygon's motion (dx, dy), in double, rounded outward to float.
//            The slabs are widened by W = |e|_1 (2^-21 C + 2^-17 D + 2^-66) + 2^-140 with C the largest |coordinate| and D the
//            larger |motion component|: the 2^-17 D term is what the sweep rule's own roundings (r, v, the quotients) need.  If
//            the swept boxes of two regular polygons are disjoint, the computed pick of the pair misses.
//   wild     what §5.10 calls wild (a non-finite real vertex or a |coordinate| >= 2^60, fewer than three vertices, no usable edge
//            pair, a box that is not finite, and, in the pipeline, a box that spans more than two cells), plus a non-finite motion
//            component, a |motion component| >= 2^60 and a displaced |coordinate| >= 2^60: tested against everything.
//   absent   a vertex count outside 1..rows: in no pair, not counted, reported through the ctx's asynchronous error word.
//   collide  the `hit` of the sweep record: the axis walk of c2d_pair_list.hpp into the pick of c2d_sweep_rule.hpp, one pair per
//            lane, hit0 || (!never && t_in <= t_out).  The lanes of a wave hold unrelated candidates: nothing here is wave-uniform.
// Padded vertex slots (index >= the count) are never read; the motion planes are read at indices below n only.
#pragma once

#include "c2d_broad.hpp"
#include "c2d_sweep_rule.hpp"   // SweepPick, sweep_motion_check; through it c2d_pair_list.hpp: MovingShape, poly_axes

namespace c2d {

using PolySweepShape = MovingShape<PolyListShape>;

// The widening of a moving object's own interval on one of its axes a: §5.8's widening plus 2^-17 |a|_1 D.
C2D_DEV double sweep_slab_widening(double n1, double C, double D) { return n1 * (0x1p-21 * C + 0x1p-17 * D + 0x1p-66) + 0x1p-140; }

// The swept conservative box of polygon P (k >= 1 real vertices, neutral padding) with its motion, or false: wild.
C2D_DEV bool poly_sweep_box(const PolySweepShape::Obj& P, float4& box)
{
    if (P.k < 3) return false;
    if (!__builtin_isfinite(P.dx) || !__builtin_isfinite(P.dy)) return false;
    const float dmax = __builtin_fmaxf(__builtin_fabsf(P.dx), __builtin_fabsf(P.dy));
    if (!(dmax < 0x1p60f)) return false;
    float cmax = 0.0f;
    double moved = 0.0;   // the largest displaced |coordinate| (each sum one double rounding)
    bool finite = true;
#pragma unroll
    for (int r = 0; r < C2D_POLY_KMAX; r++) {
        finite = finite && __builtin_isfinite(P.x[r]) && __builtin_isfinite(P.y[r]);
        cmax = __builtin_fmaxf(cmax, __builtin_fmaxf(__builtin_fabsf(P.x[r]), __builtin_fabsf(P.y[r])));
        moved = __builtin_fmax(moved, __builtin_fmax(__builtin_fabs((double)P.x[r] + (double)P.dx), __builtin_fabs((double)P.y[r] + (double)P.dy)));
    }
    if (!finite || !(cmax < 0x1p60f) || !(moved < 0x1p60)) return false;
    const double C = cmax, D = dmax;
    // p: the first usable edge; q: the usable edge behind it with the largest |det(e_p, e_q)| / |e_q|_1, as poly_broad_box
    // (c2d_poly_broad.hip) chooses them.  Edges are the float differences the test's normals are made of.
    double ex[2] = {0.0, 0.0}, ey[2] = {0.0, 0.0}, n1[2] = {0.0, 0.0}, best = 0.0;
    bool have_p = false;
#pragma unroll
    for (int m = 0; m < C2D_POLY_KMAX; m++) {
        const int m1 = (m + 1) & (C2D_POLY_KMAX - 1);
        const double dx = (double)(P.x[m1] - P.x[m]), dy = (double)(P.y[m1] - P.y[m]);
        const double l1 = __builtin_fabs(dx) + __builtin_fabs(dy);
        if (!(l1 >= 0x1p-80)) continue;
        if (!have_p) {
            have_p = true;
            ex[0] = dx; ey[0] = dy; n1[0] = l1;
        } else {
            const double score = __builtin_fabs(ex[0] * dy - ey[0] * dx) / l1;
            if (score > best) {
                best = score;
                ex[1] = dx; ey[1] = dy; n1[1] = l1;
            }
        }
    }
    if (!(best > 0.0)) return false;   // no usable edge, or every usable edge parallel to the first
    double ax[2], ay[2], slo[2], shi[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        ax[i] = -ey[i];
        ay[i] = ex[i];
        double lo = ax[i] * (double)P.x[0] + ay[i] * (double)P.y[0], hi = lo;
#pragma unroll
        for (int v = 1; v < C2D_POLY_KMAX; v++) {
            const double p = ax[i] * (double)P.x[v] + ay[i] * (double)P.y[v];
            lo = p < lo ? p : lo;
            hi = p > hi ? p : hi;
        }
        const double w = sweep_slab_widening(n1[i], C, D);
        slo[i] = lo - w;
        shi[i] = hi + w;
    }
    float4 b0;
    if (!broad_box_of_slabs(ax, ay, slo, shi, b0)) return false;
    // The hull of b0 and b0 + (dx, dy).  A corner plus a displacement is one double rounding; 2^-52 of the sum covers it.
    const double ddx = (double)P.dx, ddy = (double)P.dy;
    const double x0 = (double)b0.x + ddx, y0 = (double)b0.y + ddy, x1 = (double)b0.z + ddx, y1 = (double)b0.w + ddy;
    const float mx0 = round_down(x0 - 0x1p-52 * __builtin_fabs(x0)), my0 = round_down(y0 - 0x1p-52 * __builtin_fabs(y0));
    const float mx1 = round_up(x1 + 0x1p-52 * __builtin_fabs(x1)), my1 = round_up(y1 + 0x1p-52 * __builtin_fabs(y1));
    box = make_float4(__builtin_fminf(b0.x, mx0), __builtin_fminf(b0.y, my0), __builtin_fmaxf(b0.z, mx1), __builtin_fmaxf(b0.w, my1));
    return __builtin_isfinite(box.x) && __builtin_isfinite(box.y) && __builtin_isfinite(box.z) && __builtin_isfinite(box.w);
}

struct PolySweepBroadSet {
    PolySweepShape::Set set;   // the polygons and their two motion planes (both nullptr: the set stands still)
    uint32_t* async_err;       // the ctx's asynchronous error word (pinned host memory)
};

// the moving-polygon policy of the pipeline (c2d_broad.hpp)
struct PolySweepBroadShape {
    using Set = PolySweepBroadSet;
    using Obj = PolySweepShape::Obj;
    static C2D_DEV void load(const Set& X, size_t i, Obj& o) { PolySweepShape::load(X.set, i, o); }
    static C2D_DEV int box(const Set& X, size_t i, float4& b)
    {
        if (!PolySweepShape::present(X.set, i)) {
            __hip_atomic_fetch_or(X.async_err, C2D_ASYNC_ERR_POLY_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return kBroadAbsent;
        }
        Obj p;
        PolySweepShape::load(X.set, i, p);
        return poly_sweep_box(p, b) ? kBroadRegular : kBroadWild;
    }
    // the `hit` of SweepWork::pair (c2d_sweep.hip) without its wave-uniform shortcut: one walk gives the pairwise boolean and the pick
    static C2D_DEV bool collide(const Obj& a, const Obj& b)
    {
        SweepPick pick{b.dx - a.dx, b.dy - a.dy};
        const bool hit0 = PolySweepShape::axes(a, b, pick);
        return hit0 || (!pick.never && pick.t_in <= pick.t_out);
    }
};

}  // namespace c2d
