// c2d_poly_broad_box.hpp — the own-axes box of a convex polygon, stated once for the broad phases whose exact test
// holds the pairwise test of c2d_poly_pair.hpp (c2d_poly_broad.hip: the static pair search; c2d_near_broad.hip: the proximity pair
// search): if the boxes of two polygons are disjoint, the computed pairwise test of the pair misses.
#pragma once

#include "c2d_broad.hpp"
#include "c2d_poly_pair.hpp"

namespace c2d {

// The conservative box of polygon P (k >= 1 real vertices, neutral padding), or false: wild.  Padding repeats vertex 0, so loops
// over all 16 slots see the real vertices' values only, and a padding edge has length zero and is never usable.
C2D_DEV bool poly_broad_box(const PolyObj& P, float4& box)
{
    if (P.k < 3) return false;
    float cmax = 0.0f;
    bool finite = true;
#pragma unroll
    for (int r = 0; r < C2D_POLY_KMAX; r++) {
        finite = finite && __builtin_isfinite(P.x[r]) && __builtin_isfinite(P.y[r]);
        cmax = __builtin_fmaxf(cmax, __builtin_fmaxf(__builtin_fabsf(P.x[r]), __builtin_fabsf(P.y[r])));
    }
    if (!finite || !(cmax < 0x1p60f)) return false;
    const double C = cmax;
    // p: the first usable edge; q: the usable edge behind it with the largest |det(e_p, e_q)| / |e_q|_1 (every edge in front of p is
    // unusable).  Edges are the float differences the test's normals are made of.
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
        ax[i] = -ey[i];   // the test's axis of the edge: its normal (-e.y, e.x); |n|_1 = |e|_1
        ay[i] = ex[i];
        double lo = ax[i] * (double)P.x[0] + ay[i] * (double)P.y[0], hi = lo;   // products exact in double, one rounding each sum
#pragma unroll
        for (int v = 1; v < C2D_POLY_KMAX; v++) {
            const double p = ax[i] * (double)P.x[v] + ay[i] * (double)P.y[v];
            lo = p < lo ? p : lo;
            hi = p > hi ? p : hi;
        }
        const double w = broad_slab_widening(n1[i], C);
        slo[i] = lo - w;
        shi[i] = hi + w;
    }
    return broad_box_of_slabs(ax, ay, slo, shi, box);
}

}  // namespace c2d
