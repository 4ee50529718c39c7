// c2d_poly_broad.hip — broad-phase convex polygon pair search for gfx950 (MI355X): the pair list of c2d_sat_poly_cross_pairs
// (row_base = col_base = 0), bit for bit, through the pipeline of c2d_broad.hip (c2d_broad.hpp) with the polygon policy below.
//
// The policy:
//   box      the box of a parallelogram U whose edge normals are two of the polygon's OWN test axes, each interval widened by the
//            rounding bound of §5.8: if box(U_A) and box(U_B) are disjoint, one of those four axes separates A and B in the
//            computed test.  The two axes are the normals of the first usable edge p (|e|_1 >= 2^-80) and of the edge q that
//            maximises |det(e_p, e_q)| / |e_q|_1, decided in double.  The box itself is broad_box_of_slabs, shared with the
//            rectangles.
//   wild     a non-finite real vertex or a |coordinate| >= 2^60, fewer than three vertices, no usable edge pair, a box that is not
//            finite (and, in the pipeline, a box that spans more than two cells): tested against everything, which is what keeps
//            the "collide with far-away things" of points and segments.
//   absent   a vertex count outside 1..rows: in no pair, not counted, reported through the ctx's asynchronous error word like the
//            cross form.
//   collide  poly_collide (c2d_poly_pair.hpp), one pair per lane: the lanes of a wave hold unrelated candidates here.
// Padded vertex slots (index >= the count) are never read.
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

struct PolyBroadSet {
    PolySetDev set;
    uint32_t* async_err;   // the ctx's asynchronous error word (pinned host memory)
};

// the polygon policy of the pipeline (c2d_broad.hpp)
struct PolyShape {
    using Set = PolyBroadSet;
    using Obj = PolyObj;
    static C2D_DEV void load(const Set& X, size_t i, Obj& o) { poly_load(X.set, i, o); }
    static C2D_DEV int box(const Set& X, size_t i, float4& b)
    {
        int k;
        if (!poly_count(X.set, i, k)) {
            __hip_atomic_fetch_or(X.async_err, C2D_ASYNC_ERR_POLY_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return kBroadAbsent;
        }
        PolyObj p;
        poly_load(X.set, i, p);
        return poly_broad_box(p, b) ? kBroadRegular : kBroadWild;
    }
    static C2D_DEV bool collide(const Obj& a, const Obj& b) { return poly_collide(a, b); }
};

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_sat_poly_broad_pairs(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, int flags, uint32_t* d_pairs, size_t capacity,
                             unsigned long long* d_count, c2d_stream stream)
{
    const char* what = "c2d_sat_poly_broad_pairs";
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!a || !b) return fail_arg(ctx, "c2d_sat_poly_broad_pairs: NULL set");
    if (a->n == 0 || b->n == 0) return C2D_OK;
    PolyBroadSet A, B;
    if (int rc = poly_set_check(ctx, what, "a", a, A.set)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B.set)) return rc;
    if (int rc = broad_check_list(ctx, what, flags, d_pairs, capacity, d_count, A.set.n, B.set.n)) return rc;
    A.async_err = B.async_err = ctx->d_async_err;
    const bool same = A.set.vx == B.set.vx && A.set.vy == B.set.vy && A.set.k == B.set.k && A.set.n == B.set.n && A.set.stride == B.set.stride &&
                      A.set.rows == B.set.rows;
    DeviceGuard dg(ctx->device);
    return broad_run<PolyShape>(ctx, (hipStream_t)stream, what, A, A.set.n, B, B.set.n, same, flags, d_pairs, capacity, d_count);
}

}  // extern "C"
