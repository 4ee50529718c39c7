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
#include "c2d_poly_broad_box.hpp"   // poly_broad_box, shared with c2d_near_broad.hip
#include "c2d_poly_pair.hpp"

namespace c2d {

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
    DeviceGuard dg(ctx->device);
    return broad_run<PolyShape>(ctx, (hipStream_t)stream, what, A, A.set.n, B, B.set.n, poly_sets_same(A.set, B.set), flags, d_pairs, capacity, d_count);
}

}  // extern "C"
