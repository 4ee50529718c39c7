// c2d_sweep_broad.hip — swept broad-phase convex polygon pair search for gfx950 (MI355X): every pair (i, j) of two polygon sets in
// linear motion over the step t = 0 .. 1 whose c2d_poly_pair_sweeps record has hit == 1 (row_base = col_base = 0), in row-major order,
// bit for bit, through the pipeline of c2d_broad.hip (c2d_broad.hpp) with the moving-polygon policy.
//
// The policy — the swept box, what is wild, what is absent, the exact test — is PolySweepBroadShape (c2d_sweep_shape.hpp),
// shared with c2d_cast_grid.hip.
#include "c2d_sweep_shape.hpp"

using namespace c2d;

extern "C" {

int c2d_poly_sweep_broad_pairs(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, const float* d_a_dx, const float* d_a_dy, const float* d_b_dx,
                               const float* d_b_dy, int flags, uint32_t* d_pairs, size_t capacity, unsigned long long* d_count, c2d_stream stream)
{
    const char* what = "c2d_poly_sweep_broad_pairs";
    if (int rc = sweep_motion_check(ctx, what, d_a_dx, d_a_dy, d_b_dx, d_b_dy)) return rc;
    if (!a || !b) return fail_arg(ctx, "c2d_poly_sweep_broad_pairs: NULL set");
    if (a->n == 0 || b->n == 0) return C2D_OK;
    PolySweepBroadSet A, B;
    if (int rc = poly_set_check(ctx, what, "a", a, A.set.s)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B.set.s)) return rc;
    if (int rc = broad_check_list(ctx, what, flags, d_pairs, capacity, d_count, A.set.s.n, B.set.s.n)) return rc;
    A.set.dx = d_a_dx;
    A.set.dy = d_a_dy;
    B.set.dx = d_b_dx;
    B.set.dy = d_b_dy;
    A.async_err = B.async_err = ctx->d_async_err;
    // one set against itself only when it moves as itself: the boxes are swept boxes
    const bool same = poly_sets_same(A.set.s, B.set.s) && d_a_dx == d_b_dx && d_a_dy == d_b_dy;
    DeviceGuard dg(ctx->device);
    return broad_run<PolySweepBroadShape>(ctx, (hipStream_t)stream, what, A, A.set.s.n, B, B.set.s.n, same, flags, d_pairs, capacity, d_count);
}

}  // extern "C"
