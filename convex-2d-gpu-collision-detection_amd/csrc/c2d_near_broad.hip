// c2d_near_broad.hip — proximity pair search for gfx950 (MI355X): every pair (i, j) of two polygon sets whose c2d_poly_pair_distances
// record (row_base = col_base = 0) has hit == 1 or dist <= max_dist, in row-major order, bit for bit, through the pipeline of
// c2d_broad.hip (c2d_broad.hpp) with the margin policy of c2d_near_shape.hpp (box, wild, absent, collide: DESIGN.md §5.20), which
// c2d_clearance_grid.hip shares.
#include "c2d_near_shape.hpp"

using namespace c2d;

extern "C" {

int c2d_poly_near_broad_pairs(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, float max_dist, int flags, uint32_t* d_pairs, size_t capacity,
                              unsigned long long* d_count, c2d_stream stream)
{
    const char* what = "c2d_poly_near_broad_pairs";
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!(max_dist >= 0.0f && max_dist < kNearMaxDist)) return fail_arg(ctx, "c2d_poly_near_broad_pairs: max_dist must be finite with 0 <= max_dist < 2^60");
    if (!a || !b) return fail_arg(ctx, "c2d_poly_near_broad_pairs: NULL set");
    if (a->n == 0 || b->n == 0) return C2D_OK;
    PolyNearSet A, B;
    if (int rc = poly_set_check(ctx, what, "a", a, A.set)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B.set)) return rc;
    if (int rc = broad_check_list(ctx, what, flags, d_pairs, capacity, d_count, A.set.n, B.set.n)) return rc;
    A.r = B.r = max_dist + 0.0f;   // -0 counts as 0
    A.async_err = B.async_err = ctx->d_async_err;
    DeviceGuard dg(ctx->device);
    return broad_run<PolyNearShape>(ctx, (hipStream_t)stream, what, A, A.set.n, B, B.set.n, poly_sets_same(A.set, B.set), flags, d_pairs, capacity, d_count);
}

}  // extern "C"
