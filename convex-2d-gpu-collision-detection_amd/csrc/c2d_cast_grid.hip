// c2d_cast_grid.hip — grid shape casts for gfx950 (MI355X): c2d_poly_set_casts_grid (include/c2d.h "shape casts through a grid",
// DESIGN.md §5.22).  For every polygon A_i of a set, moving over the step t = 0 .. 1, the polygon of a set B (moving too, or at rest)
// that it touches first, with the pair's whole sweep record: the output of c2d_poly_set_casts (c2d_cast.hip), byte for byte, found
// through the grid of the pair searches on swept boxes instead of a visit to every polygon.
//
// The rule is c2d_cast.hip's.  S(i, j) is the c2d_sweep record of (A_i, B_j) with the call's motion planes.  Polygon j is considered
// when its vertex count is within 1..rows and it is not the self pair (C2D_CAST_SKIP_SELF: row_base + i == col_base + j).  The winner
// is the considered j with S(i, j).hit == 1 and the smallest key (bits of S(i, j).toi) << 32 | (col_base + j).
//
// Why the grid loses nothing: two regular polygons whose swept boxes are disjoint have a computed sweep record with
// hit == 0, so they are in no query's pick.  No margin enters: the result is that of the N x M call for every input bit pattern.
//
// The pipeline, all on the caller's stream, through the ctx scratch of the pair searches:
//   1. boxes      broad_box_kernel with PolySweepBroadShape (c2d_sweep_shape.hpp) on both sets (once when they are the same memory AND
//                 the same motion planes): the swept boxes of §5.19; wild and absent polygons as there
//   2. - 5.       the frame of c2d_grid_best.hpp with the policy below (CastGrid): grid and sort, the counters of this call for
//                 c2d_poly_set_casts_grid_stats, the row kernel's cell walk, the list kernel
//   6. finalise   cast_launch_finalise (c2d_cast.hip, its kernel unchanged): the winner's record by the sweep kernel's routines, the
//                 miss and BAD_PAIR records.
// A row has one owner in every pass: there are no atomics on the records.
//
// The per-pair step (CastGrid::pair), for a candidate with global index gj against the lane's best key K (all ones: nothing yet), in
// ANY order of the candidates (the walk visits B in cell-key order, the tail and the list in index order):
//   a. (u64)gj > K: K is (+0, a smaller index); no key at gj is below it.  Nothing runs.
//   b. one axis walk (poly_axes into SweepPick, as PolySweepBroadShape::collide and the finalise pass run it) gives hit0 and the pick.
//      The pair's key is gj when hit0 (toi = +0), else (bits of t_in) << 32 | gj when !never && t_in <= t_out, else none.
//   c. K = min(K, key).
// The compare is on the whole key, never on the time alone: c2d_cast.hip may abandon a pair on t_in >= best only because it visits B
// in index order, where an equal time at a later index loses.  Here a later candidate may have the smaller index.  There is no early
// abandon inside the walk and no bound on the box level: K only falls and is always the key of a considered hit, so the minimum over
// the candidates is the minimum over all of B whatever the order.
#include "c2d_cast_parts.hpp"
#include "c2d_grid_best.hpp"
#include "c2d_sweep_shape.hpp"

namespace c2d {

// §5.19's swept-box policy under a name of this file's own: the box kernel below is this translation unit's instance, not a second
// definition of c2d_sweep_broad.hip's
struct CastGridShape : PolySweepBroadShape {};

// the query policy of the frame (c2d_grid_best.hpp)
struct CastGrid : PolySweepShape {   // Set (the polygons with their motion planes), Obj, size, load
    using Shape = CastGridShape;
    using Out = c2d_cast;
    struct Aux {};
    struct Params {};
    // the policy's counter behind the frame's walked and met: `walks`, of the candidates the pairs that ran the axis walk (the others
    // could not beat a best at time 0)
    enum { kWalks = 2, kCounters = 3 };
    static constexpr unsigned int kMagic = 0x43534731u;   // "CSG1": the header's counters are those of a grid cast
    static constexpr unsigned long long kNoKey = kSetNoKey;
    static C2D_DEV Aux aux(const Obj&) { return Aux{}; }

    // One candidate (the file's head, a to c): best = min(best, the pair's key) when the pair is a hit.
    static C2D_DEV void pair(const Obj& a, Aux, const Obj& b, Params, uint32_t gj, unsigned long long& best, GridBestCount<kCounters>& n)
    {
        n.n[kGridBestMet]++;
        if ((unsigned long long)gj > best) return;
        n.n[kWalks]++;
        SweepPick pick{b.dx - a.dx, b.dy - a.dy};
        const bool hit0 = PolySweepShape::axes(a, b, pick);
        unsigned long long key = kSetNoKey;
        if (hit0) {
            key = (unsigned long long)gj;   // starts in overlap: toi = +0
        } else if (!pick.never && pick.t_in <= pick.t_out) {
            key = ((unsigned long long)__float_as_uint(pick.t_in) << 32) | gj;   // (t_in starts at +0 and only grows: never NaN, never -0)
        }
        best = key < best ? key : best;
    }
};

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_set_casts_grid(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, const float* d_a_dx, const float* d_a_dy, const float* d_b_dx,
                            const float* d_b_dy, size_t row_base, size_t col_base, int flags, c2d_cast* d_out, c2d_stream stream)
{
    const char* what = "c2d_poly_set_casts_grid";
    if (int rc = sweep_motion_check(ctx, what, d_a_dx, d_a_dy, d_b_dx, d_b_dy)) return rc;   // (a missing ctx too)
    if (!a || !b || !d_out) return cross_fail(ctx, what, "NULL argument");
    if (a->n == 0) return C2D_OK;
    PolySweepBroadSet A, B;
    if (int rc = poly_set_check(ctx, what, "a", a, A.set.s)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B.set.s, kEmptySetOk)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) return cross_fail(ctx, what, "the output must be 8-byte aligned");
    if (flags & ~C2D_CAST_SKIP_SELF) return cross_fail(ctx, what, "unknown flag");
    if (int rc = cross_check_index_bases(ctx, what, A.set.s.n, B.set.s.n, row_base, col_base, "n_a, n_b, row_base + n_a and col_base + n_b must not exceed 2^32"))
        return rc;
    A.set.dx = d_a_dx;
    A.set.dy = d_a_dy;
    B.set.dx = d_b_dx;
    B.set.dy = d_b_dy;
    A.async_err = B.async_err = ctx->d_async_err;

    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (B.set.s.n == 0) {   // no grid, no scratch: the miss record, or BAD_PAIR, for every query
        if (int rc = set_best_launch_init<3>(ctx, s, A.set.s.n, d_out)) return rc;
        return cast_launch_finalise(ctx, s, A.set.s, B.set.s, d_a_dx, d_a_dy, d_b_dx, d_b_dy, col_base, d_out);
    }
    // one set against itself only when it moves as itself: the boxes are swept boxes
    const bool same = poly_sets_same(A.set.s, B.set.s) && d_a_dx == d_b_dx && d_a_dy == d_b_dy;
    WorkspaceUse use(ctx, s);
    if (int rc = grid_best_run<CastGrid>(ctx, s, what, A, B, same, row_base, col_base, flags & C2D_CAST_SKIP_SELF, CastGrid::Params{}, d_out, use)) return rc;
    if (int rc = cast_launch_finalise(ctx, s, A.set.s, B.set.s, d_a_dx, d_a_dy, d_b_dx, d_b_dy, col_base, d_out)) return rc;
    use.done();
    return C2D_OK;
}

/* The counters of the last c2d_poly_set_casts_grid call with n_b > 0 on this ctx (a blocking read of the scene header). */
int c2d_poly_set_casts_grid_stats(c2d_ctx* ctx, unsigned long long out[5])
{
    GridBestStats<CastGrid::kCounters> st;
    unsigned int n_long;
    if (int rc = grid_stats_read(ctx, "c2d_poly_set_casts_grid_stats", out, "no grid cast has run on this ctx",
                                 "the ctx scratch does not hold a grid cast (another call has used it since)", CastGrid::kMagic, st, n_long))
        return rc;
    out[0] = n_long;
    for (int q = 0; q < CastGrid::kCounters; q++) out[1 + q] = st.n[q];   // walked, met, walks
    out[4] = 0ull;   // reserved
    return C2D_OK;
}

}  // extern "C"
