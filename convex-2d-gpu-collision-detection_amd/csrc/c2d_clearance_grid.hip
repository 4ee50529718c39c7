// c2d_clearance_grid.hip — grid clearance queries for gfx950 (MI355X): c2d_poly_set_clearances_grid (include/c2d.h "clearance queries
// through a grid").  For every polygon A_i of a set the polygon of a set B nearest to it among those that are hit or
// no farther than max_dist, with the pair's whole distance record: the reduction of c2d_clearance.hip over the pairs that
// c2d_poly_near_broad_pairs lists, found through the grid of the pair searches instead of a visit to every polygon.
//
// The rule.  D(i, j) is the c2d_distance record of (A_i, B_j).  Polygon j is considered when its vertex count is within 1..rows, it is
// not the self pair (C2D_CLEARANCE_SKIP_SELF: row_base + i == col_base + j) and D(i, j).hit == 1 || D(i, j).dist <= max_dist.  The
// winner is the considered j with the smallest key (bits of D(i, j).dist) << 32 | (col_base + j).
//
// The pipeline, all on the caller's stream, through the ctx scratch of the pair searches:
//   1. boxes      broad_box_kernel with PolyNearShape (c2d_near_shape.hpp) on both sets (once when they are the same memory): the margin boxes of §5.20, each
//                 holding half of max_dist; wild and absent polygons as there
//   2. - 5.       the frame of c2d_grid_best.hpp with the policy below (ClearanceGrid): grid and sort, the counters of this call for
//                 c2d_poly_set_clearances_grid_stats, the row kernel's cell walk, the list kernel
//   6. finalise   clearance_launch_finalise (c2d_clearance.hip, its kernel unchanged): the winner's record by the distance kernel's
//                 routines, the NONE and BAD_PAIR records.
// A row has one owner in every pass: there are no atomics on the records.
//
// The per-pair step (ClearanceGrid::pair), for a candidate with global index gj against the lane's best key, in ANY order of the
// candidates (the walk visits B in key order, the tail and the list in index order):
//   a. gj > best (the whole key): the best is (+0, a smaller index); no key at gj is below it.  Nothing runs.
//   b. the pairwise test.  A hit has the key (+0, gj).
//   c. not hit: l = sqrtf(clearance_lb2(vertex boxes)).  l > max_dist: every usable candidate has dist > max_dist, the pair is not
//      considered.  (bits of l) << 32 | gj > best: the pair's key is above the best.  Either way the candidate walk is skipped.
//   d. the pick of c2d_distance_rule.hpp over both sides; considered when there is a usable candidate and sqrtf(best d2) <= max_dist.
// DESIGN.md §5.21 proves c: from d2 >= lb2 for every usable candidate (c2d_clearance_bound.hpp) and the monotone square root, the
// pair's dist is at least l, so its key is at least (l, gj); the running best only falls, so a pair whose least possible key is above
// it at any time is above the final minimum.  No order of visit enters.
#include "c2d_clearance_bound.hpp"
#include "c2d_clearance_parts.hpp"
#include "c2d_grid_best.hpp"
#include "c2d_near_shape.hpp"

namespace c2d {

// §5.20's margin policy under a name of this file's own: the box kernel below is this translation unit's instance, not a second
// definition of c2d_near_broad.hip's
struct ClearanceGridShape : PolyNearShape {};

// the vertex box of a loaded polygon and its largest |coordinate| (padding repeats vertex 0: all 16 slots hold live values); a NaN or
// an infinite coordinate gives c = +inf, which clearance_lb2 never skips
C2D_DEV ClearanceBox clearance_grid_box(const PolyObj& p)
{
    const float inf = __builtin_inff();
    ClearanceBox b{p.x[0], p.x[0], p.y[0], p.y[0], 0.0f};
    float c = 0.0f;
    bool finite = true;
#pragma unroll
    for (int v = 0; v < C2D_POLY_KMAX; v++) {
        b.xlo = __builtin_fminf(b.xlo, p.x[v]);
        b.xhi = __builtin_fmaxf(b.xhi, p.x[v]);
        b.ylo = __builtin_fminf(b.ylo, p.y[v]);
        b.yhi = __builtin_fmaxf(b.yhi, p.y[v]);
        c = __builtin_fmaxf(c, __builtin_fmaxf(__builtin_fabsf(p.x[v]), __builtin_fabsf(p.y[v])));
        finite &= (__builtin_fabsf(p.x[v]) < inf) & (__builtin_fabsf(p.y[v]) < inf);
    }
    b.c = finite ? c : inf;
    return b;
}

// the query policy of the frame (c2d_grid_best.hpp)
struct ClearanceGrid {
    using Shape = ClearanceGridShape;
    using Set = PolySetDev;
    using Obj = PolyObj;
    using Aux = ClearanceBox;
    using Out = c2d_clearance;
    struct Params {
        float r;   // max_dist (finite, 0 <= r < 2^60, never -0)
    };
    // the policy's counters behind the frame's walked and met: `tested`, of the candidates the pairs that ran the pairwise test (the
    // others could not beat a best at distance 0); `walks`, of those the pairs that ran the candidate walk of the distance rule (the
    // bound skipped the others)
    enum { kTested = 2, kWalks = 3, kCounters = 4 };
    static constexpr unsigned int kMagic = 0x43474731u;   // "CGG1": the header's counters are those of a grid clearance query
    static constexpr unsigned long long kNoKey = kSetNoKey;
    static __host__ __device__ size_t size(const Set& X) { return X.n; }
    static constexpr auto& load = poly_load;   // (the function itself: a wrapper renames the kernels' registers)
    static C2D_DEV Aux aux(const Obj& a) { return clearance_grid_box(a); }

    // One candidate (the file's head, a to d): best = min(best, the pair's key) when the pair is considered and can win.
    static C2D_DEV void pair(const Obj& a, const Aux& abox, const Obj& b, Params par, uint32_t gj, unsigned long long& best,
                             GridBestCount<kCounters>& n)
    {
        n.n[kGridBestMet]++;
        if ((unsigned long long)gj > best) return;
        n.n[kTested]++;
        unsigned long long key = (unsigned long long)gj;   // a hit: dist = +0
        if (!poly_collide(a, b)) {
            const float l = __builtin_sqrtf(clearance_lb2(abox, clearance_grid_box(b)));   // (lb2 is +0, positive or +inf: never NaN, never -0)
            if (l > par.r) return;
            if ((((unsigned long long)__float_as_uint(l) << 32) | gj) > best) return;
            n.n[kWalks]++;
            PolyObj p = a, q = b;   // distance_side turns its edge polygon
            DistancePick pick;
            distance_side<C2D_POLY_KMAX>(p.x, p.y, p.k, q.x, q.y, q.k, 0u, pick);
            distance_side<C2D_POLY_KMAX>(q.x, q.y, q.k, p.x, p.y, p.k, kDistanceSide1, pick);
            if (pick.code == kDistanceNone) return;
            const float dist = __builtin_sqrtf(pick.best);   // (d2 is a sum of squares: never -0; a NaN d2 is never picked)
            if (!(dist <= par.r)) return;
            key = ((unsigned long long)__float_as_uint(dist) << 32) | gj;
        }
        best = key < best ? key : best;
    }
};

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_set_clearances_grid(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, float max_dist, size_t row_base, size_t col_base, int flags,
                                 c2d_clearance* d_out, c2d_stream stream)
{
    const char* what = "c2d_poly_set_clearances_grid";
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!(max_dist >= 0.0f && max_dist < kNearMaxDist)) return fail_arg(ctx, "c2d_poly_set_clearances_grid: max_dist must be finite with 0 <= max_dist < 2^60");
    if (!a || !b || !d_out) return cross_fail(ctx, what, "NULL argument");
    if (a->n == 0) return C2D_OK;
    PolyNearSet A, B;
    if (int rc = poly_set_check(ctx, what, "a", a, A.set)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B.set, kEmptySetOk)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return cross_fail(ctx, what, "the output must be 16-byte aligned");
    if (flags & ~C2D_CLEARANCE_SKIP_SELF) return cross_fail(ctx, what, "unknown flag");
    if (int rc = cross_check_index_bases(ctx, what, A.set.n, B.set.n, row_base, col_base, "n_a, n_b, row_base + n_a and col_base + n_b must not exceed 2^32"))
        return rc;
    A.r = B.r = max_dist + 0.0f;   // -0 counts as 0
    A.async_err = B.async_err = ctx->d_async_err;

    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (B.set.n == 0) {   // no grid, no scratch: the NONE record, or BAD_PAIR, for every query
        if (int rc = set_best_launch_init<4>(ctx, s, A.set.n, d_out)) return rc;
        return clearance_launch_finalise(ctx, s, A.set, B.set, col_base, d_out);
    }
    WorkspaceUse use(ctx, s);
    if (int rc = grid_best_run<ClearanceGrid>(ctx, s, what, A, B, poly_sets_same(A.set, B.set), row_base, col_base, flags & C2D_CLEARANCE_SKIP_SELF,
                                              ClearanceGrid::Params{A.r}, d_out, use))
        return rc;
    if (int rc = clearance_launch_finalise(ctx, s, A.set, B.set, col_base, d_out)) return rc;
    use.done();
    return C2D_OK;
}

/* The counters of the last c2d_poly_set_clearances_grid call with n_b > 0 on this ctx (a blocking read of the scene header). */
int c2d_poly_set_clearances_grid_stats(c2d_ctx* ctx, unsigned long long out[5])
{
    GridBestStats<ClearanceGrid::kCounters> st;
    unsigned int n_long;
    if (int rc = grid_stats_read(ctx, "c2d_poly_set_clearances_grid_stats", out, "no grid clearance query has run on this ctx",
                                 "the ctx scratch does not hold a grid clearance query (another call has used it since)", ClearanceGrid::kMagic, st, n_long))
        return rc;
    out[0] = n_long;
    for (int q = 0; q < ClearanceGrid::kCounters; q++) out[1 + q] = st.n[q];   // walked, met, tested, walks
    return C2D_OK;
}

}  // extern "C"
