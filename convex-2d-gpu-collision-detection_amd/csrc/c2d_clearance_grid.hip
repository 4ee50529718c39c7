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
//   2. grid, sort broad_grid_and_sort, unchanged: a box over more than two cells becomes wild
//   3. counters   clearance_grid_begin_kernel: the counters of this call, in the scene header's extent histogram (dead by now), for
//                 c2d_poly_set_clearances_grid_stats
//   4. rows       clearance_grid_row_kernel, one query per lane: the cell walk of broad_row_query (the same cell range, boxes_meet on
//                 the sorted boxes, then the wild tail) with a running best key instead of a count.  A wild query, and one whose walk
//                 would pass kCandidateCap sorted entries, goes to a list; an absent one keeps "nothing" (the last pass writes its
//                 BAD_PAIR record).  Every other query's key goes to the first eight bytes of its record.
//   5. list       clearance_grid_list_kernel, one listed query per wave over all of B in index order: the box filter where both are
//                 regular, the same per-pair step, a wave minimum of the key, one store.
//   6. finalise   clearance_launch_finalise (c2d_clearance.hip, its kernel unchanged): the winner's record by the distance kernel's
//                 routines, the NONE and BAD_PAIR records.
// A row has one owner in every pass: there are no atomics on the records.
//
// The per-pair step (clearance_grid_pair), for a candidate with global index gj against the lane's best key, in ANY order of the
// candidates (the walk visits B in key order, the tail and the list in index order):
//   a. gj > best (the whole key): the best is (+0, a smaller index); no key at gj is below it.  Nothing runs.
//   b. the pairwise test.  A hit has the key (+0, gj).
//   c. not hit: l = sqrtf(clearance_lb2(vertex boxes)).  l > max_dist: every usable candidate has dist > max_dist, the pair is not
//      considered.  (bits of l) << 32 | gj > best: the pair's key is above the best.  Either way the candidate walk is skipped.
//   d. the pick of c2d_distance_rule.hpp over both sides; considered when there is a usable candidate and sqrtf(best d2) <= max_dist.
// DESIGN.md §5.21 proves c: from d2 >= lb2 for every usable candidate (c2d_clearance_bound.hpp) and the monotone square root, the
// pair's dist is at least l, so its key is at least (l, gj); the running best only falls, so a pair whose least possible key is above
// it at any time is above the final minimum.  No order of visit enters.
#include <cstring>

#include "c2d_clearance_bound.hpp"
#include "c2d_clearance_parts.hpp"
#include "c2d_near_shape.hpp"

namespace c2d {

// §5.20's margin policy under a name of this file's own: the box kernel below is this translation unit's instance, not a second
// definition of c2d_near_broad.hip's
struct ClearanceGridShape : PolyNearShape {};

constexpr unsigned int kClearanceGridMagic = 0x43474731u;   // "CGG1": the header's counters are those of a grid clearance query

// The counters of one call live in the scene header's extent histogram, which is dead once the cell size has been picked (as
// c2d_ray_grid.hip's do).
struct ClearanceGridStats {
    unsigned long long walked;   // sorted entries the row kernel's walks looked at (the aborted walks of listed queries included)
    unsigned long long met;      // candidates: entries whose box meets the query's, the wild tail, and what the list kernel's filter let through
    unsigned long long tested;   // of those, the pairs that ran the pairwise test (the others could not beat a best at distance 0)
    unsigned long long walks;    // of those, the pairs that ran the candidate walk of the distance rule (the bound skipped the others)
    unsigned int magic;
    unsigned int pad_;
};
static_assert(sizeof(ClearanceGridStats) <= sizeof(unsigned int) * kHistBins && offsetof(BroadGrid, hist) == 0, "the counters sit at the start of the scene header");

C2D_DEV ClearanceGridStats* clearance_grid_stats(BroadGrid* g) { return reinterpret_cast<ClearanceGridStats*>(g->hist); }

struct ClearanceGridCount {
    uint32_t walked = 0, met = 0, tested = 0, walks = 0;   // per lane and launch: a lane sees far fewer than 2^32 pairs (n_b <= 2^32 in all)
};

// a wave's counts into the header: one atomic per counter and wave
C2D_DEV void clearance_grid_count(BroadGrid* g, const ClearanceGridCount& c)
{
    unsigned long long v[4] = {c.walked, c.met, c.tested, c.walks};
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        ClearanceGridStats* st = clearance_grid_stats(g);
        if (v[0]) atomicAdd(&st->walked, v[0]);
        if (v[1]) atomicAdd(&st->met, v[1]);
        if (v[2]) atomicAdd(&st->tested, v[2]);
        if (v[3]) atomicAdd(&st->walks, v[3]);
    }
}

__global__ void clearance_grid_begin_kernel(BroadGrid* __restrict__ g)
{
    if (threadIdx.x != 0) return;
    ClearanceGridStats* st = clearance_grid_stats(g);
    st->walked = st->met = st->tested = st->walks = 0ull;
    st->magic = kClearanceGridMagic;
    st->pad_ = 0u;
}

struct ClearanceGridQuery {
    PolySetDev A, B;
    const float4* box_a;        // [n_a] margin boxes (NaN: wild or absent)
    const float4* box_b;        // [n_b], index order
    const uint32_t* keys;       // [n_b] sorted keys: regular ones first, then kWildKey, then kAbsentKey
    const uint32_t* idx;        // [n_b] index of each sorted key
    const float4* sbox;         // [n_b] boxes in key order
    BroadGrid* g;
    uint32_t* listed;           // [n_a] the queries left to the list kernel (g->n_long of them)
    size_t row_base, col_base;
    float r;                    // max_dist (finite, 0 <= r < 2^60, never -0)
    int skip_self;
};

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

// One candidate (the file's head, a to d): best = min(best, the pair's key) when the pair is considered and can win.
C2D_DEV void clearance_grid_pair(const PolyObj& a, const ClearanceBox& abox, const PolyObj& b, float r, uint32_t gj, unsigned long long& best,
                                 ClearanceGridCount& n)
{
    n.met++;
    if ((unsigned long long)gj > best) return;
    n.tested++;
    unsigned long long key = (unsigned long long)gj;   // a hit: dist = +0
    if (!poly_collide(a, b)) {
        const float l = __builtin_sqrtf(clearance_lb2(abox, clearance_grid_box(b)));   // (lb2 is +0, positive or +inf: never NaN, never -0)
        if (l > r) return;
        if ((((unsigned long long)__float_as_uint(l) << 32) | gj) > best) return;
        n.walks++;
        PolyObj p = a, q = b;   // distance_side turns its edge polygon
        DistancePick pick;
        distance_side<C2D_POLY_KMAX>(p.x, p.y, p.k, q.x, q.y, q.k, 0u, pick);
        distance_side<C2D_POLY_KMAX>(q.x, q.y, q.k, p.x, p.y, p.k, kDistanceSide1, pick);
        if (pick.code == kDistanceNone) return;
        const float dist = __builtin_sqrtf(pick.best);   // (d2 is a sum of squares: never -0; a NaN d2 is never picked)
        if (!(dist <= r)) return;
        key = ((unsigned long long)__float_as_uint(dist) << 32) | gj;
    }
    best = key < best ? key : best;
}

// 4. one query per lane
__global__ __launch_bounds__(kBroadBlock) void clearance_grid_row_kernel(ClearanceGridQuery q, c2d_clearance* __restrict__ out)
{
    BroadGrid* g = q.g;
    const size_t n_a = q.A.n, n_b = q.B.n;
    const uint32_t n_reg = g->n_reg_b;
    const uint32_t gx = g->gx, gy = g->gy;
    ClearanceGridCount count;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < n_a; i += (size_t)gridDim.x * kBroadBlock) {
        const float4 ba = q.box_a[i];
        unsigned long long best = kClrNoKey;
        bool listed = box_wild(ba) && !box_absent(ba);
        if (!box_wild(ba)) {
            PolyObj a;
            poly_load(q.A, i, a);
            const ClearanceBox abox = clearance_grid_box(a);
            const size_t gi = q.row_base + i;
            // broad_row_query's cell range: B_j overlaps ba only if cx(min x_j) is in [cx(min x_i) - 1, cx(max x_i)]
            uint32_t cx0 = cell_of(ba.x, g->x0, g->ix, gx), cx1 = cell_of(ba.z, g->x0, g->ix, gx);
            uint32_t cy0 = cell_of(ba.y, g->y0, g->iy, gy), cy1 = cell_of(ba.w, g->y0, g->iy, gy);
            cx0 = cx0 ? cx0 - 1u : 0u;
            cy0 = cy0 ? cy0 - 1u : 0u;
            uint32_t walked = 0;
#pragma unroll 1
            for (uint32_t cy = cy0; cy <= cy1 && !listed; cy++) {
                const uint32_t k_lo = cy * gx + cx0, k_hi = cy * gx + cx1;
#pragma unroll 1
                for (uint32_t k = lower_bound_u32(q.keys, n_reg, k_lo); k < n_reg && q.keys[k] <= k_hi; k++) {
                    if (++walked > kCandidateCap) {
                        listed = true;
                        break;
                    }
                    if (!boxes_meet(ba, q.sbox[k])) continue;
                    const uint32_t j = q.idx[k];
                    if ((size_t)j >= n_b) continue;   // (never: a sorted entry is a polygon of B)
                    if (q.skip_self && gi == q.col_base + j) continue;
                    PolyObj b;
                    poly_load(q.B, j, b);
                    clearance_grid_pair(a, abox, b, q.r, (uint32_t)(q.col_base + j), best, count);
                }
            }
            count.walked += walked < kCandidateCap ? walked : kCandidateCap;
            if (!listed) {
#pragma unroll 1
                for (size_t k = n_reg; k < n_b && q.keys[k] != kAbsentKey; k++) {   // the wild tail ends where the absent polygons begin
                    const uint32_t j = q.idx[k];
                    if ((size_t)j >= n_b) continue;
                    if (q.skip_self && gi == q.col_base + j) continue;
                    PolyObj b;
                    poly_load(q.B, j, b);
                    clearance_grid_pair(a, abox, b, q.r, (uint32_t)(q.col_base + j), best, count);
                }
            }
        }
        if (listed) {
            const unsigned int slot = atomicAdd(&g->n_long, 1u);   // each query at most once: slot < n_a
            if ((size_t)slot < n_a) q.listed[slot] = (uint32_t)i;
        } else {
            reinterpret_cast<unsigned long long*>(out)[4 * i] = best;   // (an absent query: "nothing"; the last pass knows it is bad)
        }
    }
    clearance_grid_count(g, count);   // (every lane of the block arrives: the loop above has no early return)
}

// 5. the listed queries: one per wave over all of B's columns
__global__ __launch_bounds__(kBroadBlock) void clearance_grid_list_kernel(ClearanceGridQuery q, c2d_clearance* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_long = q.g->n_long;
    const size_t n_a = q.A.n, n_b = q.B.n;
    const size_t waves = (size_t)gridDim.x * (kBroadBlock / 64);
    ClearanceGridCount count;
    for (size_t w = (size_t)blockIdx.x * (kBroadBlock / 64) + (threadIdx.x >> 6); w < n_long && w < n_a; w += waves) {
        const size_t i = q.listed[w];
        if (i >= n_a) continue;
        const float4 ba = q.box_a[i];
        PolyObj a;
        poly_load(q.A, i, a);
        const ClearanceBox abox = clearance_grid_box(a);
        const size_t gi = q.row_base + i;
        unsigned long long best = kClrNoKey;
#pragma unroll 1
        for (size_t j = lane; j < n_b; j += 64) {
            const float4 bb = q.box_b[j];
            if (box_absent(bb)) continue;
            if (!box_wild(ba) && !box_wild(bb) && !boxes_meet(ba, bb)) continue;
            if (q.skip_self && gi == q.col_base + j) continue;
            PolyObj b;
            poly_load(q.B, j, b);
            clearance_grid_pair(a, abox, b, q.r, (uint32_t)(q.col_base + j), best, count);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(best, off, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) reinterpret_cast<unsigned long long*>(out)[4 * i] = best;
    }
    clearance_grid_count(q.g, count);
}

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
    B.set = PolySetDev{nullptr, nullptr, nullptr, 0, 0, (int)b->rows};
    if (int rc = poly_set_check(ctx, what, "a", a, A.set)) return rc;
    if (b->n == 0) {   // (no plane is read: only `rows` is looked at)
        if (b->rows < 1 || b->rows > (uint32_t)C2D_POLY_KMAX) return cross_fail(ctx, what, "set b: rows must be 1..C2D_POLY_KMAX");
    } else if (int rc = poly_set_check(ctx, what, "b", b, B.set)) {
        return rc;
    }
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return cross_fail(ctx, what, "the output must be 16-byte aligned");
    if (flags & ~C2D_CLEARANCE_SKIP_SELF) return cross_fail(ctx, what, "unknown flag");
    const size_t n_a = A.set.n, n_b = B.set.n;
    if (n_a > kBroadIndexLimit || row_base > kBroadIndexLimit - n_a || n_b > kBroadIndexLimit || col_base > kBroadIndexLimit - n_b)
        return cross_fail(ctx, what, "n_a, n_b, row_base + n_a and col_base + n_b must not exceed 2^32");
    A.r = B.r = max_dist + 0.0f;   // -0 counts as 0
    A.async_err = B.async_err = ctx->d_async_err;

    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_b == 0) {   // no grid, no scratch: the NONE record, or BAD_PAIR, for every query
        if (int rc = clearance_launch_init(ctx, s, n_a, d_out)) return rc;
        return clearance_launch_finalise(ctx, s, A.set, B.set, col_base, d_out);
    }
    const bool same = A.set.vx == B.set.vx && A.set.vy == B.set.vy && A.set.k == B.set.k && n_a == n_b && A.set.stride == B.set.stride &&
                      A.set.rows == B.set.rows;
    BroadScratch W;
    if (int rc = broad_scratch(ctx, s, what, n_a, n_b, same, W)) return rc;
    WorkspaceUse use(ctx, s);   // the kernels work through the scratch: stamp behind the last one
    use.arm();
    if (int rc = broad_begin(ctx, s, W)) return rc;
    const int grid_a = grid_for(n_a, kBroadBlock, 8192), grid_b = grid_for(n_b, kBroadBlock, 8192);
    hipLaunchKernelGGL(broad_box_kernel<ClearanceGridShape>, dim3(grid_a), dim3(kBroadBlock), 0, s, A, n_a, W.box_a, W.g);
    C2D_LAUNCH_CHECK(ctx);
    if (!same) {
        hipLaunchKernelGGL(broad_box_kernel<ClearanceGridShape>, dim3(grid_b), dim3(kBroadBlock), 0, s, B, n_b, W.box_b, W.g);
        C2D_LAUNCH_CHECK(ctx);
    }
    if (int rc = broad_grid_and_sort(ctx, s, W, n_a, n_b, same)) return rc;

    hipLaunchKernelGGL(clearance_grid_begin_kernel, dim3(1), dim3(64), 0, s, W.g);
    C2D_LAUNCH_CHECK(ctx);
    const ClearanceGridQuery q{A.set, B.set, W.box_a, W.box_b, W.keys, W.idx, W.sbox, W.g, W.long_rows, row_base, col_base, A.r,
                               (flags & C2D_CLEARANCE_SKIP_SELF) ? 1 : 0};
    hipLaunchKernelGGL(clearance_grid_row_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, q, d_out);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(clearance_grid_list_kernel, dim3(kLongGrid), dim3(kBroadBlock), 0, s, q, d_out);
    C2D_LAUNCH_CHECK(ctx);
    if (int rc = clearance_launch_finalise(ctx, s, A.set, B.set, col_base, d_out)) return rc;
    use.done();
    return C2D_OK;
}

/* The counters of the last c2d_poly_set_clearances_grid call with n_b > 0 on this ctx (a blocking read of the scene header). */
int c2d_poly_set_clearances_grid_stats(c2d_ctx* ctx, unsigned long long out[5])
{
    const char* what = "c2d_poly_set_clearances_grid_stats";
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!out) return cross_fail(ctx, what, "NULL argument");
    if (!ctx->d_scratch || ctx->scratch_bytes < sizeof(BroadGrid)) return cross_fail(ctx, what, "no grid clearance query has run on this ctx");
    DeviceGuard dg(ctx->device);
    static_assert(sizeof(BroadGrid) % 8 == 0, "copied as 64-bit words");
    unsigned long long raw[sizeof(BroadGrid) / 8];
    C2D_HIP(ctx, hipMemcpy(raw, ctx->d_scratch, sizeof(BroadGrid), hipMemcpyDeviceToHost));
    BroadGrid h;
    std::memcpy(&h, raw, sizeof h);
    ClearanceGridStats st;
    std::memcpy(&st, h.hist, sizeof st);
    if (st.magic != kClearanceGridMagic) return cross_fail(ctx, what, "the ctx scratch does not hold a grid clearance query (another call has used it since)");
    out[0] = h.n_long;
    out[1] = st.walked;
    out[2] = st.met;
    out[3] = st.tested;
    out[4] = st.walks;
    return C2D_OK;
}

}  // extern "C"
