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
//   2. grid, sort broad_grid_and_sort, unchanged: a box over more than two cells becomes wild
//   3. counters   cast_grid_begin_kernel: the counters of this call, in the scene header's extent histogram (dead by now), for
//                 c2d_poly_set_casts_grid_stats
//   4. rows       cast_grid_row_kernel, one query per lane: the cell walk of broad_row_query (the same cell range, boxes_meet on the
//                 sorted boxes, then the wild tail) with a running best key instead of a count.  A wild query, and one whose walk
//                 would pass kCandidateCap sorted entries, goes to a list; an absent one keeps "nothing" (the last pass writes its
//                 BAD_PAIR record).  Every other query's key goes to the first eight bytes of its record.
//   5. list       cast_grid_list_kernel, one listed query per wave over all of B in index order: the box filter where both are
//                 regular, the same per-pair step, a wave minimum of the key, one store.
//   6. finalise   cast_launch_finalise (c2d_cast.hip, its kernel unchanged): the winner's record by the sweep kernel's routines, the
//                 miss and BAD_PAIR records.
// A row has one owner in every pass: there are no atomics on the records.
//
// The per-pair step (cast_grid_pair), for a candidate with global index gj against the lane's best key K (all ones: nothing yet), in
// ANY order of the candidates (the walk visits B in cell-key order, the tail and the list in index order):
//   a. (u64)gj > K: K is (+0, a smaller index); no key at gj is below it.  Nothing runs.
//   b. one axis walk (poly_axes into SweepPick, as PolySweepBroadShape::collide and the finalise pass run it) gives hit0 and the pick.
//      The pair's key is gj when hit0 (toi = +0), else (bits of t_in) << 32 | gj when !never && t_in <= t_out, else none.
//   c. K = min(K, key).
// The compare is on the whole key, never on the time alone: c2d_cast.hip may abandon a pair on t_in >= best only because it visits B
// in index order, where an equal time at a later index loses.  Here a later candidate may have the smaller index.  There is no early
// abandon inside the walk and no bound on the box level: K only falls and is always the key of a considered hit, so the minimum over
// the candidates is the minimum over all of B whatever the order.
#include <cstring>

#include "c2d_cast_parts.hpp"
#include "c2d_sweep_shape.hpp"

namespace c2d {

// §5.19's swept-box policy under a name of this file's own: the box kernel below is this translation unit's instance, not a second
// definition of c2d_sweep_broad.hip's
struct CastGridShape : PolySweepBroadShape {};

constexpr unsigned int kCastGridMagic = 0x43534731u;   // "CSG1": the header's counters are those of a grid cast

// The counters of one call live in the scene header's extent histogram, which is dead once the cell size has been picked (as
// c2d_clearance_grid.hip's do).
struct CastGridStats {
    unsigned long long walked;   // sorted entries the row kernel's walks looked at (the aborted walks of listed queries included)
    unsigned long long met;      // candidates: entries whose box meets the query's, the wild tail, and what the list kernel's filter let through
    unsigned long long walks;    // of those, the pairs that ran the axis walk (the others could not beat a best at time 0)
    unsigned int magic;
    unsigned int pad_;
};
static_assert(sizeof(CastGridStats) <= sizeof(unsigned int) * kHistBins && offsetof(BroadGrid, hist) == 0, "the counters sit at the start of the scene header");

C2D_DEV CastGridStats* cast_grid_stats(BroadGrid* g) { return reinterpret_cast<CastGridStats*>(g->hist); }

struct CastGridCount {
    uint32_t walked = 0, met = 0, walks = 0;   // per lane and launch: a lane sees far fewer than 2^32 pairs (n_b <= 2^32 in all)
};

// a wave's counts into the header: one atomic per counter and wave
C2D_DEV void cast_grid_count(BroadGrid* g, const CastGridCount& c)
{
    unsigned long long v[3] = {c.walked, c.met, c.walks};
#pragma unroll
    for (int q = 0; q < 3; q++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        CastGridStats* st = cast_grid_stats(g);
        if (v[0]) atomicAdd(&st->walked, v[0]);
        if (v[1]) atomicAdd(&st->met, v[1]);
        if (v[2]) atomicAdd(&st->walks, v[2]);
    }
}

__global__ void cast_grid_begin_kernel(BroadGrid* __restrict__ g)
{
    if (threadIdx.x != 0) return;
    CastGridStats* st = cast_grid_stats(g);
    st->walked = st->met = st->walks = 0ull;
    st->magic = kCastGridMagic;
    st->pad_ = 0u;
}

struct CastGridQuery {
    PolySweepShape::Set A, B;   // the polygons with their motion planes
    const float4* box_a;        // [n_a] swept boxes (NaN: wild or absent)
    const float4* box_b;        // [n_b], index order
    const uint32_t* keys;       // [n_b] sorted keys: regular ones first, then kWildKey, then kAbsentKey
    const uint32_t* idx;        // [n_b] index of each sorted key
    const float4* sbox;         // [n_b] boxes in key order
    BroadGrid* g;
    uint32_t* listed;           // [n_a] the queries left to the list kernel (g->n_long of them)
    size_t row_base, col_base;
    int skip_self;
};

// One candidate (the file's head, a to c): best = min(best, the pair's key) when the pair is a hit.
C2D_DEV void cast_grid_pair(const PolySweepShape::Obj& a, const PolySweepShape::Obj& b, uint32_t gj, unsigned long long& best, CastGridCount& n)
{
    n.met++;
    if ((unsigned long long)gj > best) return;
    n.walks++;
    SweepPick pick{b.dx - a.dx, b.dy - a.dy};
    const bool hit0 = PolySweepShape::axes(a, b, pick);
    unsigned long long key = kCastNoKey;
    if (hit0) {
        key = (unsigned long long)gj;   // starts in overlap: toi = +0
    } else if (!pick.never && pick.t_in <= pick.t_out) {
        key = ((unsigned long long)__float_as_uint(pick.t_in) << 32) | gj;   // (t_in starts at +0 and only grows: never NaN, never -0)
    }
    best = key < best ? key : best;
}

// 4. one query per lane
__global__ __launch_bounds__(kBroadBlock) void cast_grid_row_kernel(CastGridQuery q, c2d_cast* __restrict__ out)
{
    BroadGrid* g = q.g;
    const size_t n_a = q.A.s.n, n_b = q.B.s.n;
    const uint32_t n_reg = g->n_reg_b;
    const uint32_t gx = g->gx, gy = g->gy;
    CastGridCount count;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < n_a; i += (size_t)gridDim.x * kBroadBlock) {
        const float4 ba = q.box_a[i];
        unsigned long long best = kCastNoKey;
        bool listed = box_wild(ba) && !box_absent(ba);
        if (!box_wild(ba)) {
            PolySweepShape::Obj a;
            PolySweepShape::load(q.A, i, a);
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
                    PolySweepShape::Obj b;
                    PolySweepShape::load(q.B, j, b);
                    cast_grid_pair(a, b, (uint32_t)(q.col_base + j), best, count);
                }
            }
            count.walked += walked < kCandidateCap ? walked : kCandidateCap;
            if (!listed) {
#pragma unroll 1
                for (size_t k = n_reg; k < n_b && q.keys[k] != kAbsentKey; k++) {   // the wild tail ends where the absent polygons begin
                    const uint32_t j = q.idx[k];
                    if ((size_t)j >= n_b) continue;
                    if (q.skip_self && gi == q.col_base + j) continue;
                    PolySweepShape::Obj b;
                    PolySweepShape::load(q.B, j, b);
                    cast_grid_pair(a, b, (uint32_t)(q.col_base + j), best, count);
                }
            }
        }
        if (listed) {
            const unsigned int slot = atomicAdd(&g->n_long, 1u);   // each query at most once: slot < n_a
            if ((size_t)slot < n_a) q.listed[slot] = (uint32_t)i;
        } else {
            reinterpret_cast<unsigned long long*>(out)[3 * i] = best;   // (an absent query: "nothing"; the last pass knows it is bad)
        }
    }
    cast_grid_count(g, count);   // (every lane of the block arrives: the loop above has no early return)
}

// 5. the listed queries: one per wave over all of B's columns
__global__ __launch_bounds__(kBroadBlock) void cast_grid_list_kernel(CastGridQuery q, c2d_cast* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_long = q.g->n_long;
    const size_t n_a = q.A.s.n, n_b = q.B.s.n;
    const size_t waves = (size_t)gridDim.x * (kBroadBlock / 64);
    CastGridCount count;
    for (size_t w = (size_t)blockIdx.x * (kBroadBlock / 64) + (threadIdx.x >> 6); w < n_long && w < n_a; w += waves) {
        const size_t i = q.listed[w];
        if (i >= n_a) continue;
        const float4 ba = q.box_a[i];
        PolySweepShape::Obj a;
        PolySweepShape::load(q.A, i, a);
        const size_t gi = q.row_base + i;
        unsigned long long best = kCastNoKey;
#pragma unroll 1
        for (size_t j = lane; j < n_b; j += 64) {
            const float4 bb = q.box_b[j];
            if (box_absent(bb)) continue;
            if (!box_wild(ba) && !box_wild(bb) && !boxes_meet(ba, bb)) continue;
            if (q.skip_self && gi == q.col_base + j) continue;
            PolySweepShape::Obj b;
            PolySweepShape::load(q.B, j, b);
            cast_grid_pair(a, b, (uint32_t)(q.col_base + j), best, count);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(best, off, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) reinterpret_cast<unsigned long long*>(out)[3 * i] = best;
    }
    cast_grid_count(q.g, count);
}

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
    B.set.s = PolySetDev{nullptr, nullptr, nullptr, 0, 0, (int)b->rows};
    if (int rc = poly_set_check(ctx, what, "a", a, A.set.s)) return rc;
    if (b->n == 0) {   // (no plane is read: only `rows` is looked at)
        if (b->rows < 1 || b->rows > (uint32_t)C2D_POLY_KMAX) return cross_fail(ctx, what, "set b: rows must be 1..C2D_POLY_KMAX");
    } else if (int rc = poly_set_check(ctx, what, "b", b, B.set.s)) {
        return rc;
    }
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) return cross_fail(ctx, what, "the output must be 8-byte aligned");
    if (flags & ~C2D_CAST_SKIP_SELF) return cross_fail(ctx, what, "unknown flag");
    const size_t n_a = A.set.s.n, n_b = B.set.s.n;
    if (n_a > kBroadIndexLimit || row_base > kBroadIndexLimit - n_a || n_b > kBroadIndexLimit || col_base > kBroadIndexLimit - n_b)
        return cross_fail(ctx, what, "n_a, n_b, row_base + n_a and col_base + n_b must not exceed 2^32");
    A.set.dx = d_a_dx;
    A.set.dy = d_a_dy;
    B.set.dx = d_b_dx;
    B.set.dy = d_b_dy;
    A.async_err = B.async_err = ctx->d_async_err;

    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (n_b == 0) {   // no grid, no scratch: the miss record, or BAD_PAIR, for every query
        if (int rc = cast_launch_init(ctx, s, n_a, d_out)) return rc;
        return cast_launch_finalise(ctx, s, A.set.s, B.set.s, d_a_dx, d_a_dy, d_b_dx, d_b_dy, col_base, d_out);
    }
    // one set against itself only when it moves as itself: the boxes are swept boxes
    const bool same = A.set.s.vx == B.set.s.vx && A.set.s.vy == B.set.s.vy && A.set.s.k == B.set.s.k && n_a == n_b && A.set.s.stride == B.set.s.stride &&
                      A.set.s.rows == B.set.s.rows && d_a_dx == d_b_dx && d_a_dy == d_b_dy;
    BroadScratch W;
    if (int rc = broad_scratch(ctx, s, what, n_a, n_b, same, W)) return rc;
    WorkspaceUse use(ctx, s);   // the kernels work through the scratch: stamp behind the last one
    use.arm();
    if (int rc = broad_begin(ctx, s, W)) return rc;
    const int grid_a = grid_for(n_a, kBroadBlock, 8192), grid_b = grid_for(n_b, kBroadBlock, 8192);
    hipLaunchKernelGGL(broad_box_kernel<CastGridShape>, dim3(grid_a), dim3(kBroadBlock), 0, s, A, n_a, W.box_a, W.g);
    C2D_LAUNCH_CHECK(ctx);
    if (!same) {
        hipLaunchKernelGGL(broad_box_kernel<CastGridShape>, dim3(grid_b), dim3(kBroadBlock), 0, s, B, n_b, W.box_b, W.g);
        C2D_LAUNCH_CHECK(ctx);
    }
    if (int rc = broad_grid_and_sort(ctx, s, W, n_a, n_b, same)) return rc;

    hipLaunchKernelGGL(cast_grid_begin_kernel, dim3(1), dim3(64), 0, s, W.g);
    C2D_LAUNCH_CHECK(ctx);
    const CastGridQuery q{A.set, B.set, W.box_a, W.box_b, W.keys, W.idx, W.sbox, W.g, W.long_rows, row_base, col_base, (flags & C2D_CAST_SKIP_SELF) ? 1 : 0};
    hipLaunchKernelGGL(cast_grid_row_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, q, d_out);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(cast_grid_list_kernel, dim3(kLongGrid), dim3(kBroadBlock), 0, s, q, d_out);
    C2D_LAUNCH_CHECK(ctx);
    if (int rc = cast_launch_finalise(ctx, s, A.set.s, B.set.s, d_a_dx, d_a_dy, d_b_dx, d_b_dy, col_base, d_out)) return rc;
    use.done();
    return C2D_OK;
}

/* The counters of the last c2d_poly_set_casts_grid call with n_b > 0 on this ctx (a blocking read of the scene header). */
int c2d_poly_set_casts_grid_stats(c2d_ctx* ctx, unsigned long long out[5])
{
    const char* what = "c2d_poly_set_casts_grid_stats";
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!out) return cross_fail(ctx, what, "NULL argument");
    if (!ctx->d_scratch || ctx->scratch_bytes < sizeof(BroadGrid)) return cross_fail(ctx, what, "no grid cast has run on this ctx");
    DeviceGuard dg(ctx->device);
    static_assert(sizeof(BroadGrid) % 8 == 0, "copied as 64-bit words");
    unsigned long long raw[sizeof(BroadGrid) / 8];
    C2D_HIP(ctx, hipMemcpy(raw, ctx->d_scratch, sizeof(BroadGrid), hipMemcpyDeviceToHost));
    BroadGrid h;
    std::memcpy(&h, raw, sizeof h);
    CastGridStats st;
    std::memcpy(&st, h.hist, sizeof st);
    if (st.magic != kCastGridMagic) return cross_fail(ctx, what, "the ctx scratch does not hold a grid cast (another call has used it since)");
    out[0] = h.n_long;
    out[1] = st.walked;
    out[2] = st.met;
    out[3] = st.walks;
    out[4] = 0ull;   // reserved
    return C2D_OK;
}

}  // extern "C"
