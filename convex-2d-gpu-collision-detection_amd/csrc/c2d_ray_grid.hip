// c2d_ray_grid.hip — grid-accelerated ray queries for gfx950 (MI355X): c2d_poly_ray_casts_grid (include/c2d.h "ray queries through a
// grid").  Per ray the pick of c2d_poly_ray_casts restricted to the polygons whose float vertex box the ray MEETS
// (ray_meets, c2d_ray_walk.hpp) and the polygons without a box; found by walking the broad phase's uniform grid (c2d_broad.hpp) along
// the segment instead of visiting every polygon.
//
// The pipeline, all on the caller's stream, through the ctx scratch of the pair searches:
//   1. boxes      broad_box_kernel with the policy below: the float min / max of the live vertices; a NaN or an infinite coordinate
//                 makes the polygon wild; a bad count makes it absent (reported through the asynchronous error word)
//   2. grid, sort broad_grid_and_sort over B alone (the grid's bounds are B's)
//   3. init       set_best_launch_init: every record's key = "nothing yet"; ray_grid_begin_kernel: the counters of this call
//   4. outliers   ray_outlier_kernel: the regular boxes at or above the cell-size pick (at most max(4, n / 65536)) are the ones that may
//                 lie outside the grid's bounds, where the walk's proof does not reach: they are listed and tested against every ray
//   5. walk       ray_walk_kernel, the hot path: one ray per lane.  Per key row of the walk (c2d_ray_walk.hpp) a binary search on the
//                 sorted keys, then every sorted box of the row's key range through ray_meets, the survivors through the contract's
//                 per-polygon rule on vertices gathered from B's planes; then the outliers and the wild tail.  The running best
//                 is the (t, j) key.  A non-finite ray, a ray with C >= 2^60 and a ray whose walk would visit more than
//                 kRayWalkCap sorted entries go to a list instead.
//   6. list       ray_list_kernel: one listed ray per wave, lanes over all of B's columns, ray_meets first, then the rule, a wave
//                 minimum of the key and one store.
//   7. finalise   ray_launch_finalise (c2d_ray.hip, unchanged): the record of the winning polygon.
// There is no early termination by t: with a ray nearly collinear with an edge the rule's booleans are rounding noise, and a computed
// t says nothing reliable about where a polygon is.
//
// The walk is this file's own: another enumeration (along the segment), a grid built from B alone, outliers.  Shared with the best-key
// queries (c2d_grid_best.hpp, c2d_wave.hpp): the wave minimum of the list kernel, the reader of the _stats entry, and the place of the
// counters, the scene header's dead extent histogram.  RayGridStats keeps its own layout: n_outliers is live state of the kernels.
#include "c2d_grid_best.hpp"
#include "c2d_ray_rule.hpp"
#include "c2d_ray_walk.hpp"

namespace c2d {

constexpr uint32_t kRayWalkCap = kCandidateCap;   // sorted entries a ray may visit in the walk before it goes to the list
constexpr unsigned int kRayGridMagic = 0x52474731u;   // "RGG1": the header's counters are those of a ray query

// The counters of one call live in the scene header's extent histogram, which is dead once the cell size has been picked.
struct RayGridStats {
    unsigned long long visited;      // sorted entries the walks looked at (the aborted walks of listed rays included)
    unsigned long long candidates;   // of those, the ones that passed ray_meets
    unsigned int magic;
    unsigned int n_outliers;
};
static_assert(sizeof(RayGridStats) <= sizeof(unsigned int) * kHistBins && offsetof(BroadGrid, hist) == 0, "the counters sit at the start of the scene header");

C2D_DEV RayGridStats* ray_grid_stats(BroadGrid* g) { return reinterpret_cast<RayGridStats*>(g->hist); }
C2D_DEV float key_to_float(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }   // (c2d_broad.hip f2key's inverse)

struct RayBoxSet {
    PolySetDev set;
    uint32_t* async_err;   // the ctx's asynchronous error word (pinned host memory)
};

// The box of polygon j's live vertices (count k in 1..rows) as (xl, yl, xh, yh); false: a NaN live coordinate (the polygon is unboxed).
C2D_DEV bool ray_vertex_box(const PolySetDev& X, size_t j, int k, float4& box)
{
    float xl = X.vx[j], xh = xl, yl = X.vy[j], yh = yl;
    bool nan = __builtin_isnan(xl) || __builtin_isnan(yl);
    for (int e = 1; e < k; e++) {
        const float x = X.vx[(size_t)e * X.stride + j], y = X.vy[(size_t)e * X.stride + j];
        nan = nan || __builtin_isnan(x) || __builtin_isnan(y);
        xl = __builtin_fminf(xl, x);
        xh = __builtin_fmaxf(xh, x);
        yl = __builtin_fminf(yl, y);
        yh = __builtin_fmaxf(yh, y);
    }
    box = make_float4(xl, yl, xh, yh);
    return !nan;
}

// the box policy of the pipeline (c2d_broad.hpp) for this query: only Set and box() are used
struct RayBoxShape {
    using Set = RayBoxSet;
    static C2D_DEV int box(const Set& X, size_t j, float4& b)
    {
        int k;
        if (!poly_count(X.set, j, k)) {
            __hip_atomic_fetch_or(X.async_err, C2D_ASYNC_ERR_POLY_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return kBroadAbsent;
        }
        if (!ray_vertex_box(X.set, j, k, b)) return kBroadWild;
        const bool finite = __builtin_isfinite(b.x) && __builtin_isfinite(b.y) && __builtin_isfinite(b.z) && __builtin_isfinite(b.w);
        return finite ? kBroadRegular : kBroadWild;
    }
};

// The contract's per-polygon rule for one ray (c2d_ray.hip's, with the same bits): t of polygon j, 0 when the origin is inside, +inf
// when the ray does not touch it.  With_box: the polygon's box is made on the way and the polygon only counts if it is unboxed or
// ray_meets holds.  k is in 1..rows: rows e, e1 < k lie inside the planes.
template <bool With_box>
C2D_DEV float ray_poly_t(const PolySetDev& B, size_t j, int k, float ox, float oy, float dx, float dy, const RayD& rd)
{
    const float xf = B.vx[j], yf = B.vy[j];
    float x0 = xf, y0 = yf;
    float xl = xf, xh = xf, yl = yf, yh = yf;
    bool boxed = !(__builtin_isnan(xf) || __builtin_isnan(yf));
    bool pos = false, neg = false, unordered = false;
    float tmin = __builtin_inff();
#pragma unroll 1
    for (int e = 0; e < k; e++) {
        const bool wrap = e + 1 >= k;
        const float x1 = wrap ? xf : B.vx[(size_t)(e + 1) * B.stride + j], y1 = wrap ? yf : B.vy[(size_t)(e + 1) * B.stride + j];
        if (With_box && !wrap) {
            boxed = boxed && !(__builtin_isnan(x1) || __builtin_isnan(y1));
            xl = __builtin_fminf(xl, x1);
            xh = __builtin_fmaxf(xh, x1);
            yl = __builtin_fminf(yl, y1);
            yh = __builtin_fmaxf(yh, y1);
        }
        const RayEdge x = ray_edge(ox, oy, dx, dy, x0, y0, x1 - x0, y1 - y0);
        pos |= x.tn > 0.0f;
        neg |= x.tn < 0.0f;
        unordered |= __builtin_isnan(x.tn);
        if (ray_edge_usable(x)) {
            const float t = x.tn / x.den;
            tmin = t < tmin ? t : tmin;
        }
        x0 = x1;
        y0 = y1;
    }
    if (With_box && boxed && !ray_meets(rd, xl, xh, yl, yh)) return __builtin_inff();
    const bool inside = !unordered && (pos != neg);
    return inside ? 0.0f : tmin;
}

__global__ void ray_grid_begin_kernel(BroadGrid* __restrict__ g)
{
    if (threadIdx.x != 0) return;
    RayGridStats* st = ray_grid_stats(g);
    st->visited = 0ull;
    st->candidates = 0ull;
    st->magic = kRayGridMagic;
    st->n_outliers = 0u;
    g->n_long = 0u;
}

// 4. the regular boxes that the bounds pass left out (extent at or above the cell-size pick: the same compare as broad_bounds_kernel)
__global__ __launch_bounds__(kBroadBlock) void ray_outlier_kernel(const float4* __restrict__ sbox, const uint32_t* __restrict__ idx, size_t n_b,
                                                                  BroadGrid* __restrict__ g, uint32_t* __restrict__ outliers)
{
    const size_t n_reg = g->n_reg_b < n_b ? g->n_reg_b : n_b;
    const float s = g->s;
    for (size_t k = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; k < n_reg; k += (size_t)gridDim.x * kBroadBlock) {
        if (box_extent(sbox[k]) < s) continue;
        const unsigned int slot = atomicAdd(&ray_grid_stats(g)->n_outliers, 1u);   // each entry at most once: slot < n_b
        if ((size_t)slot < n_b) outliers[slot] = idx[k];
    }
}

struct RayGridQuery {
    RayPlanes R;
    PolySetDev B;
    const uint32_t* keys;       // [n_b] sorted keys: regular ones first, then kWildKey, then kAbsentKey
    const uint32_t* idx;        // [n_b] index of each sorted key
    const float4* sbox;         // [n_b] boxes in key order (xl, yl, xh, yh)
    const uint32_t* outliers;   // [n_outliers] indices of the regular boxes outside the walk's proof
    BroadGrid* g;
    uint32_t* listed;           // [n_rays] the rays left to the list kernel (g->n_long of them)
    size_t n_rays;
    uint32_t col_base;
};

// 5. the walk: one ray per lane
__global__ __launch_bounds__(kRayBlock) void ray_walk_kernel(RayGridQuery q, c2d_ray_hit* __restrict__ out)
{
    const size_t r = (size_t)blockIdx.x * kRayBlock + threadIdx.x;
    const bool valid = r < q.n_rays;
    BroadGrid* g = q.g;
    const size_t n_b = q.B.n;
    const uint32_t n_reg = g->n_reg_b < n_b ? g->n_reg_b : (uint32_t)n_b;
    const uint32_t n_out = ray_grid_stats(g)->n_outliers < n_b ? ray_grid_stats(g)->n_outliers : (uint32_t)n_b;
    unsigned long long visited = 0, met = 0;
    if (valid) {
        const float ox = q.R.ox[r], oy = q.R.oy[r], dx = q.R.dx[r], dy = q.R.dy[r];
        const RayD rd = ray_d(ox, oy, dx, dy);
        WalkGrid wg;
        wg.x0 = g->x0;
        wg.y0 = g->y0;
        wg.ix = g->ix;
        wg.iy = g->iy;
        wg.gx = g->gx;
        wg.gy = g->gy;
        wg.G = 0.0;
        if (g->hi_x != 0u) {   // (some box lies inside the bounds)
            const double a = __builtin_fmax(__builtin_fabs((double)key_to_float(g->lo_x)), __builtin_fabs((double)key_to_float(g->hi_x)));
            const double b = __builtin_fmax(__builtin_fabs((double)key_to_float(g->lo_y)), __builtin_fabs((double)key_to_float(g->hi_y)));
            wg.G = __builtin_fmax(a, b);
        }
        RayWalk w;
        bool walked = ray_walk_begin(wg, rd, w);
        unsigned long long best = kSetNoKey;
        if (walked) {
            uint32_t seen = 0;
#pragma unroll 1
            for (uint32_t row = w.row0; walked && row <= w.row1; row++) {
                uint32_t c0, c1;
                ray_walk_row(wg, w, row, c0, c1);
                const uint32_t k_lo = row * wg.gx + c0, k_hi = row * wg.gx + c1;
#pragma unroll 1
                for (uint32_t k = lower_bound_u32(q.keys, n_reg, k_lo); k < n_reg && q.keys[k] <= k_hi; k++) {
                    if (++seen > kRayWalkCap) {
                        walked = false;
                        break;
                    }
                    const float4 b = q.sbox[k];
                    if (!ray_meets(rd, b.x, b.z, b.y, b.w)) continue;
                    met++;
                    const uint32_t j = q.idx[k];
                    int kk;
                    if ((size_t)j >= n_b || !poly_count(q.B, j, kk)) continue;   // (never: a sorted regular entry is a polygon of B with a good count)
                    const float t = ray_poly_t<false>(q.B, j, kk, ox, oy, dx, dy, rd);
                    if (t < __builtin_inff()) {
                        const unsigned long long key = ray_key(t, q.col_base + j);
                        best = key < best ? key : best;
                    }
                }
            }
            visited = seen < kRayWalkCap ? seen : kRayWalkCap;
        }
        if (walked) {
            // the outliers, then the wild tail (it ends where the absent polygons begin): each against its own box, made on the way
#pragma unroll 1
            for (size_t k = 0; k < (size_t)n_out + (n_b - n_reg); k++) {
                uint32_t j;
                if (k < n_out) {
                    j = q.outliers[k];
                } else {
                    const size_t at = n_reg + (k - n_out);
                    if (q.keys[at] == kAbsentKey) break;
                    j = q.idx[at];
                }
                int kk;
                if ((size_t)j >= n_b || !poly_count(q.B, j, kk)) continue;
                const float t = ray_poly_t<true>(q.B, j, kk, ox, oy, dx, dy, rd);
                if (t < __builtin_inff()) {
                    const unsigned long long key = ray_key(t, q.col_base + j);
                    best = key < best ? key : best;
                }
            }
            if (best != kSetNoKey) reinterpret_cast<unsigned long long*>(out)[2 * r] = best;
        } else {
            const unsigned int slot = atomicAdd(&g->n_long, 1u);   // each ray at most once: slot < n_rays
            if ((size_t)slot < q.n_rays) q.listed[slot] = (uint32_t)r;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        visited += __shfl_down(visited, off, 64);
        met += __shfl_down(met, off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (visited) atomicAdd(&ray_grid_stats(g)->visited, visited);
        if (met) atomicAdd(&ray_grid_stats(g)->candidates, met);
    }
}

// 6. the listed rays: one ray per wave over all of B's columns
__global__ __launch_bounds__(kBroadBlock) void ray_list_kernel(RayGridQuery q, c2d_ray_hit* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_long = q.g->n_long;
    const size_t n_b = q.B.n;
    const size_t waves = (size_t)gridDim.x * (kBroadBlock / 64);
    for (size_t w = (size_t)blockIdx.x * (kBroadBlock / 64) + (threadIdx.x >> 6); w < n_long && w < q.n_rays; w += waves) {
        const size_t r = q.listed[w];
        if (r >= q.n_rays) continue;
        const float ox = q.R.ox[r], oy = q.R.oy[r], dx = q.R.dx[r], dy = q.R.dy[r];
        const RayD rd = ray_d(ox, oy, dx, dy);
        unsigned long long best = kSetNoKey;
        for (size_t j = lane; j < n_b; j += 64) {
            int kk;
            if (!poly_count(q.B, j, kk)) continue;   // absent (the box pass has reported it)
            const float t = ray_poly_t<true>(q.B, j, kk, ox, oy, dx, dy, rd);
            if (t < __builtin_inff()) {
                const unsigned long long key = ray_key(t, q.col_base + (uint32_t)j);
                best = key < best ? key : best;
            }
        }
        best = wave_min_u64(best);
        if (lane == 0 && best != kSetNoKey) reinterpret_cast<unsigned long long*>(out)[2 * r] = best;
    }
}

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_ray_casts_grid(c2d_ctx* ctx, const float* const d_rays[4], size_t n_rays, const c2d_poly_set* b, size_t col_base, c2d_ray_hit* d_out,
                            c2d_stream stream)
{
    const char* what = "c2d_poly_ray_casts_grid";
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!d_rays || !b || !d_out) return cross_fail(ctx, what, "NULL argument");
    if (n_rays == 0) return C2D_OK;
    PolySetDev B;
    if (int rc = ray_check_args(ctx, what, d_rays, n_rays, b, col_base, d_out, B)) return rc;

    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const RayPlanes R{d_rays[0], d_rays[1], d_rays[2], d_rays[3]};
    if (B.n == 0) {   // no grid, no scratch: the no-hit record for every ray
        if (int rc = set_best_launch_init<2>(ctx, s, n_rays, d_out)) return rc;
        return ray_launch_finalise(ctx, s, R, n_rays, B, (uint32_t)col_base, d_out);
    }
    // the scratch of a pair search of n_rays rows against B: the row list holds the listed rays; B's boxes are the only boxes
    BroadScratch W;
    if (int rc = broad_scratch(ctx, s, what, n_rays, B.n, false, W)) return rc;
    WorkspaceUse use(ctx, s);   // the kernels work through the scratch: stamp behind the last one
    use.arm();
    if (int rc = broad_begin(ctx, s, W)) return rc;
    const int grid_b = grid_for(B.n, kBroadBlock, 8192);
    const RayBoxSet S{B, ctx->d_async_err};
    hipLaunchKernelGGL(broad_box_kernel<RayBoxShape>, dim3(grid_b), dim3(kBroadBlock), 0, s, S, B.n, W.box_b, W.g);
    C2D_LAUNCH_CHECK(ctx);
    W.box_a = W.box_b;   // the grid is built from B alone: "A is B" to the shape-independent stages
    if (int rc = broad_grid_and_sort(ctx, s, W, B.n, B.n, true)) return rc;
    uint32_t* outliers = W.keys == W.keys0 ? W.keys1 : W.keys0;   // the sort's other buffer is free again

    if (int rc = set_best_launch_init<2>(ctx, s, n_rays, d_out)) return rc;
    hipLaunchKernelGGL(ray_grid_begin_kernel, dim3(1), dim3(64), 0, s, W.g);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(ray_outlier_kernel, dim3(grid_b), dim3(kBroadBlock), 0, s, (const float4*)W.sbox, W.idx, B.n, W.g, outliers);
    C2D_LAUNCH_CHECK(ctx);
    const RayGridQuery q{R, B, W.keys, W.idx, W.sbox, outliers, W.g, W.long_rows, n_rays, (uint32_t)col_base};
    hipLaunchKernelGGL(ray_walk_kernel, dim3((unsigned)((n_rays + kRayBlock - 1) / kRayBlock)), dim3(kRayBlock), 0, s, q, d_out);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(ray_list_kernel, dim3(kLongGrid), dim3(kBroadBlock), 0, s, q, d_out);
    C2D_LAUNCH_CHECK(ctx);
    if (int rc = ray_launch_finalise(ctx, s, R, n_rays, B, (uint32_t)col_base, d_out)) return rc;
    use.done();
    return C2D_OK;
}

/* The counters of the last c2d_poly_ray_casts_grid call with n_b > 0 on this ctx (a blocking read of the scene header). */
int c2d_poly_ray_casts_grid_stats(c2d_ctx* ctx, unsigned long long out[4])
{
    RayGridStats st;
    unsigned int n_long;
    if (int rc = grid_stats_read(ctx, "c2d_poly_ray_casts_grid_stats", out, "no grid ray query has run on this ctx",
                                 "the ctx scratch does not hold a grid ray query (another call has used it since)", kRayGridMagic, st, n_long))
        return rc;
    out[0] = n_long;
    out[1] = st.visited;
    out[2] = st.candidates;
    out[3] = st.n_outliers;
    return C2D_OK;
}

}  // extern "C"
