// c2d_ray.hip — ray queries for gfx950 (MI355X): for every segment o -> o + d of a list the polygon of a set B it touches first, and
// where (c2d_poly_ray_casts; include/c2d.h "ray queries").  An R x M reduction: no R x M object is ever written.
//
// The rule (the contract of include/c2d.h).  Per ray, polygon j and live edge e < k, from vertex e at (x0, y0) to vertex (e + 1) mod k
// at (x1, y1), everything binary32 and unfused, each product first and then the difference:
//     ex = x1 - x0, ey = y1 - y0, wx = x0 - ox, wy = y0 - oy, den = dx * ey - dy * ex, tn = wx * ey - wy * ex, un = wx * dy - wy * dx
//     usable:  den > 0 && 0 <= tn <= den && 0 <= un <= den,  or  den < 0 && den <= tn <= 0 && den <= un <= 0;  then t = tn / den, u = un / den
//     inside:  no live tn is NaN, and exactly one sign occurs among the live tn; an inside polygon is the candidate t = 0
// Polygons in order of j, per polygon the inside candidate and then the edges in order of e; a candidate replaces the best only under
// strict t < best.  So the smallest t wins, among equal t the smallest j, then inside before edges, then the smallest e.
//
// The frame is c2d_set_best.hpp's (the mapping, the strips, the three launches); the query in a lane's registers is a ray (four
// VGPRs), and a tile stages the edges {x0, y0, ex, ey} and the counts alone.  Per edge a lane makes the three cross products and the
// compares, and the two divisions become one (t alone) under a wave-uniform "some lane has a usable edge" branch.
//   main      ray_main_kernel: the key's value is t, a -0 made +0: for 0 <= t <= 1 the order of the bits is the order of t
//   finalise  ray_finalise_kernel, one lane per ray: re-evaluates the winning polygon alone (at most 16 edges) by the rule's own
//             sequence and writes the whole record with one 16-byte store.
#include "c2d_ray_rule.hpp"

namespace c2d {

static_assert(sizeof(c2d_ray_hit) == 16 && offsetof(c2d_ray_hit, poly) == 0 && offsetof(c2d_ray_hit, t) == 4 && offsetof(c2d_ray_hit, u) == 8 &&
                  offsetof(c2d_ray_hit, edge) == 12 && offsetof(c2d_ray_hit, hit) == 14 && offsetof(c2d_ray_hit, flags) == 15,
              "the kernels treat a ray hit as four dwords, (poly, t) being the 64-bit key");

// Block b: row tile b / strips, strip b % strips of the col_tiles column tiles of B.
__global__ __launch_bounds__(kSetBlock) void ray_main_kernel(RayPlanes R, size_t n_rays, PolySetDev B, uint32_t col_base, size_t col_tiles, uint32_t strips,
                                                             c2d_ray_hit* __restrict__ out, uint32_t* __restrict__ async_err)
{
    __shared__ __attribute__((aligned(16))) float4 s_edge[kSetCols][kSetK];   // 16 KiB: {x0, y0, ex, ey} of every live edge
    __shared__ int s_k[kSetCols];                                             // the count; 0: not in any hit (out of range, or beyond n)
    const uint32_t lane = threadIdx.x;
    const size_t r = (size_t)(blockIdx.x / strips) * kSetBlock + lane;
    const bool row_valid = r < n_rays;
    // a lane without a ray carries NaN: every compare below fails, and it writes nothing
    const float nan = __builtin_nanf("");
    const float ox = row_valid ? R.ox[r] : nan, oy = row_valid ? R.oy[r] : nan, dx = row_valid ? R.dx[r] : nan, dy = row_valid ? R.dy[r] : nan;

    float best_t = __builtin_inff();
    uint32_t best_j = 0xFFFFFFFFu;
    // (the strip, the tile loop and the staging of the frame, spelt out in each of the three main kernels: c2d_set_best.hpp says why)
    size_t tile0, tiles;
    ray_strip_tiles(col_tiles, (size_t)strips, (size_t)(blockIdx.x % strips), tile0, tiles);
#pragma unroll 1
    for (size_t tile = tile0; tile < tile0 + tiles; tile++) {
        const size_t j0 = tile * (size_t)kSetCols;
        const uint32_t nj = (uint32_t)(B.n - j0 < (size_t)kSetCols ? B.n - j0 : (size_t)kSetCols);
        __syncthreads();   // the previous tile's readers are done
        {
            const uint32_t c = lane & 63u, g = lane >> 6;
            const size_t j = j0 + c;
            int k = 0;
            bool bad = false;
            if (c < nj) {
                bad = !poly_count(B, j, k);
                k = bad ? 0 : k;
            }
            if (g == 0) {   // (one whole wave)
                s_k[c] = k;
                if (__ballot(bad) != 0ull && c == 0) __hip_atomic_fetch_or(async_err, C2D_ASYNC_ERR_POLY_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
#pragma unroll
            for (int m = 0; m < kSetK / 4; m++) {
                const int e = (int)g + 4 * m;
                if (e < k) {   // e, e1 < k <= B.rows: inside the planes
                    const int e1 = e + 1 < k ? e + 1 : 0;
                    const float x0 = B.vx[(size_t)e * B.stride + j], y0 = B.vy[(size_t)e * B.stride + j];
                    const float x1 = B.vx[(size_t)e1 * B.stride + j], y1 = B.vy[(size_t)e1 * B.stride + j];
                    s_edge[c][e] = make_float4(x0, y0, x1 - x0, y1 - y0);
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t c = 0; c < nj; c++) {
            const int k = __builtin_amdgcn_readfirstlane(s_k[c]);
            if (k == 0) continue;   // (wave-uniform)
            bool pos = false, neg = false, unordered = false;
            float tmin = __builtin_inff();
#pragma unroll 1
            for (int e = 0; e < k; e++) {
                const float4 q = s_edge[c][e];   // (one address for the wave: a broadcast)
                const RayEdge x = ray_edge(ox, oy, dx, dy, q.x, q.y, q.z, q.w);
                pos |= x.tn > 0.0f;
                neg |= x.tn < 0.0f;
                unordered |= __builtin_isnan(x.tn);
                const bool usable = ray_edge_usable(x);
                if (__ballot(usable) != 0ull) {   // (wave-uniform) rare: a ray crosses few of the edges it looks at
                    const float t = x.tn / x.den;
                    tmin = (usable && t < tmin) ? t : tmin;
                }
            }
            const bool inside = !unordered && (pos != neg);
            const float tj = inside ? 0.0f : tmin;
            const bool take = tj < best_t;   // strict: the first of equal polygons stays
            best_t = take ? tj : best_t;
            best_j = take ? (uint32_t)j0 + c : best_j;
        }
    }
    if (row_valid && best_j != 0xFFFFFFFFu)   // -0 -> +0: then the bits order as t does
        set_best_publish(best_t == 0.0f ? 0u : __float_as_uint(best_t), col_base, best_j, out, r);
}

// One lane per ray: the record of the key's polygon by the rule's own sequence (the key holds the winner's t and col_base + j).
__global__ __launch_bounds__(kRayBlock) void ray_finalise_kernel(RayPlanes R, size_t n_rays, PolySetDev B, uint32_t col_base, c2d_ray_hit* __restrict__ out)
{
    const size_t step = (size_t)gridDim.x * kRayBlock;
    for (size_t r = (size_t)blockIdx.x * kRayBlock + threadIdx.x; r < n_rays; r += step) {
        const unsigned long long key = reinterpret_cast<const unsigned long long*>(out)[2 * r];
        uint4 rec = make_uint4(0xFFFFFFFFu, __float_as_uint(__builtin_inff()), 0u, kRayNone16);   // nothing chosen
        const uint32_t poly = (uint32_t)key;
        const size_t j = (size_t)(poly - col_base);   // the main pass wrote it: j < B.n (checked all the same: nothing outside B is read)
        if (key != kSetNoKey && j < B.n) {
            const float ox = R.ox[r], oy = R.oy[r], dx = R.dx[r], dy = R.dy[r];
            int k;
            (void)poly_count(B, j, k);   // in range: the polygon was in a hit
            k = k > B.rows ? B.rows : k;
            bool pos = false, neg = false, unordered = false;
            float best_t = __builtin_inff(), best_u = 0.0f;
            uint32_t best_e = kRayNone16;
            for (int e = 0; e < k; e++) {
                const int e1 = e + 1 < k ? e + 1 : 0;
                const float x0 = B.vx[(size_t)e * B.stride + j], y0 = B.vy[(size_t)e * B.stride + j];
                const float x1 = B.vx[(size_t)e1 * B.stride + j], y1 = B.vy[(size_t)e1 * B.stride + j];
                const RayEdge x = ray_edge(ox, oy, dx, dy, x0, y0, x1 - x0, y1 - y0);
                pos |= x.tn > 0.0f;
                neg |= x.tn < 0.0f;
                unordered |= __builtin_isnan(x.tn);
                if (ray_edge_usable(x)) {
                    const float t = x.tn / x.den, u = x.un / x.den;
                    const bool take = t < best_t;
                    best_t = take ? t : best_t;
                    best_u = take ? u : best_u;
                    best_e = take ? (uint32_t)e : best_e;
                }
            }
            if (!unordered && (pos != neg))
                rec = make_uint4(poly, 0u, 0u, kRayNone16 | (1u << 16) | ((uint32_t)C2D_RAY_START_INSIDE << 24));
            else if (best_e != kRayNone16)
                rec = make_uint4(poly, __float_as_uint(best_t), __float_as_uint(best_u), best_e | (1u << 16));
        }
        reinterpret_cast<uint4*>(out)[r] = rec;   // d_out is 16-byte aligned (checked on the host)
    }
}

template int set_best_launch_init<2>(c2d_ctx*, hipStream_t, size_t, void*);

int ray_launch_finalise(c2d_ctx* ctx, hipStream_t s, const RayPlanes& R, size_t n_rays, const PolySetDev& B, uint32_t col_base, c2d_ray_hit* d_out)
{
    hipLaunchKernelGGL(ray_finalise_kernel, dim3(grid_for(n_rays, kRayBlock, 1 << 16)), dim3(kRayBlock), 0, s, R, n_rays, B, col_base, d_out);
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}

int ray_check_args(c2d_ctx* ctx, const char* what, const float* const d_rays[4], size_t n_rays, const c2d_poly_set* b, size_t col_base,
                   c2d_ray_hit* d_out, PolySetDev& B)
{
    if (int rc = poly_set_check(ctx, what, "b", b, B, kEmptySetOk)) return rc;
    for (int p = 0; p < 4; p++) {
        if (!d_rays[p]) return cross_fail(ctx, what, "NULL ray plane");
        if (reinterpret_cast<uintptr_t>(d_rays[p]) & 3u) return cross_fail(ctx, what, "ray planes must be 4-byte aligned");
    }
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return cross_fail(ctx, what, "the output must be 16-byte aligned");
    if (B.n > kIndexLimit || col_base > kIndexLimit - B.n) return cross_fail(ctx, what, "col_base + n_b must not exceed 2^32");
    if (n_rays > kIndexLimit) return cross_fail(ctx, what, "n_rays must not exceed 2^32");
    return C2D_OK;
}

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_ray_casts(c2d_ctx* ctx, const float* const d_rays[4], size_t n_rays, const c2d_poly_set* b, size_t col_base, c2d_ray_hit* d_out,
                       c2d_stream stream)
{
    const char* what = "c2d_poly_ray_casts";
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!d_rays || !b || !d_out) return cross_fail(ctx, what, "NULL argument");
    if (n_rays == 0) return C2D_OK;
    PolySetDev B;
    if (int rc = ray_check_args(ctx, what, d_rays, n_rays, b, col_base, d_out, B)) return rc;

    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const RayPlanes R{d_rays[0], d_rays[1], d_rays[2], d_rays[3]};
    return set_best_run<2>(
        ctx, s, n_rays, B.n, d_out,
        [&](unsigned blocks, size_t col_tiles, uint32_t strips) {
            hipLaunchKernelGGL(ray_main_kernel, dim3(blocks), dim3(kSetBlock), 0, s, R, n_rays, B, (uint32_t)col_base, col_tiles, strips, d_out, ctx->d_async_err);
            C2D_LAUNCH_CHECK(ctx);
            return (int)C2D_OK;
        },
        [&] { return ray_launch_finalise(ctx, s, R, n_rays, B, (uint32_t)col_base, d_out); });
}

}  // extern "C"
