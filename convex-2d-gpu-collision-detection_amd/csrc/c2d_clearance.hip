// c2d_clearance.hip — clearance queries for gfx950 (MI355X): for every polygon A_i of a set the polygon of a set B nearest to it, by
// the distance contract, with the pair's whole distance record (c2d_poly_set_clearances; include/c2d.h "clearance queries",
// DESIGN.md §5.17).  An N x M reduction: no N x M object is ever written.
//
// The rule (the contract of include/c2d.h).  D(i, j) is the c2d_distance record of the pair (A_i, B_j) (c2d_distance_rule.hpp and the
// exact polygon test).  Polygon j is considered when its vertex count is within 1..rows and, under C2D_CLEARANCE_SKIP_SELF,
// row_base + i != col_base + j.  The winner is the considered j with the smallest (bits of D(i, j).dist, col_base + j); dist is never
// NaN and never -0, so the order of its bits is the order of its values, and equal distances fall to the smaller index.
//
// The frame is c2d_set_best.hpp's (the mapping, the strips, the three launches).  A lane keeps of its query the padded vertices, the
// count, the vertex box and the largest |coordinate|; a tile stages per live edge {x0, y0, ex, ey}, {x1, y1, len2, lo} and
// {ux, uy, off, hi} — len2 made once by the contract's own operations, (lo, hi) the polygon's own interval on that edge's normal
// with the NaN rule of its first projection folded in (c2d_poly_cross.hip), (ux, uy, off) the edge's outward unit normal and offset,
// a heuristic that only chooses WHICH canonical axis is tried first — and per polygon the vertex box and the largest |coordinate|.
// Per (lane, j), in order of j:
//   1. a lane whose best is already at distance 0 is done with its strip: no later j beats (+0, smaller j).
//   2. hit, the exact test, for every remaining pair: first B_j's edge that faces the query best (one canonical axis; an axis that
//      separates decides the pair), then behind a wave-uniform branch all axes of both polygons for the pairs it did not decide.
//      The box bound never skips this: nothing proves that the float SAT calls a box-separated pair separated.
//   3. not hit: the certified bound of c2d_clearance_bound.hpp from the two boxes; when it exceeds the lane's best d2 (strictly) the
//      candidates of the pair are skipped, else min d2 over both sides runs under strict < from +inf (a NaN d2 never enters) and one
//      square root gives the pair's dist.  The minimum's VALUE does not depend on the candidates' order, and the value is all the
//      key needs: the finalise pass recomputes the winner's record by the rule's own sequence.
//
//   main      clearance_main_kernel: the key's value is dist
//   finalise  clearance_finalise_kernel, one lane per query: A_i and the winner in registers, the exact test and the distance record
//             by the routines the distance kernel uses, the whole record in two 16-byte stores
#include "c2d_distance_rule.hpp"
#include "c2d_clearance_bound.hpp"
#include "c2d_clearance_parts.hpp"   // the last launch, which c2d_clearance_grid.hip shares; through it c2d_set_best.hpp
#include "c2d_pair_list.hpp"   // PolySetDev, PolyObj, poly_load, poly_collide, the shared argument checks
#include "c2d_wave.hpp"

namespace c2d {

static_assert(sizeof(c2d_clearance) == 32 && offsetof(c2d_clearance, poly) == 0 && offsetof(c2d_clearance, dist) == 4 && offsetof(c2d_clearance, ax) == 8 &&
                  offsetof(c2d_clearance, bx) == 16 && offsetof(c2d_clearance, edge) == 24 && offsetof(c2d_clearance, vert) == 26 &&
                  offsetof(c2d_clearance, hit) == 28 && offsetof(c2d_clearance, flags) == 29 && offsetof(c2d_clearance, reserved0) == 30,
              "the kernels treat a clearance as two halves of four dwords, (poly, dist) being the 64-bit key");

// d2 of one candidate by the contract's own sequence: the edge (x0, y0) -> (x1, y1) with its vector and len2, the vertex (xq, yq)
C2D_DEV float clearance_candidate(float x0, float y0, float x1, float y1, float ex, float ey, float len2, float xq, float yq)
{
    const float ux = xq - x0, uy = yq - y0;
    const float s = ux * ex + uy * ey;
    const bool r0 = s <= 0.0f, r1 = s >= len2;   // (region 0 first; a NaN s fails both and takes region 2)
    const float t = s / len2;
    const float tx = x0 + t * ex, ty = y0 + t * ey;
    const float cx = r0 ? x0 : (r1 ? x1 : tx), cy = r0 ? y0 : (r1 ? y1 : ty);
    const float dx = xq - cx, dy = yq - cy;
    return dx * dx + dy * dy;
}

// Block b: row tile b / strips, strip b % strips of the col_tiles column tiles of B.
__global__ __launch_bounds__(kSetBlock) void clearance_main_kernel(PolySetDev A, PolySetDev B, size_t row_base, size_t col_base, int skip_self, size_t col_tiles,
                                                                   uint32_t strips, c2d_clearance* __restrict__ out, uint32_t* __restrict__ async_err)
{
    __shared__ __attribute__((aligned(16))) float4 s_edge[kSetCols][kSetK];   // 16 KiB: {x0, y0, ex, ey} of every live edge
    __shared__ __attribute__((aligned(16))) float4 s_aux[kSetCols][kSetK];    // 16 KiB: {x1, y1, len2, lo}
    __shared__ __attribute__((aligned(16))) float4 s_face[kSetCols][kSetK];   // 16 KiB: {ux, uy, off, hi}
    __shared__ ClearanceBox s_box[kSetCols];
    __shared__ int s_k[kSetCols];   // the count; 0: not considered by any query (out of range, or beyond n)
    const uint32_t lane = threadIdx.x;
    const float inf = __builtin_inff();

    // (the same text, up to what this query adds, in c2d_cast.hip; spelt out in both: c2d_set_best.hpp says why)
    // ---- the lane's query: count, padded vertices, vertex box, largest |coordinate| --------------------------------------------
    const size_t i = (size_t)(blockIdx.x / strips) * kSetBlock + lane;
    const bool row_valid = i < A.n;
    int ka = 1;
    bool bad_a = false;
    if (row_valid) bad_a = !poly_count(A, i, ka);
    ka = bad_a ? 1 : ka;
    const bool row_live = row_valid && !bad_a;   // (a query with a count out of range gets its record from the finalise pass)
    const int kmax_a = (int)wave_max_u32((uint32_t)ka);   // wave-uniform bound of the loops over A's slots
    float ax[kSetK], ay[kSetK];
#pragma unroll
    for (int r = 0; r < kSetK; r++) {
        ax[r] = 0.0f;
        ay[r] = 0.0f;
        if (row_live && r < ka) {   // r < ka <= A.rows: inside the planes
            ax[r] = A.vx[(size_t)r * A.stride + i];
            ay[r] = A.vy[(size_t)r * A.stride + i];
        }
    }
    ClearanceBox abox{ax[0], ax[0], ay[0], ay[0], 0.0f};
    {
        float c = __builtin_fmaxf(__builtin_fabsf(ax[0]), __builtin_fabsf(ay[0]));
        bool finite = (__builtin_fabsf(ax[0]) < inf) & (__builtin_fabsf(ay[0]) < inf);
#pragma unroll
        for (int r = 1; r < kSetK; r++) {
            const bool used = r < ka;
            ax[r] = used ? ax[r] : ax[0];   // neutral padding: a repeated vertex adds a zero-length edge and repeats a projection
            ay[r] = used ? ay[r] : ay[0];
            abox.xlo = __builtin_fminf(abox.xlo, ax[r]);
            abox.xhi = __builtin_fmaxf(abox.xhi, ax[r]);
            abox.ylo = __builtin_fminf(abox.ylo, ay[r]);
            abox.yhi = __builtin_fmaxf(abox.yhi, ay[r]);
            c = __builtin_fmaxf(c, __builtin_fmaxf(__builtin_fabsf(ax[r]), __builtin_fabsf(ay[r])));
            finite &= (__builtin_fabsf(ax[r]) < inf) & (__builtin_fabsf(ay[r]) < inf);
        }
        abox.c = finite ? c : inf;   // a NaN or an infinite coordinate: never skipped
    }
    const float cax = 0.5f * abox.xlo + 0.5f * abox.xhi, cay = 0.5f * abox.ylo + 0.5f * abox.yhi;   // (heuristic only)
    const float ax0 = ax[0], ay0 = ay[0];   // vertex 0, whichever way the polygon is turned
    const size_t gi = row_base + i;

    // (the strip, the tile loop and the staging of the frame, spelt out in each of the three main kernels: c2d_set_best.hpp says why)
    size_t tile0, tiles;
    ray_strip_tiles(col_tiles, (size_t)strips, (size_t)(blockIdx.x % strips), tile0, tiles);

    float best_dist = inf, best_d2 = inf;
    uint32_t best_j = 0;
    bool have = false;
#pragma unroll 1
    for (size_t tile = tile0; tile < tile0 + tiles; tile++) {
        const size_t j0 = tile * (size_t)kSetCols;
        const uint32_t nj = (uint32_t)(B.n - j0 < (size_t)kSetCols ? B.n - j0 : (size_t)kSetCols);
        __syncthreads();   // the previous tile's readers are done
        // ---- stage 64 polygons: edges, len2, the count ---------------------------------------------------------------------------
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
                    const float ex = x1 - x0, ey = y1 - y0;
                    s_edge[c][e] = make_float4(x0, y0, ex, ey);
                    s_aux[c][e] = make_float4(x1, y1, ex * ex + ey * ey, 0.0f);
                }
            }
        }
        __syncthreads();
        // (the own interval, the NaN bit and the outward sign are the same text in c2d_cast.hip; spelt out in both: c2d_set_best.hpp)
        // ---- hoist: lane (polygon c, edge a) -> the own interval on the edge's normal and the facing heuristic; (c, 0): the box ------
#pragma unroll 1
        for (int m = 0; m < kSetCols * kSetK / kSetBlock; m++) {
            const uint32_t item = lane + (uint32_t)kSetBlock * m, c = item >> 4, a = item & 15u;
            const int k = s_k[c];
            if ((int)a < k) {
                const float4 ed = s_edge[c][a];
                const float nx = -ed.w, ny = ed.z;   // the true normal (-e.y, e.x) of the exact test
                float mn = inf, mx = -inf;
                for (int r = 0; r < k; r++) {
                    const float4 v = s_edge[c][r];
                    poly_minmax(nx, ny, v.x, v.y, mn, mx);
                }
                const float4 v0 = s_edge[c][0];
                const bool nan0 = __builtin_isnan(nx * v0.x + ny * v0.y);
                const float lo = nan0 ? -inf : mn, hi = nan0 ? inf : mx;
                // outward: away from the side the polygon's own projections extend to (heuristic only; fast arithmetic)
                const float pa = nx * ed.x + ny * ed.y;
                const float len2 = s_aux[c][a].z;
                const float sg = (mx - pa) > (pa - mn) ? -1.0f : 1.0f;
                const float inv = sg * __builtin_amdgcn_rsqf(len2);
                s_aux[c][a].w = lo;
                s_face[c][a] = make_float4(nx * inv, ny * inv, pa * inv, hi);
            }
            if (a == 0 && k > 0) {
                const float4 v0 = s_edge[c][0];
                ClearanceBox bb{v0.x, v0.x, v0.y, v0.y, 0.0f};
                float cm = 0.0f;
                bool finite = true;
                for (int r = 0; r < k; r++) {
                    const float4 v = s_edge[c][r];
                    bb.xlo = __builtin_fminf(bb.xlo, v.x);
                    bb.xhi = __builtin_fmaxf(bb.xhi, v.x);
                    bb.ylo = __builtin_fminf(bb.ylo, v.y);
                    bb.yhi = __builtin_fmaxf(bb.yhi, v.y);
                    cm = __builtin_fmaxf(cm, __builtin_fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)));
                    finite &= (__builtin_fabsf(v.x) < inf) & (__builtin_fabsf(v.y) < inf);
                }
                bb.c = finite ? cm : inf;
                s_box[c] = bb;
            }
        }
        __syncthreads();
        // ---- the pairs ------------------------------------------------------------------------------------------------------------
        if (__ballot(row_live && !(have && best_dist == 0.0f)) == 0ull) continue;   // (wave-uniform) a wave of finished lanes skips the tile
#pragma unroll 1
        for (uint32_t c = 0; c < nj; c++) {
            const int k = __builtin_amdgcn_readfirstlane(s_k[c]);
            if (k == 0) continue;   // (wave-uniform) a count out of range: not considered
            const size_t gj = col_base + j0 + c;
            const bool considered = row_live && !(have && best_dist == 0.0f) && !(skip_self && gi == gj);
            if (__ballot(considered) == 0ull) continue;   // (wave-uniform)
            // (the pick below is the same text in c2d_cast.hip, over another staged layout; spelt out in both: c2d_set_best.hpp)
            // step 2, first axis: the edge of B_j whose outward normal sees the query's box centre farthest out
            uint32_t fe = 0;
            {
                float fs = -inf;
#pragma unroll 1
                for (int e = 0; e < k; e++) {
                    const float4 f = s_face[c][e];   // (one address for the wave: a broadcast)
                    const float sc = fma_(f.x, cax, fma_(f.y, cay, -f.z));
                    const bool better = sc > fs;
                    fs = better ? sc : fs;
                    fe = better ? (uint32_t)e : fe;
                }
            }
            bool sep;
            {
                const float4 ed = s_edge[c][fe];
                const float nx = -ed.w, ny = ed.z, lo = s_aux[c][fe].w, hi = s_face[c][fe].w;
                float mn = inf, mx = -inf;
#pragma unroll
                for (int r = 0; r < kSetK; r++)
                    if (r < kmax_a) poly_minmax(nx, ny, ax[r], ay[r], mn, mx);
                // (B_j's own first projection is folded into lo / hi; A_i's is checked here: first_projections_ordered)
                sep = ((hi < mn) || (mx < lo)) && !__builtin_isnan(nx * ax[0] + ny * ay[0]);
            }
            if (__ballot(considered && !sep) != 0ull) {   // (wave-uniform) the pairs the first axis did not decide: every axis of both
                // A's axes: always the one from slot 0 to slot 1, A turned by one slot per trip and back in place after 16 (the loop
                // stays rolled and nothing of an edge is kept across pairs); slot ka is vertex 0 again, so the polygon closes itself
#pragma unroll 1
                for (int a = 0; a < kSetK; a++) {
                    if (a < kmax_a) {   // (wave-uniform) beyond it every lane's axis is a zero vector: it never separates
                        const float nx = -(ay[1] - ay[0]), ny = ax[1] - ax[0];
                        float mnp = inf, mxp = -inf, mnq = inf, mxq = -inf;
#pragma unroll
                        for (int r = 0; r < kSetK; r++) poly_minmax(nx, ny, ax[r], ay[r], mnp, mxp);
#pragma unroll 1
                        for (int r = 0; r < k; r++) {
                            const float4 v = s_edge[c][r];
                            poly_minmax(nx, ny, v.x, v.y, mnq, mxq);
                        }
                        const float4 v0 = s_edge[c][0];
                        sep |= a < ka && ((mxp < mnq) || (mxq < mnp)) && first_projections_ordered(nx * ax0 + ny * ay0, nx * v0.x + ny * v0.y);
                    }
                    set_best_turn(ax, ay);
                }
#pragma unroll 1
                for (int eb = 0; eb < k; eb++) {
                    const float4 ed = s_edge[c][eb];
                    const float nx = -ed.w, ny = ed.z, lo = s_aux[c][eb].w, hi = s_face[c][eb].w;
                    float mn = inf, mx = -inf;
#pragma unroll
                    for (int r = 0; r < kSetK; r++)
                        if (r < kmax_a) poly_minmax(nx, ny, ax[r], ay[r], mn, mx);
                    sep |= ((hi < mn) || (mx < lo)) && !__builtin_isnan(nx * ax[0] + ny * ay[0]);
                }
            }
            const bool hit = considered && !sep;
            // step 3: the certified bound, then the candidates of the pairs it does not skip
#ifdef C2D_CLEARANCE_NO_SKIP   // measurement build only (`make lib-ab-clearance`): the straight kernel, for csrc/tools/clearance_bench.py
            const float lb2 = 0.0f;
#else
            const float lb2 = clearance_lb2(abox, s_box[c]);
#endif
            const bool run = considered && !hit && !(lb2 > best_d2);
            float d2min = inf;
            if (__ballot(run) != 0ull) {   // (wave-uniform)
                // side 0: A's edges (registers) against B_j's vertices
#pragma unroll 1
                for (int e = 0; e < kSetK; e++) {   // (A turned by one slot per trip, as above)
                    if (e < kmax_a) {   // (wave-uniform)
                        const float x0 = ax[0], y0 = ay[0], x1 = ax[1], y1 = ay[1];
                        const float ex = x1 - x0, ey = y1 - y0;
                        const float len2 = ex * ex + ey * ey;
                        const bool live_e = e < ka;
#pragma unroll 1
                        for (int v = 0; v < k; v++) {
                            const float4 q = s_edge[c][v];
                            const float d2 = clearance_candidate(x0, y0, x1, y1, ex, ey, len2, q.x, q.y);
                            d2min = (live_e && d2 < d2min) ? d2 : d2min;   // strict, from +inf: a NaN never enters
                        }
                    }
                    set_best_turn(ax, ay);
                }
                // side 1: B_j's edges against A's vertices (registers)
#pragma unroll 1
                for (int e = 0; e < k; e++) {
                    const float4 ed = s_edge[c][e], au = s_aux[c][e];
#pragma unroll
                    for (int v = 0; v < kSetK; v++) {
                        if (v < kmax_a) {   // (wave-uniform)
                            const float d2 = clearance_candidate(ed.x, ed.y, au.x, au.y, ed.z, ed.w, au.z, ax[v], ay[v]);
                            d2min = (v < ka && d2 < d2min) ? d2 : d2min;
                        }
                    }
                }
            }
            const float dist = hit ? 0.0f : __builtin_sqrtf(d2min);
            const bool take = (hit || run) && (!have || dist < best_dist);   // strict: the first of equal polygons stays
            best_dist = take ? dist : best_dist;
            best_d2 = take ? (hit ? 0.0f : d2min) : best_d2;
            best_j = take ? (uint32_t)(j0 + c) : best_j;
            have |= take;
        }
    }
    if (have) set_best_publish(best_dist == 0.0f ? 0u : __float_as_uint(best_dist), (uint32_t)col_base, best_j, out, i);   // (never -0; all the same)
}

// (The wave-trip loop, the bad-count report, the key decode and the two loads are the same text in c2d_cast.hip; spelt out in both,
// because as one routine or kernel template they changed this kernel's code: c2d_set_best.hpp.)
// One lane per query: the record of the key's polygon by the routines of the distance kernel (the key holds col_base + j).
__global__ __launch_bounds__(kSetBlock) void clearance_finalise_kernel(PolySetDev A, PolySetDev B, size_t col_base, c2d_clearance* __restrict__ out,
                                                                       uint32_t* __restrict__ async_err)
{
    const size_t step = (size_t)gridDim.x * kSetBlock;
    // every lane of a wave makes the same trips: the ballot below sees whole waves
    for (size_t i0 = (size_t)blockIdx.x * kSetBlock + (threadIdx.x & ~63u); i0 < A.n; i0 += step) {
        const size_t i = i0 + (threadIdx.x & 63u);
        const bool in = i < A.n;
        int ka = 1;
        const bool bad_a = in && !poly_count(A, i, ka);
        if (__ballot(bad_a) != 0ull && (threadIdx.x & 63u) == 0) __hip_atomic_fetch_or(async_err, C2D_ASYNC_ERR_POLY_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (!in) continue;
        const unsigned long long key = reinterpret_cast<const unsigned long long*>(out)[4 * i];
        // nothing considered
        uint4 d0 = make_uint4(0xFFFFFFFFu, __float_as_uint(__builtin_inff()), 0u, 0u), d1 = make_uint4(0u, 0u, kDistanceNone, (uint32_t)C2D_CLEARANCE_NONE << 8);
        const uint32_t poly = (uint32_t)key;
        const size_t j = (size_t)(uint32_t)(poly - (uint32_t)col_base);   // the main pass wrote it: j < B.n (checked all the same)
        if (bad_a) {
            d0 = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
            d1 = make_uint4(0u, 0u, kDistanceNone, (uint32_t)C2D_DISTANCE_BAD_PAIR << 8);
        } else if (key != kSetNoKey && j < B.n) {
            PolyObj a, b;
            poly_load(A, i, a);
            poly_load(B, j, b);
            uint4 s0 = make_uint4(0u, 0u, 0u, 0u), s1 = make_uint4(0u, kDistanceNone, 1u, 0u);   // the record of a hit pair
            if (!poly_collide(a, b)) distance_record<C2D_POLY_KMAX>(a.x, a.y, a.k, b.x, b.y, b.k, s0, s1);
            d0 = make_uint4(poly, s0.x, s0.y, s0.z);
            d1 = make_uint4(s0.w, s1.x, s1.y, s1.z);
        }
        reinterpret_cast<uint4*>(out)[2 * i] = d0;   // d_out is 16-byte aligned (checked on the host)
        reinterpret_cast<uint4*>(out)[2 * i + 1] = d1;
    }
}

template int set_best_launch_init<4>(c2d_ctx*, hipStream_t, size_t, void*);

int clearance_launch_finalise(c2d_ctx* ctx, hipStream_t s, const PolySetDev& A, const PolySetDev& B, size_t col_base, c2d_clearance* d_out)
{
    hipLaunchKernelGGL(clearance_finalise_kernel, dim3(grid_for(A.n, kSetBlock, 1 << 16)), dim3(kSetBlock), 0, s, A, B, col_base, d_out, ctx->d_async_err);
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_set_clearances(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, size_t row_base, size_t col_base, int flags, c2d_clearance* d_out,
                            c2d_stream stream)
{
    const char* what = "c2d_poly_set_clearances";
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!a || !b || !d_out) return cross_fail(ctx, what, "NULL argument");
    if (a->n == 0) return C2D_OK;
    PolySetDev A, B;
    if (int rc = poly_set_check(ctx, what, "a", a, A)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B, kEmptySetOk)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return cross_fail(ctx, what, "the output must be 16-byte aligned");
    if (flags & ~C2D_CLEARANCE_SKIP_SELF) return cross_fail(ctx, what, "unknown flag");
    if (int rc = cross_check_index_bases(ctx, what, A.n, B.n, row_base, col_base, "row_base + n_a and col_base + n_b must not exceed 2^32")) return rc;

    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    return set_best_run<4>(
        ctx, s, A.n, B.n, d_out,
        [&](unsigned blocks, size_t col_tiles, uint32_t strips) {
            hipLaunchKernelGGL(clearance_main_kernel, dim3(blocks), dim3(kSetBlock), 0, s, A, B, row_base, col_base, (flags & C2D_CLEARANCE_SKIP_SELF) ? 1 : 0,
                               col_tiles, strips, d_out, ctx->d_async_err);
            C2D_LAUNCH_CHECK(ctx);
            return (int)C2D_OK;
        },
        [&] { return clearance_launch_finalise(ctx, s, A, B, col_base, d_out); });
}

}  // extern "C"
