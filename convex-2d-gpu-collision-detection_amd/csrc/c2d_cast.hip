// c2d_cast.hip — shape casts for gfx950 (MI355X): for every polygon A_i of a set, moving over the step t = 0 .. 1, the polygon of a
// set B (moving too, or at rest) that it touches first, by the sweep contract, with the pair's whole sweep record
// (c2d_poly_set_casts; include/c2d.h "shape casts").  An N x M reduction: no N x M object is ever written.
//
// The rule (the contract of include/c2d.h).  S(i, j) is the c2d_sweep record of the pair (A_i, B_j) with the call's motion planes
// (c2d_sweep_rule.hpp and the exact polygon test).  Polygon j is considered when its vertex count is within 1..rows and, under
// C2D_CAST_SKIP_SELF, row_base + i != col_base + j.  The winner is the considered j with S(i, j).hit == 1 and the smallest
// (bits of S(i, j).toi, col_base + j); a hit's toi is t_in, never NaN, never -0 and at most 1, so the order of its bits is the order
// of its values, and equal times fall to the smaller index.
//
// The frame is c2d_set_best.hpp's (the mapping, the strips, the three launches).  A lane keeps of its query the padded vertices, the
// count, the motion and the centre of the vertex box; a tile stages per live edge {x0, y0, ex, ey} (the vertex and the edge vector),
// {mn, mx, nan0, off} (the polygon's OWN interval on that edge's normal, whether its first projection there is NaN, and the offset of
// the facing heuristic) and {ux, uy} (the outward unit normal: a heuristic that only chooses WHICH axis is walked first), and per
// polygon the count and the motion.  Every staged value the walk uses is made by the contract's own unfused operations.
// Per (lane, j), in order of j within the strip:
//   1. a lane whose best is toi = +0 does nothing more: no later j beats (+0, smaller j).  A wave of such lanes skips the tile.
//   2. one walk over the axes of the pairwise test yields sep, never, t_in and t_out by the contract's arithmetic (CastWalk below):
//      sep is the pairwise test's strict separation under the NaN rule of the first projections, so hit0 = !sep; per axis two
//      correctly rounded divisions.  All four are order-independent as VALUES — an OR, an OR, a maximum and a minimum under
//      compare-and-select, a NaN bound failing its compare — so the axes are visited in another order than the contract's: first
//      B_j's edge whose outward normal sees the query's box centre farthest out, then behind a wave-uniform branch B_j's edges
//      (intervals of A from registers, B_j's own staged), then A's (A turned by one slot per trip).
//   3. THE EXACT ABANDON.  t_in only grows and t_out only shrinks while axes are added, and sep and never only rise.  Once an axis
//      has set sep, the pair cannot win when `never`, when t_in > t_out, or when t_in >= the lane's best toi: the lane's best came
//      from a smaller j of the same strip, so an equal time loses too.  Such a lane is done with the pair, and the wave leaves the
//      walk when all its lanes are done.  The condition NEEDS sep: with a NaN first projection an axis can raise t_in without
//      separating, and the pair may still be hit0 with toi = 0.  Nothing else is skipped: there is no bound and no estimate here.
//   4. hit0, or a hit with t_in below the best, updates the lane's best.  Only the values hit and toi are carried: no axis, sign or
//      normal.
//
//   main      cast_main_kernel: the key's value is toi (no hit has the key of "nothing yet": toi <= 1)
//   finalise  cast_finalise_kernel, one lane per query: A_i and the winner in registers with their motions, the exact test and the
//             sweep record by the routines the sweep kernel uses, the whole record in three 8-byte stores
#include "c2d_cast_parts.hpp"   // the last launch, which c2d_cast_grid.hip shares; through it c2d_set_best.hpp
#include "c2d_sweep_rule.hpp"   // SweepPick; through it c2d_pair_list.hpp: PolySetDev, PolyObj, poly_load, poly_collide, poly_axes, the checks
#include "c2d_wave.hpp"

namespace c2d {

static_assert(sizeof(c2d_cast) == 24 && offsetof(c2d_cast, poly) == 0 && offsetof(c2d_cast, toi) == 4 && offsetof(c2d_cast, nx) == 8 &&
                  offsetof(c2d_cast, ny) == 12 && offsetof(c2d_cast, axis) == 16 && offsetof(c2d_cast, hit) == 18 && offsetof(c2d_cast, flags) == 19 &&
                  offsetof(c2d_cast, reserved0) == 20,
              "the kernels treat a cast as three pairs of dwords, (poly, toi) being the 64-bit key");

// What the main kernel keeps of one pair: the four values of the sweep rule that decide `hit` and `toi`.  add() is SweepPick::add
// without what the finalise pass recomputes (axis, sign, normal) and with the pairwise test's separation beside it; `live` masks an
// axis that the pair does not have.  [mna, mxa], [mnb, mxb]: the two projection intervals; ordered: neither first projection is NaN.
struct CastWalk {
    float rx, ry;   // the displacement of B relative to A
    float t_in = 0.0f, t_out = 1.0f;
    bool sep = false, never = false;
    C2D_DEV void add(bool live, float nx, float ny, float mna, float mxa, float mnb, float mxb, bool ordered)
    {
        sep |= live && ((mxa < mnb) || (mxb < mna)) && ordered;
        const float o1 = mxa - mnb, o2 = mxb - mna;
        const float v = nx * rx + ny * ry;
        const bool pos = v > 0.0f, neg = v < 0.0f;
        never |= live && v == 0.0f && (o1 < 0.0f || o2 < 0.0f);
        const float q1 = o1 / v, q2 = (-o2) / v;
        const float lo = pos ? q2 : q1, hi = pos ? q1 : q2;
        const bool enters = live && (pos || neg) && lo > t_in, leaves = live && (pos || neg) && hi < t_out;   // (a NaN bound fails its compare)
        t_in = enters ? lo : t_in;
        t_out = leaves ? hi : t_out;
    }
    // the exact abandon: separated at t = 0, and no hit before `best` whatever the remaining axes add
    C2D_DEV bool lost(float best) const { return sep && (never || t_in > t_out || t_in >= best); }
    C2D_DEV bool hit() const { return !never && t_in <= t_out; }
};

// Block b: row tile b / strips, strip b % strips of the col_tiles column tiles of B.
__global__ __launch_bounds__(kSetBlock) void cast_main_kernel(PolySetDev A, PolySetDev B, const float* __restrict__ a_dx, const float* __restrict__ a_dy,
                                                               const float* __restrict__ b_dx, const float* __restrict__ b_dy, size_t row_base, size_t col_base,
                                                               int skip_self, size_t col_tiles, uint32_t strips, c2d_cast* __restrict__ out,
                                                               uint32_t* __restrict__ async_err)
{
    __shared__ __attribute__((aligned(16))) float4 s_edge[kSetCols][kSetK];   // 16 KiB: {x0, y0, ex, ey} of every live edge
    __shared__ __attribute__((aligned(16))) float4 s_own[kSetCols][kSetK];    // 16 KiB: {mn, mx, nan0 (1 or 0), off}
    __shared__ __attribute__((aligned(8))) float2 s_face[kSetCols][kSetK];    //  8 KiB: {ux, uy}
    __shared__ float2 s_move[kSetCols];                                         // the polygon's (dx, dy)
    __shared__ int s_k[kSetCols];   // the count; 0: not considered by any query (out of range, or beyond n)
    const uint32_t lane = threadIdx.x;
    const float inf = __builtin_inff();

    // (the same text, up to what this query adds, in c2d_clearance.hip; spelt out in both: c2d_set_best.hpp says why)
    // ---- the lane's query: count, padded vertices, motion, the centre of the vertex box ---------------------------------------
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
    float adx = 0.0f, ady = 0.0f;
    if (row_live && a_dx) {   // (both planes or neither: checked on the host)
        adx = a_dx[i];
        ady = a_dy[i];
    }
    float xlo = ax[0], xhi = ax[0], ylo = ay[0], yhi = ay[0];
#pragma unroll
    for (int r = 1; r < kSetK; r++) {
        const bool used = r < ka;
        ax[r] = used ? ax[r] : ax[0];   // neutral padding: a repeated vertex adds a zero-length edge and repeats a projection
        ay[r] = used ? ay[r] : ay[0];
        xlo = __builtin_fminf(xlo, ax[r]);
        xhi = __builtin_fmaxf(xhi, ax[r]);
        ylo = __builtin_fminf(ylo, ay[r]);
        yhi = __builtin_fmaxf(yhi, ay[r]);
    }
    const float cax = 0.5f * xlo + 0.5f * xhi, cay = 0.5f * ylo + 0.5f * yhi;   // (heuristic only)
    const float ax0 = ax[0], ay0 = ay[0];   // vertex 0, whichever way the polygon is turned
    const size_t gi = row_base + i;

    // (the strip, the tile loop and the staging of the frame, spelt out in each of the three main kernels: c2d_set_best.hpp says why)
    size_t tile0, tiles;
    ray_strip_tiles(col_tiles, (size_t)strips, (size_t)(blockIdx.x % strips), tile0, tiles);

    float best = inf;   // the toi of the lane's best so far; +inf: none yet (a hit's toi is at most 1)
    uint32_t best_j = 0;
#pragma unroll 1
    for (size_t tile = tile0; tile < tile0 + tiles; tile++) {
        const size_t j0 = tile * (size_t)kSetCols;
        const uint32_t nj = (uint32_t)(B.n - j0 < (size_t)kSetCols ? B.n - j0 : (size_t)kSetCols);
        __syncthreads();   // the previous tile's readers are done
        // ---- stage 64 polygons: vertices and edge vectors, the count, the motion ---------------------------------------------------
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
                float2 mv = make_float2(0.0f, 0.0f);
                if (k > 0 && b_dx) mv = make_float2(b_dx[j], b_dy[j]);   // k > 0: c < nj, so j < B.n
                s_move[c] = mv;
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
        // (the own interval, the NaN bit and the outward sign are the same text in c2d_clearance.hip; spelt out in both: c2d_set_best.hpp)
        // ---- hoist: lane (polygon c, edge a) -> the own interval on the edge's normal, its NaN bit and the facing heuristic ----------
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
                // outward: away from the side the polygon's own projections extend to (heuristic only; fast arithmetic)
                const float pa = nx * ed.x + ny * ed.y;
                const float sg = (mx - pa) > (pa - mn) ? -1.0f : 1.0f;
                const float inv = sg * __builtin_amdgcn_rsqf(ed.z * ed.z + ed.w * ed.w);
                s_own[c][a] = make_float4(mn, mx, nan0 ? 1.0f : 0.0f, pa * inv);
                s_face[c][a] = make_float2(nx * inv, ny * inv);
            }
        }
        __syncthreads();
        // ---- the pairs ------------------------------------------------------------------------------------------------------------
        if (__ballot(row_live && best != 0.0f) == 0ull) continue;   // (wave-uniform) a wave of finished lanes skips the tile
#pragma unroll 1
        for (uint32_t c = 0; c < nj; c++) {
            const int k = __builtin_amdgcn_readfirstlane(s_k[c]);
            if (k == 0) continue;   // (wave-uniform) a count out of range: not considered
            const size_t gj = col_base + j0 + c;
            const bool considered = row_live && best != 0.0f && !(skip_self && gi == gj);
            if (__ballot(considered) == 0ull) continue;   // (wave-uniform)
            const float2 mv = s_move[c];
            CastWalk w{mv.x - adx, mv.y - ady};
            // (the pick below is the same text in c2d_clearance.hip, over another staged layout; spelt out in both: c2d_set_best.hpp)
            // the first axis: the edge of B_j whose outward normal sees the query's box centre farthest out
            uint32_t fe = 0;
            {
                float fs = -inf;
#pragma unroll 1
                for (int e = 0; e < k; e++) {
                    const float2 f = s_face[c][e];   // (one address for the wave: a broadcast)
                    const float sc = fma_(f.x, cax, fma_(f.y, cay, -s_own[c][e].w));
                    const bool better = sc > fs;
                    fs = better ? sc : fs;
                    fe = better ? (uint32_t)e : fe;
                }
            }
            {
                const float4 ed = s_edge[c][fe], own = s_own[c][fe];
                const float nx = -ed.w, ny = ed.z;
                float mn = inf, mx = -inf;
#pragma unroll
                for (int r = 0; r < kSetK; r++)
                    if (r < kmax_a) poly_minmax(nx, ny, ax[r], ay[r], mn, mx);
                w.add(true, nx, ny, mn, mx, own.x, own.y, own.z == 0.0f && !__builtin_isnan(nx * ax0 + ny * ay0));
            }
            if (__ballot(considered && !w.lost(best)) != 0ull) {   // (wave-uniform) some pair is still open: the other axes
                // B_j's edges (the first axis comes by again: every value is idempotent)
                bool open = true;
#pragma unroll 1
                for (int eb = 0; eb < k && open; eb++) {
                    const float4 ed = s_edge[c][eb], own = s_own[c][eb];
                    const float nx = -ed.w, ny = ed.z;
                    float mn = inf, mx = -inf;
#pragma unroll
                    for (int r = 0; r < kSetK; r++)
                        if (r < kmax_a) poly_minmax(nx, ny, ax[r], ay[r], mn, mx);
                    w.add(true, nx, ny, mn, mx, own.x, own.y, own.z == 0.0f && !__builtin_isnan(nx * ax0 + ny * ay0));
                    open = __ballot(considered && !w.lost(best)) != 0ull;   // (wave-uniform)
                }
                // A's axes: always the one from slot 0 to slot 1, A turned by one slot per trip and back in place after 16 (the loop
                // stays rolled and nothing of an edge is kept across pairs); slot ka is vertex 0 again, so the polygon closes itself.
                // Once the wave is done the trips only turn.
                if (open) {   // (wave-uniform)
#pragma unroll 1
                    for (int a = 0; a < kSetK; a++) {
                        if (a < kmax_a && open) {   // (wave-uniform) beyond kmax_a every lane's axis is padding
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
                            w.add(a < ka, nx, ny, mnp, mxp, mnq, mxq, first_projections_ordered(nx * ax0 + ny * ay0, nx * v0.x + ny * v0.y));
                            open = __ballot(considered && !w.lost(best)) != 0ull;   // (wave-uniform)
                        }
                        set_best_turn(ax, ay);
                    }
                }
            }
            // step 4.  (A lane that was done before the last axis stays done: sep and never only rise, t_in only grows, t_out only
            // shrinks, so the test below fails for it whatever the later axes added.)
            const bool hit0 = !w.sep;
            const float toi = hit0 ? 0.0f : w.t_in;
            const bool take = considered && (hit0 || (w.hit() && toi < best));   // strict: the first of equal times stays
            best = take ? toi : best;
            best_j = take ? (uint32_t)(j0 + c) : best_j;
        }
    }
    if (best != inf) set_best_publish(__float_as_uint(best), (uint32_t)col_base, best_j, out, i);
}

// (The wave-trip loop, the bad-count report, the key decode and the two loads are the same text in c2d_clearance.hip; spelt out in both,
// because as one routine or kernel template they changed this kernel's code: c2d_set_best.hpp.)
// One lane per query: the record of the key's polygon by the routines of the sweep kernel (the key holds col_base + j).
__global__ __launch_bounds__(kSetBlock) void cast_finalise_kernel(PolySetDev A, PolySetDev B, const float* __restrict__ a_dx, const float* __restrict__ a_dy,
                                                                   const float* __restrict__ b_dx, const float* __restrict__ b_dy, size_t col_base,
                                                                   c2d_cast* __restrict__ out, uint32_t* __restrict__ async_err)
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
        const unsigned long long key = reinterpret_cast<const unsigned long long*>(out)[3 * i];
        uint32_t poly = 0xFFFFFFFFu;
        uint4 s = make_uint4(__float_as_uint(__builtin_inff()), 0u, 0u, kSweepNoAxis);   // no considered polygon is hit
        const size_t j = (size_t)(uint32_t)((uint32_t)key - (uint32_t)col_base);   // the main pass wrote it: j < B.n (checked all the same)
        if (bad_a) {
            s = make_uint4(0u, 0u, 0u, kSweepNoAxis | ((uint32_t)C2D_SWEEP_BAD_PAIR << 24));
        } else if (key != kSetNoKey && j < B.n) {
            PolyObj a, b;
            poly_load(A, i, a);
            poly_load(B, j, b);
            const float rx = (b_dx ? b_dx[j] : 0.0f) - (a_dx ? a_dx[i] : 0.0f), ry = (b_dx ? b_dy[j] : 0.0f) - (a_dx ? a_dy[i] : 0.0f);
            poly = (uint32_t)key;
            s = make_uint4(0u, 0u, 0u, kSweepNoAxis | (1u << 16) | ((uint32_t)C2D_SWEEP_START_OVERLAP << 24));   // the record of a pair that starts in overlap
            if (!poly_collide(a, b)) {
                SweepPick pick{rx, ry};
                (void)poly_axes(a, b, pick);
                s = pick.record();
            }
        }
        uint2* o = reinterpret_cast<uint2*>(out) + 3 * i;   // d_out is 8-byte aligned (checked on the host)
        o[0] = make_uint2(poly, s.x);
        o[1] = make_uint2(s.y, s.z);
        o[2] = make_uint2(s.w, 0u);
    }
}

template int set_best_launch_init<3>(c2d_ctx*, hipStream_t, size_t, void*);

int cast_launch_finalise(c2d_ctx* ctx, hipStream_t s, const PolySetDev& A, const PolySetDev& B, const float* d_a_dx, const float* d_a_dy,
                         const float* d_b_dx, const float* d_b_dy, size_t col_base, c2d_cast* d_out)
{
    hipLaunchKernelGGL(cast_finalise_kernel, dim3(grid_for(A.n, kSetBlock, 1 << 16)), dim3(kSetBlock), 0, s, A, B, d_a_dx, d_a_dy, d_b_dx, d_b_dy,
                       col_base, d_out, ctx->d_async_err);
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_set_casts(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, const float* d_a_dx, const float* d_a_dy, const float* d_b_dx,
                       const float* d_b_dy, size_t row_base, size_t col_base, int flags, c2d_cast* d_out, c2d_stream stream)
{
    const char* what = "c2d_poly_set_casts";
    if (int rc = sweep_motion_check(ctx, what, d_a_dx, d_a_dy, d_b_dx, d_b_dy)) return rc;   // (a missing ctx too)
    if (!a || !b || !d_out) return cross_fail(ctx, what, "NULL argument");
    if (a->n == 0) return C2D_OK;
    PolySetDev A, B;
    if (int rc = poly_set_check(ctx, what, "a", a, A)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B, kEmptySetOk)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) return cross_fail(ctx, what, "the output must be 8-byte aligned");
    if (flags & ~C2D_CAST_SKIP_SELF) return cross_fail(ctx, what, "unknown flag");
    if (int rc = cross_check_index_bases(ctx, what, A.n, B.n, row_base, col_base, "row_base + n_a and col_base + n_b must not exceed 2^32")) return rc;

    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    return set_best_run<3>(
        ctx, s, A.n, B.n, d_out,
        [&](unsigned blocks, size_t col_tiles, uint32_t strips) {
            hipLaunchKernelGGL(cast_main_kernel, dim3(blocks), dim3(kSetBlock), 0, s, A, B, d_a_dx, d_a_dy, d_b_dx, d_b_dy, row_base, col_base,
                               (flags & C2D_CAST_SKIP_SELF) ? 1 : 0, col_tiles, strips, d_out, ctx->d_async_err);
            C2D_LAUNCH_CHECK(ctx);
            return (int)C2D_OK;
        },
        [&] { return cast_launch_finalise(ctx, s, A, B, d_a_dx, d_a_dy, d_b_dx, d_b_dy, col_base, d_out); });
}

}  // extern "C"
