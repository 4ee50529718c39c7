// c2d_pair_list.hpp — what the list-driven queries share (c2d_contact.hip: contacts and manifolds; c2d_distance.hip: distances;
// c2d_sweep.hip: sweeps): one pair of a device-resident list per lane.  It owns, each stated once:
//   the axis walk      every axis of the pairwise test with its two projection intervals, to a pick (contacts, manifolds, sweeps)
//   the shapes         the two forms a set comes in (polygons, rectangle planes) with their pairwise test and walk, and either in motion
//   the kernel frame   the bound read on the device, bad pairs and the error word, the substitution that keeps every lane of a wave on
//                      loadable indices, and the row-uniform load of A; and the one __global__ kernel around it
//   the host front end the checks every such entry point states (include/c2d.h, "contact queries"), in the order the header promises
// A query's own file keeps its rule: the pick or the record, its W for the frame, and its entry points.
#pragma once

#include <initializer_list>

#include "c2d_cross.hpp"
#include "c2d_math.hpp"
#include "c2d_poly_pair.hpp"

namespace c2d {

constexpr int kPairListBlock = 256;
constexpr int kPairListMaxGrid = 1 << 16;   // blocks per launch; the frame grid-strides beyond it

// ---- the axis walk -----------------------------------------------------------------------------------------------------------------
// Every axis of the pairwise test in axis order, with its two projection intervals, to pick.add(axis, nx, ny, maxA - minB, maxB - minA);
// returns the pairwise boolean (a caller that drops it pays nothing for it).  Every vertex index is a compile-time slot: the lanes of
// a wave hold unrelated pairs.

// poly_collide (c2d_poly_pair.hpp) with the intervals kept: axes 0 .. ka - 1 are A's edges, ka .. ka + kb - 1 are B's.
template <class Pick>
C2D_DEV bool poly_axes(const PolyObj& A, const PolyObj& B, Pick& pick)
{
    const float inf = __builtin_inff();
    PolyObj P = A, Q = B;
    bool sep = false;
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
        const uint32_t base = side ? (uint32_t)A.k : 0u;
#pragma unroll
        for (int a = 0; a < C2D_POLY_KMAX; a++) {
            if (a < P.k) {   // axes >= P.k come from padding (zero vectors): they never separate and are out of the pick
                const int a1 = (a + 1) & (C2D_POLY_KMAX - 1);
                const float nx = -(P.y[a1] - P.y[a]), ny = P.x[a1] - P.x[a];
                float mnp = inf, mxp = -inf, mnq = inf, mxq = -inf;
#pragma unroll
                for (int r = 0; r < C2D_POLY_KMAX; r++) {
                    poly_minmax(nx, ny, P.x[r], P.y[r], mnp, mxp);
                    poly_minmax(nx, ny, Q.x[r], Q.y[r], mnq, mxq);
                }
                sep |= ((mxp < mnq) || (mxq < mnp)) && first_projections_ordered(nx * P.x[0] + ny * P.y[0], nx * Q.x[0] + ny * Q.y[0]);
                const float u = mxp - mnq, v = mxq - mnp;   // side 0: P is A, so u = maxA - minB; side 1: P is B, so v is
                pick.add(base + (uint32_t)a, nx, ny, side ? v : u, side ? u : v);
            }
        }
        const PolyObj t = P;
        P = Q;
        Q = t;
    }
    return !sep;
}

// rect_collide (c2d_math.hpp) with the intervals kept: axes 0 .. 3 are the edge vectors of rectangle 1, 4 .. 7 those of rectangle 2.
template <class Pick>
C2D_DEV bool rect_axes(const float (&r1)[8], const float (&r2)[8], Pick& pick)
{
    bool sep = false;
#pragma unroll
    for (int which = 0; which < 2; which++) {
        const float (&r)[8] = which == 0 ? r1 : r2;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float ax = r[(2 * i + 2) & 7] - r[2 * i], ay = r[(2 * i + 3) & 7] - r[2 * i + 1];
            const float p10 = dot2(ax, r1[0], ay, r1[1]), p11 = dot2(ax, r1[2], ay, r1[3]);
            const float p12 = dot2(ax, r1[4], ay, r1[5]), p13 = dot2(ax, r1[6], ay, r1[7]);
            const float p20 = dot2(ax, r2[0], ay, r2[1]), p21 = dot2(ax, r2[2], ay, r2[3]);
            const float p22 = dot2(ax, r2[4], ay, r2[5]), p23 = dot2(ax, r2[6], ay, r2[7]);
            const float min1 = min4(p10, p11, p12, p13), max1 = max4(p10, p11, p12, p13);
            const float min2 = min4(p20, p21, p22, p23), max2 = max4(p20, p21, p22, p23);
            sep |= ((max1 < min2) || (max2 < min1)) && first_projections_ordered(p10, p20);
            pick.add((uint32_t)(4 * which + i), ax, ay, max1 - min2, max2 - min1);
        }
    }
    return !sep;
}

// ---- the shapes -----------------------------------------------------------------------------------------------------------------
//   S::Set                 the device-side description of one set (a kernel argument);  S::size(set): its objects
//   S::present(set, i)     false: object i is in no pair (a polygon with a vertex count outside 1..rows)
//   S::load(set, i, obj)   object i in registers: what the frame calls
//   S::vertices(...)       a list shape's load, under the name a shape with more per object builds its own load on.  (Not on the
//                          base's load: every level is inlined, and still one more call around poly_load turns two address
//                          computations of the polygon kernels the other way round; profiles/pair_list_refactor_isa.txt holds them
//                          to the code they had.)
//   S::collide(a, b)       the pairwise boolean of the pair
//   S::axes(a, b, pick)    the axis walk of the pair to `pick`; returns the pairwise boolean
struct PolyListShape {
    using Set = PolySetDev;
    using Obj = PolyObj;
    static constexpr uint32_t kAbsentErr = C2D_ASYNC_ERR_POLY_K;
    static __host__ __device__ size_t size(const Set& X) { return X.n; }
    static C2D_DEV bool present(const Set& X, size_t i)
    {
        int k;
        return poly_count(X, i, k);
    }
    static constexpr auto& vertices = poly_load;
    static C2D_DEV void load(const Set& X, size_t i, Obj& o) { vertices(X, i, o); }
    static C2D_DEV bool collide(const Obj& a, const Obj& b) { return poly_collide(a, b); }
    template <class Pick>
    static C2D_DEV bool axes(const Obj& a, const Obj& b, Pick& pick) { return poly_axes(a, b, pick); }
};

struct RectListSet {
    const float* p[8];
    size_t n;
};

struct RectListShape {
    using Set = RectListSet;
    struct Obj { float r[8]; };
    static constexpr uint32_t kAbsentErr = 0u;
    static __host__ __device__ size_t size(const Set& X) { return X.n; }
    static C2D_DEV bool present(const Set&, size_t) { return true; }
    static C2D_DEV void vertices(const Set& X, size_t i, Obj& o)
    {
#pragma unroll
        for (int k = 0; k < 8; k++) o.r[k] = X.p[k][i];
    }
    static C2D_DEV void load(const Set& X, size_t i, Obj& o) { vertices(X, i, o); }
    static C2D_DEV bool collide(const Obj& a, const Obj& b) { return rect_collide(a.r, b.r); }
    template <class Pick>
    static C2D_DEV bool axes(const Obj& a, const Obj& b, Pick& pick) { return rect_axes(a.r, b.r, pick); }
};

// A list shape in linear motion over one step: Set is the base set plus the two displacement planes, Obj the base object plus its
// displacement, loaded next to its vertices.  kAbsentErr, collide and axes are the base's (an Obj is a base object).
template <class Base>
struct MovingShape : Base {
    struct Set {
        typename Base::Set s;
        const float *dx, *dy;   // both nullptr: the set stands still
    };
    struct Obj : Base::Obj {
        float dx, dy;
    };
    static __host__ __device__ size_t size(const Set& X) { return Base::size(X.s); }
    static C2D_DEV bool present(const Set& X, size_t i) { return Base::present(X.s, i); }
    static C2D_DEV void load(const Set& X, size_t i, Obj& o)
    {
        Base::vertices(X.s, i, o);
        o.dx = X.dx ? X.dx[i] : 0.0f;
        o.dy = X.dx ? X.dy[i] : 0.0f;
    }
};

// ---- the kernel frame -----------------------------------------------------------------------------------------------------------
// One pair per lane, blocks of kPairListBlock.  Entry p of the list is processed when p < min(n_pairs, *d_n); no other record is
// touched.  A pair with an index outside its set, or with an absent object, reads no vertex and keeps the record W starts with.
// W is the query: a default-constructed W holds the BAD_PAIR record; w.pair(a, b, valid) is called by whole waves that have at least
// one valid lane (wave-uniform: it may ballot) and keeps its result only where `valid`; w.store(p, out...) writes entry p.
template <class S, class W, class... Out>
C2D_DEV void listed_pairs(const typename S::Set& A, const typename S::Set& B, const uint32_t* __restrict__ pairs, size_t n_pairs,
                          const unsigned long long* __restrict__ d_n, size_t row_base, size_t col_base, uint32_t* __restrict__ async_err, Out... out)
{
    size_t bound = n_pairs;
    if (d_n) {
        const unsigned long long listed = *d_n;
        if (listed < (unsigned long long)bound) bound = (size_t)listed;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const size_t n_a = S::size(A), n_b = S::size(B);
    const size_t step = (size_t)gridDim.x * kPairListBlock;
    // every lane of a wave makes the same trips (the loop variable is the wave's first entry): the ballots below see whole waves
    for (size_t p0 = (size_t)blockIdx.x * kPairListBlock + (threadIdx.x & ~63u); p0 < bound; p0 += step) {
        const size_t p = p0 + lane;
        const bool in = p < bound;
        uint32_t gi = 0, gj = 0;
        if (in) {
            gi = pairs[2 * p];
            gj = pairs[2 * p + 1];
        }
        // local indices; one below its base wraps to far above any n (n and the bases stay below 2^62)
        const size_t i = (size_t)gi - row_base, j = (size_t)gj - col_base;
        const bool ranged = in && i < n_a && j < n_b;
        bool valid = false;
        if (ranged) valid = S::present(A, i) && S::present(B, j);   // (the count planes are read inside the sets only)
        const unsigned long long bad_index = __ballot(in && !ranged), absent = __ballot(ranged && !valid);
        if (lane == 0) {
            const uint32_t e = (bad_index ? C2D_ASYNC_ERR_PAIR_INDEX : 0u) | (absent ? S::kAbsentErr : 0u);
            if (e) __hip_atomic_fetch_or(async_err, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        W w;
        const unsigned long long vm = __ballot(valid);
        if (vm != 0ull) {   // (wave-uniform)
            // Lanes without a valid pair compute the first valid lane's pair and drop the result: every index used below is inside
            // its set, and no branch of the pair routine depends on who is valid.  i, j < 2^32 for a valid pair (gi, gj are u32).
            const int first = (int)__builtin_ctzll(vm);
            const uint32_t i0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)i, first);
            const uint32_t j0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)j, first);
            const uint32_t ia = valid ? (uint32_t)i : i0, jb = valid ? (uint32_t)j : j0;
            typename S::Obj a, b;
            if (__ballot(ia != i0) == 0ull)
                S::load(A, (size_t)i0, a);   // the whole wave is in one row: one wave-uniform index
            else
                S::load(A, (size_t)ia, a);
            S::load(B, (size_t)jb, b);
            w.pair(a, b, valid);
        }
        if (in) w.store(p, out...);
    }
}

// The kernel of query W on shape S: the arguments of every list-driven kernel, in their one order (the outputs in front of the error word).
template <class S, class W, class... Out>
__global__ __launch_bounds__(kPairListBlock) void pair_list_kernel(typename S::Set A, typename S::Set B, const uint32_t* __restrict__ pairs, size_t n_pairs,
                                                                   const unsigned long long* __restrict__ d_n, size_t row_base, size_t col_base,
                                                                   Out* __restrict__... out, uint32_t* __restrict__ async_err)
{
    listed_pairs<S, W>(A, B, pairs, n_pairs, d_n, row_base, col_base, async_err, out...);
}

// ---- the host front end ---------------------------------------------------------------------------------------------------------
// The list, its count, the bases and the outputs (each required and 16-byte aligned), as every list-driven entry point states them.
inline int pair_list_check(c2d_ctx* ctx, const char* what, size_t n_a, size_t n_b, const uint32_t* d_pairs, size_t n_pairs,
                           const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, std::initializer_list<const void*> outs)
{
    if (int rc = cross_check_flags_bases(ctx, what, n_a, n_b, row_base, col_base, 0)) return rc;
    if (!d_pairs) return cross_fail(ctx, what, "NULL pair list");
    uintptr_t bits = 0;
    for (const void* o : outs) {
        if (!o) return cross_fail(ctx, what, "NULL output");
        bits |= reinterpret_cast<uintptr_t>(o);
    }
    if (reinterpret_cast<uintptr_t>(d_pairs) & 3u) return cross_fail(ctx, what, "the pair list must be 4-byte aligned");
    if (bits & 15u) return cross_fail(ctx, what, outs.size() > 1 ? "both outputs must be 16-byte aligned" : "the output must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_n_pairs) & 7u) return cross_fail(ctx, what, "d_n_pairs must be 8-byte aligned");
    if (n_pairs > kBaseLimit) return cross_fail(ctx, what, "n_pairs must stay below 2^62");
    return C2D_OK;
}

// A polygon entry point: the checks in the order the header promises them, then launch(A, B, grid) under the ctx's device.
template <class Launch>
int poly_pair_list_call(c2d_ctx* ctx, const char* what, const c2d_poly_set* a, const c2d_poly_set* b, const uint32_t* d_pairs, size_t n_pairs,
                        const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, std::initializer_list<const void*> outs, Launch&& launch)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!a || !b) return cross_fail(ctx, what, "NULL set");
    if (n_pairs == 0) return C2D_OK;
    PolySetDev A, B;
    if (int rc = poly_set_check(ctx, what, "a", a, A)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B)) return rc;
    if (int rc = pair_list_check(ctx, what, A.n, B.n, d_pairs, n_pairs, d_n_pairs, row_base, col_base, outs)) return rc;
    DeviceGuard dg(ctx->device);
    launch(A, B, grid_for(n_pairs, kPairListBlock, kPairListMaxGrid));
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}

// The same for two rectangle sets given as 8 vertex planes each.
template <class Launch>
int rect_pair_list_call(c2d_ctx* ctx, const char* what, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b,
                        const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs, size_t row_base, size_t col_base,
                        std::initializer_list<const void*> outs, Launch&& launch)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!d_a || !d_b) return cross_fail(ctx, what, "NULL argument");
    if (n_pairs == 0) return C2D_OK;
    RectListSet A, B;
    A.n = n_a;
    B.n = n_b;
    for (int k = 0; k < 8; k++) {
        if (!d_a[k] || !d_b[k]) return cross_fail(ctx, what, "NULL plane");
        if ((reinterpret_cast<uintptr_t>(d_a[k]) | reinterpret_cast<uintptr_t>(d_b[k])) & 3u) return cross_fail(ctx, what, "planes must be 4-byte aligned");
        A.p[k] = d_a[k];
        B.p[k] = d_b[k];
    }
    if (int rc = pair_list_check(ctx, what, n_a, n_b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, outs)) return rc;
    DeviceGuard dg(ctx->device);
    launch(A, B, grid_for(n_pairs, kPairListBlock, kPairListMaxGrid));
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}

}  // namespace c2d
