// c2d_sweep.hip — swept queries for gfx950 (MI355X): for each listed pair (A_i, B_j), both in linear motion over the step t = 0 .. 1,
// whether the two shapes touch during the step, the first time at which they do and the unit normal from A to B at that touch
// (c2d_poly_pair_sweeps, c2d_rect_pair_sweeps; include/c2d.h "swept queries").
//
// The rule (the contract of include/c2d.h).  A pair that the pairwise test reports at t = 0 starts in overlap and is done.  Otherwise,
// with r = (b_dx - a_dx, b_dy - a_dy) the displacement of B relative to A, per axis n of the pairwise test in axis order, with
// [minA, maxA] and [minB, maxB] the projection intervals of the contact rule, everything binary32 and unfused:
//     o1 = maxA - minB,  o2 = maxB - minA,  v = n.x * r.x + n.y * r.y
//     v > 0: lo = (-o2) / v, hi = o1 / v;   v < 0: lo = o1 / v, hi = (-o2) / v;   v == 0: `never` when o1 < 0 || o2 < 0;   NaN v: ignored
//     lo > t_in replaces t_in (from +0) with its axis and the sign of v;  hi < t_out replaces t_out (from 1)
//     hit = !never && t_in <= t_out,  toi = t_in,  normal = -+ n / sqrt(n.x * n.x + n.y * n.y) with + when v < 0.
// One pair per lane on the frame of c2d_pair_list.hpp: the motion of an object rides in its shape and is loaded next to its
// vertices, so the frame's first-valid-lane substitution keeps those loads on valid indices as well.  The axis walk is the contact
// kernel's (compile-time vertex slots, one unrolled body per side with the polygons exchanged, axes at or beyond k masked out); the
// pick carries the winner's raw axis and sign, and the square root and the two normal divisions are paid once, after the walk.
// The two quotients per axis are the contract's own correctly rounded divisions: there is no estimate pass here.
#include "c2d_pair_list.hpp"

namespace c2d {

static_assert(sizeof(c2d_sweep) == 16 && offsetof(c2d_sweep, nx) == 4 && offsetof(c2d_sweep, ny) == 8 && offsetof(c2d_sweep, axis) == 12 &&
                  offsetof(c2d_sweep, hit) == 14 && offsetof(c2d_sweep, flags) == 15,
              "the kernel stores a sweep as four dwords");

constexpr uint32_t kSweepNoAxis = 0xFFFFu;

// The sequential pick of one pair.  add() takes the live axes in axis order.
struct SweepPick {
    float rx, ry;                                      // the displacement of B relative to A
    float t_in = 0.0f, t_out = 1.0f, nx = 0.0f, ny = 0.0f;   // (nx, ny): the raw axis of t_in
    uint32_t axis = kSweepNoAxis;
    bool closing = false, never = false;               // closing: v < 0 on the axis of t_in
    C2D_DEV void add(uint32_t axis_, float nx_, float ny_, float o1, float o2)
    {
        const float v = nx_ * rx + ny_ * ry;
        const bool pos = v > 0.0f, neg = v < 0.0f;
        never |= v == 0.0f && (o1 < 0.0f || o2 < 0.0f);
        const float q1 = o1 / v, q2 = (-o2) / v;
        const float lo = pos ? q2 : q1, hi = pos ? q1 : q2;
        const bool enters = (pos || neg) && lo > t_in, leaves = (pos || neg) && hi < t_out;   // (a NaN bound fails its compare)
        t_in = enters ? lo : t_in;
        nx = enters ? nx_ : nx;
        ny = enters ? ny_ : ny;
        axis = enters ? axis_ : axis;
        closing = enters ? neg : closing;
        t_out = leaves ? hi : t_out;
    }
    // the record of a pair that does not start in overlap: {toi, nx, ny, axis | hit << 16 | flags << 24}
    C2D_DEV uint4 record() const
    {
        if (never || !(t_in <= t_out)) return make_uint4(__float_as_uint(__builtin_inff()), 0u, 0u, kSweepNoAxis);
        if (axis == kSweepNoAxis) return make_uint4(__float_as_uint(t_in), 0u, 0u, kSweepNoAxis | (1u << 16));
        const float len = __builtin_sqrtf(nx * nx + ny * ny);
        const float ux = nx / len, uy = ny / len;
        return make_uint4(__float_as_uint(t_in), __float_as_uint(closing ? ux : -ux), __float_as_uint(closing ? uy : -uy), axis | (1u << 16));
    }
};

// poly_collide (c2d_poly_pair.hpp) with the intervals kept, as the contact kernel walks it: axes 0 .. ka - 1 are A's edges,
// ka .. ka + kb - 1 are B's.
C2D_DEV void poly_sweep_axes(const PolyObj& A, const PolyObj& B, SweepPick& pick)
{
    const float inf = __builtin_inff();
    PolyObj P = A, Q = B;
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
        const uint32_t base = side ? (uint32_t)A.k : 0u;
#pragma unroll
        for (int a = 0; a < C2D_POLY_KMAX; a++) {
            if (a < P.k) {   // axes >= P.k come from padding: out of the pick
                const int a1 = (a + 1) & (C2D_POLY_KMAX - 1);
                const float nx = -(P.y[a1] - P.y[a]), ny = P.x[a1] - P.x[a];
                float mnp = inf, mxp = -inf, mnq = inf, mxq = -inf;
#pragma unroll
                for (int r = 0; r < C2D_POLY_KMAX; r++) {
                    poly_minmax(nx, ny, P.x[r], P.y[r], mnp, mxp);
                    poly_minmax(nx, ny, Q.x[r], Q.y[r], mnq, mxq);
                }
                const float u = mxp - mnq, w = mxq - mnp;   // side 0: P is A, so u = maxA - minB; side 1: P is B, so w is
                pick.add(base + (uint32_t)a, nx, ny, side ? w : u, side ? u : w);
            }
        }
        const PolyObj t = P;
        P = Q;
        Q = t;
    }
}

// rect_collide (c2d_math.hpp) with the intervals kept: axes 0 .. 3 are the edge vectors of rectangle 1, 4 .. 7 those of rectangle 2.
C2D_DEV void rect_sweep_axes(const float (&r1)[8], const float (&r2)[8], SweepPick& pick)
{
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
            pick.add((uint32_t)(4 * which + i), ax, ay, max1 - min2, max2 - min1);
        }
    }
}

// Every coordinate below 2^60 in magnitude (a NaN is not): every axis component is then below 2^61 and every projection below 2^122,
// so with r = 0 every v is an exact zero and o1 < 0 || o2 < 0 says exactly what the pairwise test's strict compares say.
template <int N>
C2D_DEV bool sweep_bounded(const float (&c)[N])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; k++) ok &= __builtin_fabsf(c[k]) < 0x1p60f;
    return ok;
}

// ---- the shapes: those of c2d_pair_list.hpp with the motion of each object next to its vertices ------------------------------------
//   S::collide(a, b)       the pairwise boolean of the pair at t = 0
//   S::bounded(a, b)       sweep_bounded of every coordinate of the pair
//   S::axes(a, b, pick)    the live axes of the pairwise test, with their two intervals, to `pick`
struct PolySweepShape {
    struct Set {
        PolySetDev s;
        const float *dx, *dy;   // both nullptr: the set stands still
    };
    struct Obj {
        PolyObj p;
        float dx, dy;
    };
    static constexpr uint32_t kAbsentErr = PolyListShape::kAbsentErr;
    static __host__ __device__ size_t size(const Set& X) { return X.s.n; }
    static C2D_DEV bool present(const Set& X, size_t i) { return PolyListShape::present(X.s, i); }
    static C2D_DEV void load(const Set& X, size_t i, Obj& o)
    {
        poly_load(X.s, i, o.p);
        o.dx = X.dx ? X.dx[i] : 0.0f;
        o.dy = X.dx ? X.dy[i] : 0.0f;
    }
    static C2D_DEV bool collide(const Obj& a, const Obj& b) { return poly_collide(a.p, b.p); }
    static C2D_DEV bool bounded(const Obj& a, const Obj& b) { return sweep_bounded(a.p.x) && sweep_bounded(a.p.y) && sweep_bounded(b.p.x) && sweep_bounded(b.p.y); }
    static C2D_DEV void axes(const Obj& a, const Obj& b, SweepPick& pick) { poly_sweep_axes(a.p, b.p, pick); }
};

struct RectSweepShape {
    struct Set {
        RectListSet s;
        const float *dx, *dy;
    };
    struct Obj {
        float r[8];
        float dx, dy;
    };
    static constexpr uint32_t kAbsentErr = RectListShape::kAbsentErr;
    static __host__ __device__ size_t size(const Set& X) { return X.s.n; }
    static C2D_DEV bool present(const Set&, size_t) { return true; }
    static C2D_DEV void load(const Set& X, size_t i, Obj& o)
    {
#pragma unroll
        for (int k = 0; k < 8; k++) o.r[k] = X.s.p[k][i];
        o.dx = X.dx ? X.dx[i] : 0.0f;
        o.dy = X.dx ? X.dy[i] : 0.0f;
    }
    static C2D_DEV bool collide(const Obj& a, const Obj& b) { return rect_collide(a.r, b.r); }
    static C2D_DEV bool bounded(const Obj& a, const Obj& b) { return sweep_bounded(a.r) && sweep_bounded(b.r); }
    static C2D_DEV void axes(const Obj& a, const Obj& b, SweepPick& pick) { rect_sweep_axes(a.r, b.r, pick); }
};

// The query of listed_pairs: starts as the BAD_PAIR record.  A pair is settled without the walk when it starts in overlap, or when
// nothing moves and its coordinates are bounded (its answer is then a miss); a wave all of whose valid pairs are settled skips the walk.
template <class S>
struct SweepWork {
    uint4 word = make_uint4(0u, 0u, 0u, kSweepNoAxis | ((uint32_t)C2D_SWEEP_BAD_PAIR << 24));
    C2D_DEV void pair(const typename S::Obj& a, const typename S::Obj& b, bool valid)
    {
        const bool hit0 = S::collide(a, b);
        const float rx = b.dx - a.dx, ry = b.dy - a.dy;
        const bool settled = hit0 || (rx == 0.0f && ry == 0.0f && S::bounded(a, b));
        uint4 v = hit0 ? make_uint4(0u, 0u, 0u, kSweepNoAxis | (1u << 16) | ((uint32_t)C2D_SWEEP_START_OVERLAP << 24))
                       : make_uint4(__float_as_uint(__builtin_inff()), 0u, 0u, kSweepNoAxis);
        if (__ballot(valid && !settled) != 0ull) {   // (wave-uniform)
            SweepPick pick{rx, ry};
            S::axes(a, b, pick);
            if (!hit0) v = pick.record();
        }
        if (valid) word = v;
    }
    C2D_DEV void store(size_t p, c2d_sweep* __restrict__ out) const
    {
        reinterpret_cast<uint4*>(out)[p] = word;   // d_out is 16-byte aligned (checked on the host)
    }
};

template <class S>
__global__ __launch_bounds__(kPairListBlock) void sweep_kernel(typename S::Set A, typename S::Set B, const uint32_t* __restrict__ pairs, size_t n_pairs,
                                                               const unsigned long long* __restrict__ d_n, size_t row_base, size_t col_base,
                                                               c2d_sweep* __restrict__ out, uint32_t* __restrict__ async_err)
{
    listed_pairs<S, SweepWork<S>>(A, B, pairs, n_pairs, d_n, row_base, col_base, async_err, out);
}

// What the front ends of c2d_pair_list.hpp do not state: the motion of a set is two planes or none, 4-byte aligned.
inline int sweep_motion_check(c2d_ctx* ctx, const char* what, const float* d_a_dx, const float* d_a_dy, const float* d_b_dx, const float* d_b_dy)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if ((d_a_dx == nullptr) != (d_a_dy == nullptr) || (d_b_dx == nullptr) != (d_b_dy == nullptr))
        return cross_fail(ctx, what, "a set's motion is both planes or neither");
    if ((reinterpret_cast<uintptr_t>(d_a_dx) | reinterpret_cast<uintptr_t>(d_a_dy) | reinterpret_cast<uintptr_t>(d_b_dx) | reinterpret_cast<uintptr_t>(d_b_dy)) & 3u)
        return cross_fail(ctx, what, "motion planes must be 4-byte aligned");
    return C2D_OK;
}

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_pair_sweeps(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, const float* d_a_dx, const float* d_a_dy, const float* d_b_dx,
                         const float* d_b_dy, const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs, size_t row_base, size_t col_base,
                         c2d_sweep* d_out, c2d_stream stream)
{
    if (int rc = sweep_motion_check(ctx, "c2d_poly_pair_sweeps", d_a_dx, d_a_dy, d_b_dx, d_b_dy)) return rc;
    return poly_pair_list_call(ctx, "c2d_poly_pair_sweeps", a, b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const PolySetDev& A, const PolySetDev& B, int grid) {
                                   hipLaunchKernelGGL(sweep_kernel<PolySweepShape>, dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream,
                                                      PolySweepShape::Set{A, d_a_dx, d_a_dy}, PolySweepShape::Set{B, d_b_dx, d_b_dy}, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_out, ctx->d_async_err);
                               });
}

int c2d_rect_pair_sweeps(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b, const float* d_a_dx, const float* d_a_dy,
                         const float* d_b_dx, const float* d_b_dy, const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs, size_t row_base,
                         size_t col_base, c2d_sweep* d_out, c2d_stream stream)
{
    if (int rc = sweep_motion_check(ctx, "c2d_rect_pair_sweeps", d_a_dx, d_a_dy, d_b_dx, d_b_dy)) return rc;
    return rect_pair_list_call(ctx, "c2d_rect_pair_sweeps", d_a, n_a, d_b, n_b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const RectListSet& A, const RectListSet& B, int grid) {
                                   hipLaunchKernelGGL(sweep_kernel<RectSweepShape>, dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream,
                                                      RectSweepShape::Set{A, d_a_dx, d_a_dy}, RectSweepShape::Set{B, d_b_dx, d_b_dy}, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_out, ctx->d_async_err);
                               });
}

}  // extern "C"
