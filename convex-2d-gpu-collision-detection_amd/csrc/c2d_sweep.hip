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
// One pair per lane on the frame of c2d_pair_list.hpp: the motion of an object rides in its shape (MovingShape there) and is loaded
// next to its vertices, so the frame's first-valid-lane substitution keeps those loads on valid indices as well.  The axis walk is
// that header's, the one the contact kernels use (compile-time vertex slots, one unrolled body per side with the polygons exchanged,
// axes at or beyond k masked out), with its boolean dropped: this file keeps the settled-pair shortcut and the record's store; the
// pick (c2d_sweep_rule.hpp, shared with the shape casts of c2d_cast.hip) carries the winner's raw axis and sign, and the square root
// and the two normal divisions are paid once, after the walk.  The two quotients per axis are the contract's own correctly rounded divisions: there is no estimate pass here.
#include "c2d_sweep_rule.hpp"   // SweepPick, sweep_bounded, sweep_motion_check; through it c2d_pair_list.hpp

namespace c2d {

static_assert(sizeof(c2d_sweep) == 16 && offsetof(c2d_sweep, nx) == 4 && offsetof(c2d_sweep, ny) == 8 && offsetof(c2d_sweep, axis) == 12 &&
                  offsetof(c2d_sweep, hit) == 14 && offsetof(c2d_sweep, flags) == 15,
              "the kernel stores a sweep as four dwords");

using PolySweepShape = MovingShape<PolyListShape>;
using RectSweepShape = MovingShape<RectListShape>;

// The query of listed_pairs on a MovingShape S (the W of pair_list_kernel): starts as the BAD_PAIR record.  A pair is settled without
// the walk when it starts in overlap, or when nothing moves and its coordinates are bounded (its answer is then a miss); a wave all of
// whose valid pairs are settled skips the walk.
template <class S>
struct SweepWork {
    uint4 word = make_uint4(0u, 0u, 0u, kSweepNoAxis | ((uint32_t)C2D_SWEEP_BAD_PAIR << 24));
    C2D_DEV void pair(const typename S::Obj& a, const typename S::Obj& b, bool valid)
    {
        const bool hit0 = S::collide(a, b);
        const float rx = b.dx - a.dx, ry = b.dy - a.dy;
        const bool settled = hit0 || (rx == 0.0f && ry == 0.0f && sweep_bounded(a) && sweep_bounded(b));
        uint4 v = hit0 ? make_uint4(0u, 0u, 0u, kSweepNoAxis | (1u << 16) | ((uint32_t)C2D_SWEEP_START_OVERLAP << 24))
                       : make_uint4(__float_as_uint(__builtin_inff()), 0u, 0u, kSweepNoAxis);
        if (__ballot(valid && !settled) != 0ull) {   // (wave-uniform)
            SweepPick pick{rx, ry};
            (void)S::axes(a, b, pick);   // (the pairwise boolean is hit0 already)
            if (!hit0) v = pick.record();
        }
        if (valid) word = v;
    }
    C2D_DEV void store(size_t p, c2d_sweep* __restrict__ out) const
    {
        reinterpret_cast<uint4*>(out)[p] = word;   // d_out is 16-byte aligned (checked on the host)
    }
};

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
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<PolySweepShape, SweepWork<PolySweepShape>, c2d_sweep>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream,
                                                      PolySweepShape::Set{A, d_a_dx, d_a_dy}, PolySweepShape::Set{B, d_b_dx, d_b_dy}, d_pairs,
                                                      n_pairs, d_n_pairs, row_base, col_base, d_out, ctx->d_async_err);
                               });
}

int c2d_rect_pair_sweeps(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b, const float* d_a_dx, const float* d_a_dy,
                         const float* d_b_dx, const float* d_b_dy, const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs, size_t row_base,
                         size_t col_base, c2d_sweep* d_out, c2d_stream stream)
{
    if (int rc = sweep_motion_check(ctx, "c2d_rect_pair_sweeps", d_a_dx, d_a_dy, d_b_dx, d_b_dy)) return rc;
    return rect_pair_list_call(ctx, "c2d_rect_pair_sweeps", d_a, n_a, d_b, n_b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const RectListSet& A, const RectListSet& B, int grid) {
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<RectSweepShape, SweepWork<RectSweepShape>, c2d_sweep>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream,
                                                      RectSweepShape::Set{A, d_a_dx, d_a_dy}, RectSweepShape::Set{B, d_b_dx, d_b_dy}, d_pairs,
                                                      n_pairs, d_n_pairs, row_base, col_base, d_out, ctx->d_async_err);
                               });
}

}  // extern "C"
