// c2d_sweep_rule.hpp — the sweep rule of include/c2d.h ("swept queries"), stated once for the translation units that need it
// (c2d_sweep.hip: one record per listed pair; c2d_cast.hip: the record of the first-touched polygon of a set): the sequential pick over
// the axes of one pair with its record, the bound under which a pair at rest is settled without a walk, and the check of the motion
// planes that every entry point with motions states.  c2d_sweep.hip states the rule in words.
#pragma once

#include "c2d_pair_list.hpp"

namespace c2d {

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

// (of an object: every coordinate of it)
C2D_DEV bool sweep_bounded(const PolyObj& o) { return sweep_bounded(o.x) && sweep_bounded(o.y); }
C2D_DEV bool sweep_bounded(const RectListShape::Obj& o) { return sweep_bounded(o.r); }

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
