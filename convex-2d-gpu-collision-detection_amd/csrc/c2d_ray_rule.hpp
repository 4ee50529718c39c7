// c2d_ray_rule.hpp — what the ray queries share (c2d_ray.hip: c2d_poly_ray_casts; c2d_ray_grid.hip: c2d_poly_ray_casts_grid): the ray
// planes, the three cross products of one (ray, edge) and the usable-edge test of the contract of include/c2d.h, the 64-bit (t, j)
// key, and the last launch of either call (the first is c2d_set_best.hpp's set_best_launch_init<2>).
#pragma once

#include "c2d_cross.hpp"
#include "c2d_math.hpp"
#include "c2d_set_best.hpp"   // kSetNoKey, set_best_launch_init; through it c2d_poly_pair.hpp: PolySetDev, poly_set_check, poly_count

namespace c2d {

constexpr int kRayBlock = 256;   // rays per block: one per lane
constexpr uint32_t kRayNone16 = 0xFFFFu;

struct RayPlanes {
    const float* ox;
    const float* oy;
    const float* dx;
    const float* dy;
};

// the three cross products of one (ray, edge)
struct RayEdge {
    float den, tn, un;
};

C2D_DEV RayEdge ray_edge(float ox, float oy, float dx, float dy, float x0, float y0, float ex, float ey)
{
    const float wx = x0 - ox, wy = y0 - oy;
    return RayEdge{dx * ey - dy * ex, wx * ey - wy * ex, wx * dy - wy * dx};
}

// The rule's two cases folded into one by den's sign bit: with tn, un and den flipped where den is negative the second case reads as
// the first (a zero of either sign passes both "<= 0" and ">= 0", before and after the flip; a NaN fails either way; |den| > 0 fails
// for a den of +-0 or NaN).  Compares only, joined without branches: the boolean is the rule's for every bit pattern.
C2D_DEV bool ray_edge_usable(const RayEdge& c)
{
    const uint32_t sgn = __float_as_uint(c.den) & 0x80000000u;
    const float den = __uint_as_float(__float_as_uint(c.den) ^ sgn), tn = __uint_as_float(__float_as_uint(c.tn) ^ sgn),
                un = __uint_as_float(__float_as_uint(c.un) ^ sgn);
    return (int)(den > 0.0f) & (int)(tn >= 0.0f) & (int)(tn <= den) & (int)(un >= 0.0f) & (int)(un <= den);
}

// the 64-bit key of a candidate: t's bits (a -0 made +0) in the high word and col_base + j in the low word; for 0 <= t <= 1 the
// order of the keys is the order of (t, j)
C2D_DEV unsigned long long ray_key(float t, uint32_t poly)
{
    const uint32_t tb = t == 0.0f ? 0u : __float_as_uint(t);
    return ((unsigned long long)tb << 32) | (unsigned long long)poly;
}

// c2d_ray.hip: every record from its key, by the rule's own sequence
int ray_launch_finalise(c2d_ctx* ctx, hipStream_t s, const RayPlanes& R, size_t n_rays, const PolySetDev& B, uint32_t col_base, c2d_ray_hit* d_out);
// the argument checks both calls share (everything but the ctx): C2D_OK with B filled in, or the refusal
int ray_check_args(c2d_ctx* ctx, const char* what, const float* const d_rays[4], size_t n_rays, const c2d_poly_set* b, size_t col_base,
                   c2d_ray_hit* d_out, PolySetDev& B);

}  // namespace c2d
