// c2d_ray_walk.hpp — the candidate predicate of the grid-accelerated ray query (c2d_poly_ray_casts_grid; include/c2d.h)
// and the enumeration of the grid cells a ray has to look at.  Plain C++ (under hipcc the functions are also marked for the device:
// the walk kernel of c2d_ray_grid.hip runs them), so that both can be tested on a CPU (tests/test_ray_walk_cpu.py).  Everything here
// is binary64, unfused, in the written order.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define C2D_WALK_HD __host__ __device__ inline
#else
#define C2D_WALK_HD inline
#endif

namespace c2d {

// ---- the contract's predicate -------------------------------------------------------------------------------------------------
struct RayD {
    double ox, oy, dx, dy, bx, by;   // bx = ox + dx, by = oy + dy
    double c;                        // the largest magnitude among ox, oy, bx, by; NaN when one of them is
};

// the larger of c and |v|; a NaN stays
C2D_WALK_HD double ray_mag(double c, double v)
{
    const double a = __builtin_fabs(v);
    return (a > c || a != a) ? a : c;
}
C2D_WALK_HD double ray_min(double a, double b) { return b < a ? b : a; }
C2D_WALK_HD double ray_max(double a, double b) { return b > a ? b : a; }

C2D_WALK_HD RayD ray_d(float ox, float oy, float dx, float dy)
{
    RayD r;
    r.ox = ox;
    r.oy = oy;
    r.dx = dx;
    r.dy = dy;
    r.bx = r.ox + r.dx;
    r.by = r.oy + r.dy;
    r.c = ray_mag(ray_mag(ray_mag(ray_mag(0.0, r.ox), r.oy), r.bx), r.by);
    return r;
}

// meets(r, box) of include/c2d.h: the box xl, xh, yl, yh (no NaN among them) against the ray.  Every compare fails on a NaN, so a
// non-finite ray or an infinite box meets.
C2D_WALK_HD bool ray_meets(const RayD& r, float xlf, float xhf, float ylf, float yhf)
{
    const double xl = xlf, xh = xhf, yl = ylf, yh = yhf;
    const double C = ray_mag(ray_mag(ray_mag(ray_mag(r.c, xl), xh), yl), yh);
    const double m = 0x1p-20 * C;
    const bool sx = ray_min(r.ox, r.bx) > xh + m || ray_max(r.ox, r.bx) < xl - m;
    const bool sy = ray_min(r.oy, r.by) > yh + m || ray_max(r.oy, r.by) < yl - m;
    const double cx = 0.5 * xl + 0.5 * xh, hx = (0.5 * xh - 0.5 * xl) + m;
    const double cy = 0.5 * yl + 0.5 * yh, hy = (0.5 * yh - 0.5 * yl) + m;
    const bool sn = __builtin_fabs(r.dx * (cy - r.oy) - r.dy * (cx - r.ox)) > hx * __builtin_fabs(r.dy) + hy * __builtin_fabs(r.dx);
    return !(sx || sy || sn);
}

// ---- the grid -----------------------------------------------------------------------------------------------------------------
// The broad phase's uniform grid (c2d_broad.hpp BroadGrid): cell of v = floor((v - v0) * inv) clamped to [0, g - 1], in double as in
// DESIGN.md §5.8; monotone non-decreasing in v.  G is the largest |coordinate| of the grid's bounds: every box inside the bounds has
// its four coordinates at or below G in magnitude.
struct WalkGrid {
    double x0, y0, ix, iy;
    uint32_t gx, gy;
    double G;
};

C2D_WALK_HD uint32_t walk_cell(double v, double v0, double inv, uint32_t g)
{
    double t = (v - v0) * inv;
    t = t > 0.0 ? __builtin_floor(t) : 0.0;   // (a NaN goes to 0)
    const double top = (double)(g - 1);
    return (uint32_t)(t < top ? t : top);
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------
// A regular box of the grid is keyed by the cell of its min corner, key = cy(yl) * gx + cx(xl), and spans at most two cells per axis:
// cx(xh) <= cx(xl) + 1, cy(yh) <= cy(yl) + 1.  The walk of a FINITE ray with c < 2^60 enumerates, per key row R of
// [row0, row1], one key range [R * gx + col0(R), R * gx + col1(R)].
//
// THE PROOF OBLIGATION: for a regular box that lies inside the grid's bounds, ray_meets implies that its key lies in an enumerated
// range.  (Regular boxes outside the bounds are few — at most max(4, n / 65536), the boxes at or above the cell-size pick — and the
// caller tests them against every ray, as it tests the wild ones.)
//
//   Let M = 2^-20 max(c, G) and W = 3 M.  The box's m is at most M (its C is at most max(c, G)).
//   (1) !sx, !sy: fl(xl - m) <= max(ox, bx), and fl is monotone, so xl <= max(ox, bx) + M (1 + 2^-31): the rounding of one double
//       operation on values at or below 2^62 max(c, G) is below 2^-32 M.  Likewise xh >= min(ox, bx) - M (1 + 2^-31), and in y.
//   (2) !sn: the three products, the differences and the sums of the test carry a relative error below 2^-50, an absolute error
//       below 2^-48 C (|dx| + |dy|) <= 2^-28 M (|dx| + |dy|); so in exact arithmetic |d x (centre - o)| <= (hx0 + 2M)|dy| + (hy0 + 2M)|dx|
//       with the exact half extents hx0, hy0: the infinite line of the ray meets the box widened by 2M on every side.
//   (3) A line that meets an axis-parallel box Q, whose segment's own box meets Q too, meets Q within the segment: were the line's
//       point q of Q beyond the end point p, and s a point of Q in the segment's box, then p lies in the box spanned by q and s,
//       which Q contains.  So some point p of the segment has  xl - 2M <= p.x <= xh + 2M  and  yl - 2M <= p.y <= yh + 2M.
//   (4) Rows: cy(yl) <= cell(p.y + 2M) <= row1 and cy(yl) >= cy(yh) - 1 >= cell(p.y - 2M) - 1 >= row0, with p.y inside the
//       segment's y range and cell() monotone.
//   (5) Columns of key row R = cy(yl): yl lies in row R and yh in row R or R + 1, so p.y lies in the band
//       [bottom(R) - 2M, top(R + 1) + 2M], where bottom / top are the inverses of cell() (-inf below row 1, +inf from row
//       gy - 1 on).  The inverses, the parameters t = (band - oy) / dy clamped to [0, 1] and the points ox + t dx are computed
//       with errors below 2^-28 M each (2^-49 G for the inverses, 2^-50 c for the points); the third M of W covers them.  The
//       segment's points inside the band have x in [xa, xb], so xl <= xb + 2M and xh >= xa - 2M:
//       cx(xl) <= cell(xb + W) = col1 and cx(xl) >= cx(xh) - 1 >= cell(xa - W) - 1 = col0.
// The enumeration is never empty and never more than the rows and columns the segment's own box covers (plus the low sides).
struct RayWalk {
    RayD r;
    double W;
    uint32_t row0, row1;
};

// false: the ray is not walked (non-finite, or c >= 2^60): the caller tests it against everything
C2D_WALK_HD bool ray_walk_begin(const WalkGrid& g, const RayD& r, RayWalk& w)
{
    if (!(r.c < 0x1p60) || !(__builtin_fabs(r.dx) < __builtin_inf()) || !(__builtin_fabs(r.dy) < __builtin_inf())) return false;
    w.r = r;
    w.W = 3.0 * (0x1p-20 * ray_max(r.c, g.G));
    const uint32_t lo = walk_cell(ray_min(r.oy, r.by) - w.W, g.y0, g.iy, g.gy);
    w.row0 = lo ? lo - 1u : 0u;
    w.row1 = walk_cell(ray_max(r.oy, r.by) + w.W, g.y0, g.iy, g.gy);
    return true;
}

// the columns [col0, col1] of key row R (row0 <= R <= row1)
C2D_WALK_HD void ray_walk_row(const WalkGrid& g, const RayWalk& w, uint32_t R, uint32_t& col0, uint32_t& col1)
{
    const RayD& r = w.r;
    double xa = ray_min(r.ox, r.bx), xb = ray_max(r.ox, r.bx);
    if (r.dy != 0.0) {
        const double inf = __builtin_inf();
        const double ya = R == 0u ? -inf : (g.y0 + (double)R / g.iy) - w.W;
        const double yb = R + 2u >= g.gy ? inf : (g.y0 + (double)(R + 2u) / g.iy) + w.W;
        double ta = (ya - r.oy) / r.dy, tb = (yb - r.oy) / r.dy;
        ta = ta > 0.0 ? (ta < 1.0 ? ta : 1.0) : 0.0;
        tb = tb > 0.0 ? (tb < 1.0 ? tb : 1.0) : 0.0;
        const double pa = r.ox + ta * r.dx, pb = r.ox + tb * r.dx;
        // (the points never leave the segment's own x range: t is in [0, 1])
        xa = ray_max(xa, ray_min(pa, pb));
        xb = ray_min(xb, ray_max(pa, pb));
    }
    const uint32_t lo = walk_cell(xa - w.W, g.x0, g.ix, g.gx);
    col0 = lo ? lo - 1u : 0u;
    col1 = walk_cell(xb + w.W, g.x0, g.ix, g.gx);
}

}  // namespace c2d
