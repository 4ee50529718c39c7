// c2d_clearance_bound.hpp — the certified skip of the clearance query (c2d_clearance.hip): a lower bound of every usable candidate's
// d2 of a pair that is not hit, from the two polygons' vertex boxes alone.  Plain C++ (under hipcc the function is also marked for the
// device), binary32 and unfused: compile it with -ffp-contract=off, as the library is, so that it can be tested on a CPU against the
// numpy reference of the distance contract (tests/test_clearance_bound_cpu.py).
//
// The promise.  Let lb2 = clearance_lb2(box of A's live vertices, ca, box of B's live vertices, cb), a box being the exact float
// min / max of the live vertices' coordinates and ca, cb >= every |coordinate| of that polygon's live vertices.  Then for EVERY
// candidate (edge, vertex) of the pair by the distance contract of include/c2d.h, on either side, whose d2 is not NaN:  d2 >= lb2.
// Whether the pair is hit plays no part: the bound speaks of candidates only (the kernel asks it only about pairs that are not hit).
// lb2 = 0 promises nothing and skips nothing.
//
// The bound.  u = 2^-24, C = max(ca, cb).  The four axis gaps as floats, g1 = fl(bxlo - axhi), g2 = fl(axlo - bxhi), g3 = fl(bylo -
// ayhi), g4 = fl(aylo - byhi); g = the largest; m = 8 u C = 2^-21 C (exact: a power of two times a normal float that stays
// normal); L = fl(g - m); lb2 = fl(L * L) when L > 0, else 0.
//
// Proof.  Take a candidate with a d2 that is not NaN: edge (x0, y0) -> (x1, y1) of the polygon P, vertex (xp, yp) of the polygon Q;
// (P, Q) is (A, B) on side 0 and (B, A) on side 1, all three points are LIVE vertices, so x0, x1 lie in P's box, xp in Q's, and
// every coordinate is at most C in magnitude.  Let g_k be a gap with fl(g_k - m) > 0; by symmetry (exchange x and y, and the roles
// of the boxes) say g_k = fl(qxlo - pxhi), Q's box to the right of P's.  Write G = qxlo - pxhi for the real gap: |G| <= 2C, so
// |g_k - G| <= u |G| <= 2uC, and G >= g_k - 2uC > 0 since g_k > m = 8uC.
//   (1) The closest point's abscissa as computed, cx, is at most pxhi + 5.01 uC.
//       Regions 0 and 1: cx is x0 or x1 itself, at most pxhi.
//       Region 2 is reached when neither s <= 0 nor s >= len2 holds.  A NaN s makes t, cx, cy and d2 NaN: no such candidate is
//       usable.  Otherwise 0 < s < len2, both finite (domain, below), and the correctly rounded quotient of a real number in (0, 1)
//       lies in [0, 1]: 0 <= t <= 1.  ex = fl(x1 - x0) = (x1 - x0)(1 + d1), |d1| <= u, |x1 - x0| <= 2C.  In reals x0 + t (x1 - x0) lies
//       between x0 and x1, hence is at most pxhi, and x0 + t ex is at most pxhi + 2uC.  fl(t ex) differs from t ex by at most
//       u |t ex| <= 2uC (1 + u), or by at most 2^-150 where the product is subnormal (below 2^-26 uC in the domain).  The sum
//       x0 + fl(t ex) is at most C + 2C (1 + u) in magnitude but, being within 4.01 uC of [pxlo, pxhi], at most C (1 + 4.01u): its
//       rounding adds at most u C (1 + 4.01u).  Together: cx <= pxhi + (2 + 2 + 1) uC (1 + 2^-20) <= pxhi + 5.01 uC.
//   (2) dx = fl(xp - cx), and in reals xp - cx >= qxlo - pxhi - 5.01 uC = G - 5.01 uC >= g_k - 7.01 uC >= g_k - m.  Rounding to
//       nearest is monotone: dx = fl(xp - cx) >= fl(g_k - m) = L_k > 0.  (Sums and differences of floats are exact when subnormal.)
//   (3) Rounding is monotone on products of non-negative floats and on sums with a non-negative term:
//       fl(L_k L_k) <= fl(dx dx) <= fl(fl(dx dx) + fl(dy dy)) = d2.  An overflow on the right gives d2 = +inf, which is usable and
//       not below any float.
//   With P's box to the right of Q's the same holds for -dx; with a y gap for dy.  The largest g_k gives the largest L_k, and
//   fl(L L) is monotone in L >= 0: lb2 = max_k fl(L_k L_k) <= d2.
//
// Domain.  Finite coordinates with 2^-100 <= C <= 2^60: then |ex| <= 2^61, len2 and s stay below 2^124 (finite, as (1) uses), m and
// uC are normal (uC >= 2^-124) and the one underflow of (1) is far inside the slack between 5 (1 + 2^-20) and 5.01.  Outside the
// domain, or with any of the ten inputs NaN or infinite, lb2 = 0: every condition below is written so that a NaN fails it, and
// every box coordinate is checked against C, so a caller cannot pass a C that does not cover its boxes (a polygon whose live
// vertices hold a NaN or an infinity is passed with a largest coordinate of NaN or +inf and is never skipped).
//
// Use (c2d_clearance.hip).  The kernel walks the polygons of its strip in order of j with a running best (dist, j, d2) per lane and
// skips the candidate loops of pair j only when lb2 > best d2, strictly: every usable candidate of j then has d2 >= lb2 > best d2,
// hence a dist (the square root is monotone) that does not beat the best, which belongs to a smaller j; and a pair without a
// usable candidate has dist = +inf, which does not beat it either.
#pragma once

#if defined(__HIPCC__)
#define C2D_CLR_HD __host__ __device__ inline
#else
#define C2D_CLR_HD inline
#endif

namespace c2d {

constexpr float kClearanceCMin = 0x1p-100f, kClearanceCMax = 0x1p60f;   // the domain of the proof
constexpr float kClearanceMargin = 0x1p-21f;                            // m = 8 u C

// the vertex box of one polygon's live vertices and the largest |coordinate| among them (NaN or +inf: never skipped)
struct ClearanceBox {
    float xlo, xhi, ylo, yhi, c;
};

C2D_CLR_HD float clearance_lb2(const ClearanceBox& a, const ClearanceBox& b)
{
    const float C = a.c > b.c ? a.c : b.c;   // (a NaN in either fails its own compare below, whichever way this one goes)
    if (!((a.c >= 0.0f) & (b.c >= 0.0f) & (C >= kClearanceCMin) & (C <= kClearanceCMax))) return 0.0f;
    // every box coordinate within C: fails for a NaN or an infinite coordinate, and for a C that does not cover its boxes
    const bool inside = (a.xlo >= -C) & (a.xlo <= C) & (a.xhi >= -C) & (a.xhi <= C) & (a.ylo >= -C) & (a.ylo <= C) & (a.yhi >= -C) & (a.yhi <= C) &
                        (b.xlo >= -C) & (b.xlo <= C) & (b.xhi >= -C) & (b.xhi <= C) & (b.ylo >= -C) & (b.ylo <= C) & (b.yhi >= -C) & (b.yhi <= C);
    if (!inside) return 0.0f;
    const float g1 = b.xlo - a.xhi, g2 = a.xlo - b.xhi, g3 = b.ylo - a.yhi, g4 = a.ylo - b.yhi;   // (finite: every term is within C)
    float g = g1;
    g = g2 > g ? g2 : g;
    g = g3 > g ? g3 : g;
    g = g4 > g ? g4 : g;
    const float L = g - kClearanceMargin * C;
    return L > 0.0f ? L * L : 0.0f;
}

}  // namespace c2d
