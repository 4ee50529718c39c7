// c2d_poly_pair.hpp — one convex polygon of a c2d_poly_set in registers, and the exact polygon test of one pair per lane.
//
// poly_collide(A, B) is value-equal to what c2d_sat_poly_pairs_rows computes for the pair (c2d_poly.hip): the true normals
// (-e.y, e.x) of all ka + kb own edges, projections nx * x + ny * y unfused in every build (poly_minmax, c2d_math.hpp), strict <, and the NaN rule
// of first_projections_ordered (c2d_math.hpp).  It is the form for callers whose lanes hold unrelated pairs (the broad phase,
// c2d_poly_broad.hip): every loop runs over the 16 vertex slots with compile-time indices, so the vertices stay in registers.
// Slots >= k repeat vertex 0, which is exactly neutral: a repeated vertex adds a zero-length edge, whose axis (0, 0) never
// separates, and repeats a projection, which changes no min / max (c2d_poly.hip).
#pragma once

#include <cstdio>

#include "c2d_internal.hpp"
#include "c2d_math.hpp"

namespace c2d {

static_assert(C2D_POLY_KMAX == 16, "the polygon loops are written for 16 vertex slots");

struct PolySetDev {
    const float* vx;
    const float* vy;
    const uint8_t* k;   // nullptr: every polygon has `rows` vertices
    size_t n, stride;
    int rows;
};

constexpr bool kEmptySetOk = true;

// The checks of one c2d_poly_set (rows, planes, alignment, stride); C2D_OK or the status to return.  empty_ok, for set b of a query
// that has a result against no polygons at all: of an empty set only `rows` is looked at, and no plane is read.
inline int poly_set_check(c2d_ctx* ctx, const char* what, const char* which, const c2d_poly_set* set, PolySetDev& out, bool empty_ok = false)
{
    char msg[192];
    auto fail = [&](const char* why) {
        std::snprintf(msg, sizeof msg, "%s: set %s: %s", what, which, why);
        return fail_arg(ctx, msg);
    };
    if (set->rows < 1 || set->rows > (uint32_t)C2D_POLY_KMAX) return fail("rows must be 1..C2D_POLY_KMAX");
    if (empty_ok && set->n == 0) {
        out = PolySetDev{nullptr, nullptr, nullptr, 0, 0, (int)set->rows};
        return C2D_OK;
    }
    if (!set->d_vx || !set->d_vy) return fail("NULL plane");
    if ((reinterpret_cast<uintptr_t>(set->d_vx) | reinterpret_cast<uintptr_t>(set->d_vy)) & 3u) return fail("planes must be 4-byte aligned");
    const size_t stride = set->stride ? set->stride : set->n;
    if (stride < set->n) return fail("stride < n");
    out = PolySetDev{set->d_vx, set->d_vy, set->d_k, set->n, stride, (int)set->rows};
    return C2D_OK;
}


// "B is A": the same planes read the same way, so one pass over them serves both sides
inline bool poly_sets_same(const PolySetDev& A, const PolySetDev& B)
{
    return A.vx == B.vx && A.vy == B.vy && A.k == B.k && A.n == B.n && A.stride == B.stride && A.rows == B.rows;
}

// one polygon: k real vertices, slots >= k repeat vertex 0
struct PolyObj {
    float x[C2D_POLY_KMAX], y[C2D_POLY_KMAX];
    int k;
};

// The vertex count of polygon i as stored; false when it is outside 1..rows.
C2D_DEV bool poly_count(const PolySetDev& X, size_t i, int& k)
{
    k = X.k ? (int)X.k[i] : X.rows;
    return k >= 1 && k <= X.rows;
}

// Polygon i with neutral padding.  A count outside 1..rows is clamped (memory safety: only rows below the count are read, and the
// count never exceeds the rows the planes have); the caller decides what such a polygon means.
C2D_DEV void poly_load(const PolySetDev& X, size_t i, PolyObj& p)
{
    int k;
    (void)poly_count(X, i, k);
    k = k < 1 ? 1 : (k > X.rows ? X.rows : k);
    p.k = k;
    p.x[0] = X.vx[i];
    p.y[0] = X.vy[i];
#pragma unroll
    for (int r = 1; r < C2D_POLY_KMAX; r++) {
        p.x[r] = p.x[0];
        p.y[r] = p.y[0];
        if (r < k) {   // r < k <= rows: inside the planes
            p.x[r] = X.vx[(size_t)r * X.stride + i];
            p.y[r] = X.vy[(size_t)r * X.stride + i];
        }
    }
}

// "some own edge normal of P separates P and Q".  Axes >= P.k are zero vectors and are skipped (they never separate).
C2D_DEV bool poly_own_axes_separate(const PolyObj& P, const PolyObj& Q)
{
    const float inf = __builtin_inff();
    bool sep = false;
#pragma unroll
    for (int a = 0; a < C2D_POLY_KMAX; a++) {
        if (a < P.k) {
            const int a1 = (a + 1) & (C2D_POLY_KMAX - 1);
            const float nx = -(P.y[a1] - P.y[a]), ny = P.x[a1] - P.x[a];
            float mnp = inf, mxp = -inf, mnq = inf, mxq = -inf;
#pragma unroll
            for (int r = 0; r < C2D_POLY_KMAX; r++) {
                poly_minmax(nx, ny, P.x[r], P.y[r], mnp, mxp);
                poly_minmax(nx, ny, Q.x[r], Q.y[r], mnq, mxq);
            }
            sep |= ((mxp < mnq) || (mxq < mnp)) && first_projections_ordered(nx * P.x[0] + ny * P.y[0], nx * Q.x[0] + ny * Q.y[0]);
        }
    }
    return sep;
}

// The exact test of the pair (A, B): no axis of either polygon separates them.  The two halves run as two trips of one loop with
// the polygons exchanged, so that the unrolled body exists once per call site.
C2D_DEV bool poly_collide(const PolyObj& A, const PolyObj& B)
{
    PolyObj P = A, Q = B;
    bool sep = false;
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
        sep |= poly_own_axes_separate(P, Q);
        const PolyObj t = P;
        P = Q;
        Q = t;
    }
    return !sep;
}

}  // namespace c2d
