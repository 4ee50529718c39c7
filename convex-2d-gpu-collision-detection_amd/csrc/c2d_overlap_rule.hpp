// c2d_overlap_rule.hpp — the overlap rule of include/c2d.h ("overlap queries"), stated once for the translation units that need it
// (c2d_overlap.hip: one record per listed pair; a set-level reduction can share it later, as c2d_distance_rule.hpp is shared): the
// shift to A's vertex 0, the two shoelace sums, the boundary integral of A ∩ B over the clipped edges of both shapes held in
// registers, and the record's two halves.  c2d_overlap.hip states the rule in words.
#pragma once

#include "c2d_internal.hpp"
#include "c2d_math.hpp"

namespace c2d {

constexpr uint32_t kOverlapQuietNaN = 0x7FC00000u;   // what a NaN float of the record is stored as

// The bits of a float of the record: a NaN, whatever its sign and payload, is stored as the one quiet NaN.
C2D_DEV uint32_t overlap_bits(float v) { return __builtin_isnan(v) ? kOverlapQuietNaN : __float_as_uint(v); }

// Both shapes to the frame of r = A's vertex 0 (one rounding per coordinate; padding stays a copy of the shape's vertex 0).
template <int K>
C2D_DEV void overlap_shift(float (&ax)[K], float (&ay)[K], float (&bx)[K], float (&by)[K], float& rx, float& ry)
{
    rx = ax[0];
    ry = ay[0];
#pragma unroll
    for (int v = 0; v < K; v++) {
        ax[v] = ax[v] - rx; ay[v] = ay[v] - ry;
        bx[v] = bx[v] - rx; by[v] = by[v] - ry;
    }
}

// The shoelace sum of the k real vertices, from 0 in vertex order (slot k, or slot 0 behind slot K - 1, closes the polygon).
template <int K>
C2D_DEV float overlap_shoelace(const float (&x)[K], const float (&y)[K], int k)
{
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const int i1 = (i + 1) & (K - 1);
        const float c = x[i] * y[i1] - y[i] * x[i1];
        sum = i < k ? sum + c : sum;
    }
    return sum;
}

struct OverlapSums {
    float S, Mx, My;
    uint32_t pieces;
};

constexpr float kOverlapOnLine = 0x1p-21f;   // 8 u: two edges lie on one line within 8 u D (|x| + |y|) of each of their four cross products

// kD = 8 u D, D the largest |coordinate| of the shifted pair (compare and select from 0; the padded slots repeat vertex 0).
template <int K>
C2D_DEV float overlap_extent(const float (&ax)[K], const float (&ay)[K], const float (&bx)[K], const float (&by)[K])
{
    float D = 0.0f;
#pragma unroll
    for (int v = 0; v < K; v++) {
        const float c0 = __builtin_fabsf(ax[v]), c1 = __builtin_fabsf(ay[v]);
        D = c0 > D ? c0 : D;
        D = c1 > D ? c1 : D;
    }
#pragma unroll
    for (int v = 0; v < K; v++) {
        const float c0 = __builtin_fabsf(bx[v]), c1 = __builtin_fabsf(by[v]);
        D = c0 > D ? c0 : D;
        D = c1 > D ? c1 : D;
    }
    return kOverlapOnLine * D;
}

// One side: the kp edges of P, each clipped against every edge of Q, to the side's sums (from 0, in edge order).  P is turned by one
// slot per trip and ends as it began.  Q needs no mask: an edge between two padded slots has length zero and is skipped, or is NaN
// and fails every compare.  `wanted`: this lane keeps the result (a trip that no lane of the wave wants only turns P).  `side0` is
// the same in every lane, so what only one side needs sits behind a branch on it; the split of two edges on one line sits behind
// a ballot (hardly any wave of unrelated pairs holds such a pair).
template <int K>
C2D_DEV void overlap_side(float (&px)[K], float (&py)[K], int kp, float sp, const float (&qx)[K], const float (&qy)[K], float sq, bool side0, bool wanted,
                          float kD, OverlapSums& o)
{
    constexpr int kEdgeUnroll = K <= 4 ? K : 1;   // rectangles: 16 clips per side, flat; polygons: one body of 16 per trip
    const float spq = sp * sq;
    o.S = 0.0f; o.Mx = 0.0f; o.My = 0.0f;
    o.pieces = 0u;
#pragma unroll kEdgeUnroll
    for (int e = 0; e < K; e++) {
        const bool live_e = wanted && e < kp;
        if (__ballot(live_e) != 0ull) {   // (wave-uniform)
            const float x0 = px[0], y0 = py[0], x1 = px[1], y1 = py[1];
            const float ex = x1 - x0, ey = y1 - y0;
            const float tol_e = kD * (__builtin_fabsf(ex) + __builtin_fabsf(ey));
            float t0 = 0.0f, t1 = 1.0f;
            float ux = x0, uy = y0, vx = x1, vy = y1;
            bool alive = true;
#pragma unroll
            for (int f = 0; f < K; f++) {
                const int f1 = (f + 1) & (K - 1);
                const float a0 = qx[f], b0 = qy[f], a1 = qx[f1], b1 = qy[f1];
                const float gx = a1 - a0, gy = b1 - b0;
                const float tol_g = kD * (__builtin_fabsf(gx) + __builtin_fabsf(gy));
                const float c_p0 = gx * (y0 - b0) - gy * (x0 - a0);
                const bool real = !(gx == 0.0f && gy == 0.0f);
                // on one line?  The first of the four cross products says no for nearly every pair of edges; the other three are
                // computed only where it does not for some lane that keeps its result.
                const bool near = real && __builtin_fabsf(c_p0) <= tol_g;
                float c_p1 = 0.0f, c_q0 = 0.0f, c_q1 = 0.0f;
                bool on_line = false;
                if (__ballot(live_e && near) != 0ull) {   // (wave-uniform)
                    c_p1 = gx * (y1 - b0) - gy * (x1 - a0);
                    c_q0 = ex * (b0 - y0) - ey * (a0 - x0);
                    c_q1 = ex * (b1 - y0) - ey * (a1 - x0);
                    on_line = near && __builtin_fabsf(c_p1) <= tol_g && __builtin_fabsf(c_q0) <= tol_e && __builtin_fabsf(c_q1) <= tol_e;
                }
                const bool same_way = spq * (ex * gx + ey * gy) > 0.0f;
                // two edges that cross: one point for both sides, A's p0 + t * e (computed where some lane's t0 or t1 moves)
                const float num = sq * c_p0;
                const float den = sq * (gx * ey - gy * ex);
                const float q = (-num) / den;
                const bool cuts = real && !on_line;
                const bool lower = cuts && den > 0.0f && q > t0, upper = cuts && den < 0.0f && q < t1;   // a NaN quotient moves nothing
                if (__ballot(live_e && (lower || upper)) != 0ull) {   // (wave-uniform)
                    float tc = q;
                    if (!side0) tc = (-(sp * (ex * (b0 - y0) - ey * (a0 - x0)))) / (sp * (ex * gy - ey * gx));   // (wave-uniform) A's edge is Q's here
                    const float cx = (side0 ? x0 : a0) + tc * (side0 ? ex : gx), cy = (side0 ? y0 : b0) + tc * (side0 ? ey : gy);
                    t0 = lower ? q : t0; ux = lower ? cx : ux; uy = lower ? cy : uy;
                    t1 = upper ? q : t1; vx = upper ? cx : vx; vy = upper ? cy : vy;
                }
                const bool keeps = num > 0.0f || (side0 && num == 0.0f && same_way);
                alive = alive && !(cuts && den == 0.0f && !keeps) && !(on_line && !same_way);
                // two edges on one line that run the same way: A's is the boundary where it is inside B, B's elsewhere
                const bool split = on_line && same_way;
                if (__ballot(live_e && split) != 0ull) {   // (wave-uniform)
                    const float da = side0 ? sq * c_p0 : sp * c_q0, db = side0 ? sq * c_p1 : sp * c_q1;
                    const bool inside = da >= 0.0f && db >= 0.0f;
                    const bool outside = !inside && da <= 0.0f && db <= 0.0f;
                    const bool enters = da < 0.0f && db > 0.0f, leaves = da > 0.0f && db < 0.0f;
                    const float ts = da / (da - db);
                    const float sx = (side0 ? x0 : a0) + ts * (side0 ? ex : gx), sy = (side0 ? y0 : b0) + ts * (side0 ? ey : gy);
                    float s = ts;
                    if (!side0) s = ((sx - x0) * ex + (sy - y0) * ey) / (ex * ex + ey * ey);   // (wave-uniform)
                    const bool along = side0 || spq > 0.0f;
                    const bool from_s = side0 ? enters : (along ? leaves : enters), to_s = side0 ? leaves : (along ? enters : leaves);
                    alive = alive && !(split && (side0 ? outside : inside));
                    const bool lo = split && from_s && s > t0, hi = split && to_s && s < t1;
                    t0 = lo ? s : t0; ux = lo ? sx : ux; uy = lo ? sy : uy;
                    t1 = hi ? s : t1; vx = hi ? sx : vx; vy = hi ? sy : vy;
                }
            }
            const float c = sp * (ux * vy - uy * vx);
            const bool piece = live_e && alive && t0 < t1;
            o.S = piece ? o.S + c : o.S;
            o.Mx = piece ? o.Mx + (ux + vx) * c : o.Mx;
            o.My = piece ? o.My + (uy + vy) * c : o.My;
            o.pieces += piece ? 1u : 0u;
        }
        const float fx = px[0], fy = py[0];
#pragma unroll
        for (int r = 0; r + 1 < K; r++) {
            px[r] = px[r + 1];
            py[r] = py[r + 1];
        }
        px[K - 1] = fx;
        py[K - 1] = fy;
    }
}

// What the record needs of one pair: the frame, the two shoelace sums, and (after overlap_clip) the boundary integral.
struct OverlapPair {
    float rx, ry, sum_a, sum_b;
    float S = 0.0f, Mx = 0.0f, My = 0.0f;
    uint32_t pieces_a = 0u, pieces_b = 0u;
};

// Both sides of one pair (already shifted).  The two shapes change places between the sides, so the clip's text exists once.
template <int K>
C2D_DEV void overlap_clip(float (&ax)[K], float (&ay)[K], int ka, float (&bx)[K], float (&by)[K], int kb, bool wanted, OverlapPair& o)
{
    const float sa = o.sum_a > 0.0f ? 1.0f : -1.0f, sb = o.sum_b > 0.0f ? 1.0f : -1.0f;
    const float kD = overlap_extent<K>(ax, ay, bx, by);
    if constexpr (K <= 4) {
        OverlapSums s0, s1;
        overlap_side<K>(ax, ay, ka, sa, bx, by, sb, true, wanted, kD, s0);
        overlap_side<K>(bx, by, kb, sb, ax, ay, sa, false, wanted, kD, s1);
        o.S = s0.S + s1.S; o.Mx = s0.Mx + s1.Mx; o.My = s0.My + s1.My;
        o.pieces_a = s0.pieces;
        o.pieces_b = s1.pieces;
    } else {
        int kp = ka, kq = kb;
        float sp = sa, sq = sb;
#pragma unroll 1
        for (int side = 0; side < 2; side++) {
            OverlapSums s;
            overlap_side<K>(ax, ay, kp, sp, bx, by, sq, side == 0, wanted, kD, s);
            o.S = side ? o.S + s.S : s.S;
            o.Mx = side ? o.Mx + s.Mx : s.Mx;
            o.My = side ? o.My + s.My : s.My;
            o.pieces_a = side ? o.pieces_a : s.pieces;
            o.pieces_b = side ? s.pieces : 0u;
#pragma unroll
            for (int v = 0; v < K; v++) {
                const float tx = ax[v], ty = ay[v];
                ax[v] = bx[v]; ay[v] = by[v];
                bx[v] = tx; by[v] = ty;
            }
            const int tk = kp;
            kp = kq; kq = tk;
            const float ts = sp;
            sp = sq; sq = ts;
        }
    }
}

// The record's two halves: d0 = {area, iou, cx, cy}, d1 = {area_a, area_b, hit | flags << 8 | pieces_a << 16 | pieces_b << 24, 0}.
C2D_DEV void overlap_halves(const OverlapPair& o, bool hit, uint4& d0, uint4& d1)
{
    const float area_a = 0.5f * __builtin_fabsf(o.sum_a), area_b = 0.5f * __builtin_fabsf(o.sum_b);
    const uint32_t ua = overlap_bits(area_a), ub = overlap_bits(area_b);
    if (!hit) {
        d0 = make_uint4(0u, 0u, 0u, 0u);
        d1 = make_uint4(ua, ub, (uint32_t)C2D_OVERLAP_NO_CENTROID << 8, 0u);
        return;
    }
    if (!(o.sum_a > 0.0f || o.sum_a < 0.0f) || !(o.sum_b > 0.0f || o.sum_b < 0.0f)) {   // a sum of 0 or NaN
        d0 = make_uint4(0u, 0u, 0u, 0u);
        d1 = make_uint4(ua, ub, 1u | (uint32_t)(C2D_OVERLAP_DEGENERATE | C2D_OVERLAP_NO_CENTROID) << 8, 0u);
        return;
    }
    const float raw = 0.5f * o.S;
    const float lo = raw > 0.0f ? raw : 0.0f;
    const float cap = area_b < area_a ? area_b : area_a;
    const float area = cap < lo ? cap : lo;
    uint32_t flags = area == raw ? 0u : (uint32_t)C2D_OVERLAP_CLAMPED;
    const float uni = (area_a + area_b) - area;
    const float iou = uni > 0.0f ? area / uni : 0.0f;
    float cx = 0.0f, cy = 0.0f;
    if (o.S > 0.0f) {
        const float s3 = 3.0f * o.S;
        cx = o.rx + o.Mx / s3;
        cy = o.ry + o.My / s3;
    } else {
        flags |= (uint32_t)C2D_OVERLAP_NO_CENTROID;
    }
    d0 = make_uint4(overlap_bits(area), overlap_bits(iou), overlap_bits(cx), overlap_bits(cy));
    d1 = make_uint4(ua, ub, 1u | flags << 8 | o.pieces_a << 16 | o.pieces_b << 24, 0u);
}

}  // namespace c2d
