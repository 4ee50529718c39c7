// c2d_distance_rule.hpp — the distance rule of include/c2d.h ("distance queries"), stated once for the translation units that need
// it (c2d_distance.hip: one record per listed pair; c2d_clearance.hip: the record of the nearest polygon of a set): the sequential
// pick over the candidates (edge, vertex) of one pair held in registers, and the record's two halves.  c2d_distance.hip states the
// rule in words.
#pragma once

#include "c2d_internal.hpp"
#include "c2d_math.hpp"

namespace c2d {

constexpr uint32_t kDistanceNone = 0xFFFFFFFFu;   // edge = vert = 0xFFFF
constexpr uint32_t kDistanceInterior = 1u << 8, kDistanceSide1 = 1u << 9;   // in DistancePick::code

// The sequential pick.  code = v | e << 4 | (region 2) << 8 | side << 9 of the best candidate so far; kDistanceNone: none yet.
struct DistancePick {
    float best = __builtin_inff(), cx = 0.0f, cy = 0.0f, px = 0.0f, py = 0.0f;   // d2, the closest point on the edge, the vertex
    uint32_t code = kDistanceNone;
};

// One side: the kp edges of P against the kq vertices of Q, in the order e, v.  P is turned by one slot per trip and ends as it began.
template <int K>
C2D_DEV void distance_side(float (&px)[K], float (&py)[K], int kp, const float (&qx)[K], const float (&qy)[K], int kq, uint32_t side_bits, DistancePick& pick)
{
    constexpr int kEdgeUnroll = K <= 4 ? K : 1;   // rectangles: 16 candidates per side, flat; polygons: one body of 16 per trip
#pragma unroll kEdgeUnroll
    for (int e = 0; e < K; e++) {
        const float x0 = px[0], y0 = py[0], x1 = px[1], y1 = py[1];
        const float ex = x1 - x0, ey = y1 - y0;
        const float len2 = ex * ex + ey * ey;
        const bool live_e = e < kp;
        const uint32_t code_e = side_bits | ((uint32_t)e << 4);
#pragma unroll
        for (int v = 0; v < K; v++) {
            const float xq = qx[v], yq = qy[v];
            const float ux = xq - x0, uy = yq - y0;
            const float s = ux * ex + uy * ey;
            const bool r0 = s <= 0.0f, r1 = s >= len2;   // (region 0 first; a NaN s fails both and takes region 2)
            const float t = s / len2;
            const float tx = x0 + t * ex, ty = y0 + t * ey;
            const float cx = r0 ? x0 : (r1 ? x1 : tx), cy = r0 ? y0 : (r1 ? y1 : ty);
            const float dx = xq - cx, dy = yq - cy;
            const float d2 = dx * dx + dy * dy;
            const bool take = live_e && v < kq && !__builtin_isnan(d2) && (pick.code == kDistanceNone || d2 < pick.best);
            pick.best = take ? d2 : pick.best;
            pick.cx = take ? cx : pick.cx;
            pick.cy = take ? cy : pick.cy;
            pick.px = take ? xq : pick.px;
            pick.py = take ? yq : pick.py;
            pick.code = take ? (code_e | (uint32_t)v | ((r0 || r1) ? 0u : kDistanceInterior)) : pick.code;
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

// Both sides of one pair to the record's two halves: d0 = {dist, ax, ay, bx}, d1 = {by, edge | vert << 16, hit | flags << 8, 0}.
template <int K>
C2D_DEV void distance_record(float (&ax)[K], float (&ay)[K], int ka, float (&bx)[K], float (&by)[K], int kb, uint4& d0, uint4& d1)
{
    DistancePick pick;
    distance_side<K>(ax, ay, ka, bx, by, kb, 0u, pick);
    distance_side<K>(bx, by, kb, ax, ay, ka, kDistanceSide1, pick);
    if (pick.code == kDistanceNone) {
        d0 = make_uint4(__float_as_uint(__builtin_inff()), 0u, 0u, 0u);
        d1 = make_uint4(0u, kDistanceNone, (uint32_t)C2D_DISTANCE_NO_CANDIDATE << 8, 0u);
        return;
    }
    const bool on_b = (pick.code & kDistanceSide1) != 0u;
    const uint32_t flags = (on_b ? (uint32_t)C2D_DISTANCE_EDGE_ON_B : 0u) | ((pick.code & kDistanceInterior) ? (uint32_t)C2D_DISTANCE_INTERIOR : 0u);
    const float pax = on_b ? pick.px : pick.cx, pay = on_b ? pick.py : pick.cy, pbx = on_b ? pick.cx : pick.px, pby = on_b ? pick.cy : pick.py;
    d0 = make_uint4(__float_as_uint(__builtin_sqrtf(pick.best)), __float_as_uint(pax), __float_as_uint(pay), __float_as_uint(pbx));
    d1 = make_uint4(__float_as_uint(pby), ((pick.code >> 4) & 15u) | ((pick.code & 15u) << 16), flags << 8, 0u);
}

}  // namespace c2d
