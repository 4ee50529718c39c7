// c2d_distance.hip — distance queries for gfx950 (MI355X): for each listed pair (A_i, B_j) the boolean of the pairwise test and, when
// the pair is separated, the Euclidean distance of the two shapes with the two points that realise it (c2d_poly_pair_distances,
// c2d_rect_pair_distances; include/c2d.h "distance queries").
//
// The rule (the contract of include/c2d.h).  A candidate is an edge of one shape and a vertex of the other: side 0 takes A's edges
// e = 0 .. ka - 1 against B's vertices v = 0 .. kb - 1, side 1 B's edges against A's vertices.  Per candidate, with the edge
// (x0, y0) -> (x1, y1) and the vertex (xp, yp), everything binary32 and unfused:
//     ex = x1 - x0, ey = y1 - y0, qx = xp - x0, qy = yp - y0, len2 = ex * ex + ey * ey, s = qx * ex + qy * ey
//     region 0: s <= 0: c = (x0, y0);  region 1: else s >= len2: c = (x1, y1);  region 2: else t = s / len2, c = (x0 + t * ex, y0 + t * ey)
//     d2 = (xp - cx)^2 + (yp - cy)^2; unusable when d2 is NaN.
// In the order side, e, v the first usable candidate is the first best and a later one replaces it only under strict d2 < best.
//
// One pair per lane on the frame of c2d_pair_list.hpp, which also holds the kernel and, in its list shapes, the pairwise boolean
// (S::collide): this file adds the candidates' record to those shapes and keeps the query.  The lanes of a wave hold unrelated pairs,
// so the vertices stay in registers and every vertex index is a compile-time slot: the sweep always works on the edge from slot 0 to
// slot 1 of the edge polygon and turns that polygon by one slot per trip, so the edge loop stays rolled (one body of K candidates
// instead of K * K) and the polygon is back in place after K trips.  poly_load's padding repeats vertex 0, which closes the polygon
// for free: slot k is vertex 0, and slot 16 is slot 0.  The padding is NOT neutral otherwise: a padded candidate reaches vertex 0
// directly, a real one reaches the same point through t, and the two d2 can differ by a rounding — so slots with e >= k or v >= k are
// masked out of the pick.  The pick and the record live in c2d_distance_rule.hpp, which the clearance query (c2d_clearance.hip) shares.
#include "c2d_distance_rule.hpp"
#include "c2d_pair_list.hpp"

namespace c2d {

static_assert(sizeof(c2d_distance) == 32 && offsetof(c2d_distance, ax) == 4 && offsetof(c2d_distance, bx) == 12 && offsetof(c2d_distance, by) == 16 &&
                  offsetof(c2d_distance, edge) == 20 && offsetof(c2d_distance, vert) == 22 && offsetof(c2d_distance, hit) == 24 &&
                  offsetof(c2d_distance, flags) == 25 && offsetof(c2d_distance, reserved0) == 26 && offsetof(c2d_distance, reserved1) == 28,
              "the kernel stores a distance as two halves of four dwords");

// The shapes of c2d_pair_list.hpp with what the distance kernel adds:
//   S::record(a, b, d0, d1)      the record of a pair that is not hit (a and b are turned and restored)
struct PolyDistanceShape : PolyListShape {
    static C2D_DEV void record(Obj& a, Obj& b, uint4& d0, uint4& d1) { distance_record<C2D_POLY_KMAX>(a.x, a.y, a.k, b.x, b.y, b.k, d0, d1); }
};

struct RectDistanceShape : RectListShape {
    static C2D_DEV void record(Obj& a, Obj& b, uint4& d0, uint4& d1)
    {
        float ax[4], ay[4], bx[4], by[4];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            ax[v] = a.r[2 * v]; ay[v] = a.r[2 * v + 1];
            bx[v] = b.r[2 * v]; by[v] = b.r[2 * v + 1];
        }
        distance_record<4>(ax, ay, 4, bx, by, 4, d0, d1);
    }
};

// The query of listed_pairs (the W of pair_list_kernel): starts as the BAD_PAIR record; a hit pair gets {0, (0, 0), (0, 0), 0xFFFF, 0xFFFF, 1, 0}.
template <class S>
struct DistanceWork {
    uint4 d0 = make_uint4(0u, 0u, 0u, 0u), d1 = make_uint4(0u, kDistanceNone, (uint32_t)C2D_DISTANCE_BAD_PAIR << 8, 0u);
    C2D_DEV void pair(const typename S::Obj& a_in, const typename S::Obj& b_in, bool valid)
    {
        const bool hit = S::collide(a_in, b_in);
        uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = make_uint4(0u, kDistanceNone, 1u, 0u);
        if (__ballot(valid && !hit) != 0ull) {   // (wave-uniform) a wave all of whose pairs are hit has no candidate to look at
            typename S::Obj a = a_in, b = b_in;
            uint4 s0, s1;
            S::record(a, b, s0, s1);
            if (!hit) {
                v0 = s0;
                v1 = s1;
            }
        }
        if (valid) {
            d0 = v0;
            d1 = v1;
        }
    }
    C2D_DEV void store(size_t p, c2d_distance* __restrict__ out) const
    {
        reinterpret_cast<uint4*>(out)[2 * p] = d0;   // d_out is 16-byte aligned (checked on the host)
        reinterpret_cast<uint4*>(out)[2 * p + 1] = d1;
    }
};

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_pair_distances(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, const uint32_t* d_pairs, size_t n_pairs,
                            const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, c2d_distance* d_out, c2d_stream stream)
{
    return poly_pair_list_call(ctx, "c2d_poly_pair_distances", a, b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const PolySetDev& A, const PolySetDev& B, int grid) {
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<PolyDistanceShape, DistanceWork<PolyDistanceShape>, c2d_distance>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream, A, B, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_out, ctx->d_async_err);
                               });
}

int c2d_rect_pair_distances(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b, const uint32_t* d_pairs,
                            size_t n_pairs, const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, c2d_distance* d_out, c2d_stream stream)
{
    return rect_pair_list_call(ctx, "c2d_rect_pair_distances", d_a, n_a, d_b, n_b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const RectListSet& A, const RectListSet& B, int grid) {
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<RectDistanceShape, DistanceWork<RectDistanceShape>, c2d_distance>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream, A, B, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_out, ctx->d_async_err);
                               });
}

}  // extern "C"
