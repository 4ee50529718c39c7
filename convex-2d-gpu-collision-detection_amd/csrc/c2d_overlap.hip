// c2d_overlap.hip — overlap queries for gfx950 (MI355X): for each listed pair (A_i, B_j) the boolean of the pairwise test and, when
// the pair is hit, the area of A ∩ B with its centroid, the two shapes' own areas and the IoU (c2d_poly_pair_overlaps,
// c2d_rect_pair_overlaps; include/c2d.h "overlap queries").
//
// The rule (the contract of include/c2d.h).  The area and the first moments of A ∩ B are a boundary integral, and the boundary of
// A ∩ B is made of the parts of A's edges that lie inside B and the parts of B's edges that lie inside A: no intersection polygon is
// built, so nothing is indexed at run time.  Everything is binary32 and unfused, in the frame of r = A's vertex 0:
//     sA, sB        the signs of the two shoelace sums (either winding is taken); area_a = 0.5 * |sum_A|
//     side 0 / 1    every edge p0 -> p1 of A (of B) is clipped to [t0, t1] in [0, 1] by the half-planes of B's (A's) edges q0 -> q1:
//                   g = q1 - q0 (a zero g imposes nothing), num = sQ * cross(g, p0 - q0), den = sQ * cross(g, p1 - p0);
//                   den > 0: t0 = max(t0, -num / den); den < 0: t1 = min(t1, -num / den); den == 0: the edge lives on if num > 0,
//                   and, on side 0 alone, if num == 0 and the two edges run the same way.  Where a quotient moves t0 or t1 the
//                   piece's end becomes the crossing X of the two edges, and X is one point for both sides: p0 + t * e on A's
//                   edge, which side 1 computes by side 0's operations on the same operands, so that the pieces close a loop
//     on one line   all four of cross(g, p0 - q0), cross(g, p1 - q0), cross(e, q0 - p0), cross(e, q1 - p0) within 8 u D (|x| + |y|)
//                   of 0 (the same four expressions on both sides): edges that run opposite ways are dropped; of two that run
//                   the same way A's is the boundary where it is inside B's half-plane and B's elsewhere, split, where A's edge
//                   passes through, at da / (da - db) of A's edge (da, db: its ends against B's half-plane)
//     a piece       a surviving edge with t0 < t1, from a to b (an end that no clip moved is the vertex itself), c = sP * cross(a, b);
//                   S += c, Mx += (a.x + b.x) * c, My += (a.y + b.y) * c
//     the record    area = clamp(0.5 * S, 0, min(area_a, area_b)), centroid = r + M / (3 * S), iou = area / (area_a + area_b - area)
//
// One pair per lane on the frame of c2d_pair_list.hpp, which also holds the kernel and, in its list shapes, the pairwise boolean
// (S::collide): this file adds the rule's record to those shapes and keeps the query.  The lanes of a wave hold unrelated pairs, so
// the vertices stay in registers and every vertex index is a compile-time slot, as in c2d_distance.hip: the clipped polygon is
// turned by one slot per trip, the clipping polygon's edges are unrolled, and the clipped polygon's padded edges are masked out of
// the sums.  The rule and the record live in c2d_overlap_rule.hpp.
#include "c2d_overlap_rule.hpp"
#include "c2d_pair_list.hpp"

namespace c2d {

static_assert(sizeof(c2d_overlap) == 32 && offsetof(c2d_overlap, iou) == 4 && offsetof(c2d_overlap, cx) == 8 && offsetof(c2d_overlap, cy) == 12 &&
                  offsetof(c2d_overlap, area_a) == 16 && offsetof(c2d_overlap, area_b) == 20 && offsetof(c2d_overlap, hit) == 24 &&
                  offsetof(c2d_overlap, flags) == 25 && offsetof(c2d_overlap, pieces_a) == 26 && offsetof(c2d_overlap, pieces_b) == 27 &&
                  offsetof(c2d_overlap, reserved) == 28,
              "the kernel stores an overlap as two halves of four dwords");

// The shapes of c2d_pair_list.hpp with what the overlap kernel adds:
//   S::frame(a, b, o)         both objects shifted to A's vertex 0, and the two shoelace sums (every pair needs them)
//   S::clip(a, b, wanted, o)  the boundary integral of a shifted pair (a and b are turned and restored)
struct PolyOverlapShape : PolyListShape {
    static C2D_DEV void frame(Obj& a, Obj& b, OverlapPair& o)
    {
        overlap_shift<C2D_POLY_KMAX>(a.x, a.y, b.x, b.y, o.rx, o.ry);
        o.sum_a = overlap_shoelace<C2D_POLY_KMAX>(a.x, a.y, a.k);
        o.sum_b = overlap_shoelace<C2D_POLY_KMAX>(b.x, b.y, b.k);
    }
    static C2D_DEV void clip(Obj& a, Obj& b, bool wanted, OverlapPair& o) { overlap_clip<C2D_POLY_KMAX>(a.x, a.y, a.k, b.x, b.y, b.k, wanted, o); }
};

struct RectOverlapShape : RectListShape {
    struct Obj {
        float x[4], y[4];
    };
    static C2D_DEV void load(const Set& X, size_t i, Obj& o)
    {
#pragma unroll
        for (int v = 0; v < 4; v++) {
            o.x[v] = X.p[2 * v][i];
            o.y[v] = X.p[2 * v + 1][i];
        }
    }
    static C2D_DEV bool collide(const Obj& a, const Obj& b)
    {
        float r1[8], r2[8];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            r1[2 * v] = a.x[v]; r1[2 * v + 1] = a.y[v];
            r2[2 * v] = b.x[v]; r2[2 * v + 1] = b.y[v];
        }
        return rect_collide(r1, r2);
    }
    static C2D_DEV void frame(Obj& a, Obj& b, OverlapPair& o)
    {
        overlap_shift<4>(a.x, a.y, b.x, b.y, o.rx, o.ry);
        o.sum_a = overlap_shoelace<4>(a.x, a.y, 4);
        o.sum_b = overlap_shoelace<4>(b.x, b.y, 4);
    }
    static C2D_DEV void clip(Obj& a, Obj& b, bool wanted, OverlapPair& o) { overlap_clip<4>(a.x, a.y, 4, b.x, b.y, 4, wanted, o); }
};

// The query of listed_pairs (the W of pair_list_kernel): starts as the BAD_PAIR record.
template <class S>
struct OverlapWork {
    uint4 d0 = make_uint4(0u, 0u, 0u, 0u), d1 = make_uint4(0u, 0u, (uint32_t)C2D_OVERLAP_BAD_PAIR << 8, 0u);
    C2D_DEV void pair(const typename S::Obj& a_in, const typename S::Obj& b_in, bool valid)
    {
        const bool hit = S::collide(a_in, b_in);
        typename S::Obj a = a_in, b = b_in;
        OverlapPair o;
        S::frame(a, b, o);
        const bool wanted = valid && hit;
        if (__ballot(wanted) != 0ull) S::clip(a, b, wanted, o);   // (wave-uniform) a wave none of whose pairs is hit has nothing to clip
        uint4 v0, v1;
        overlap_halves(o, hit, v0, v1);
        if (valid) {
            d0 = v0;
            d1 = v1;
        }
    }
    C2D_DEV void store(size_t p, c2d_overlap* __restrict__ out) const
    {
        reinterpret_cast<uint4*>(out)[2 * p] = d0;   // d_out is 16-byte aligned (checked on the host)
        reinterpret_cast<uint4*>(out)[2 * p + 1] = d1;
    }
};

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_pair_overlaps(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, const uint32_t* d_pairs, size_t n_pairs,
                           const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, c2d_overlap* d_out, c2d_stream stream)
{
    return poly_pair_list_call(ctx, "c2d_poly_pair_overlaps", a, b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const PolySetDev& A, const PolySetDev& B, int grid) {
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<PolyOverlapShape, OverlapWork<PolyOverlapShape>, c2d_overlap>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream, A, B, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_out, ctx->d_async_err);
                               });
}

int c2d_rect_pair_overlaps(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b, const uint32_t* d_pairs,
                           size_t n_pairs, const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, c2d_overlap* d_out, c2d_stream stream)
{
    return rect_pair_list_call(ctx, "c2d_rect_pair_overlaps", d_a, n_a, d_b, n_b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const RectListSet& A, const RectListSet& B, int grid) {
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<RectOverlapShape, OverlapWork<RectOverlapShape>, c2d_overlap>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream, A, B, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_out, ctx->d_async_err);
                               });
}

}  // extern "C"
