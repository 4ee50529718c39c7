// c2d_contact.hip — contact queries for gfx950 (MI355X): for each listed pair (A_i, B_j) the minimum-translation contact over the
// pairwise test's own axes — a signed depth, a unit normal from A to B, the axis it came from — and the boolean of the pairwise
// test itself (c2d_poly_pair_contacts, c2d_rect_pair_contacts; include/c2d.h) — and, for polygons, the same contact
// with its manifold of up to two points in one fused call (c2d_poly_pair_manifolds; poly_manifold below).
//
// The rule (the contract of include/c2d.h), per axis n in axis order, with [minA, maxA] and [minB, maxB] the projection intervals
// the pairwise test computes on n:
//     o1 = maxA - minB,  o2 = maxB - minA,  o = o1 <= o2 ? o1 : o2,  len2 = n.x * n.x + n.y * n.y  (unfused)
//     unusable: len2 == 0, or d = o / sqrt(len2) is NaN;   otherwise the first axis with the smallest d (strict <) wins:
//     depth = d, normal = +-n / sqrt(len2) with + when o1 <= o2.
// One pair per lane; the lanes of a wave hold unrelated pairs, so every loop runs over all vertex slots with compile-time indices
// (c2d_poly_pair.hpp).  The pair list is row-major: the lanes of a wave mostly share their row, so A is loaded through one
// wave-uniform index when they all do; B is a gather (listed_pairs, c2d_pair_list.hpp, which the distance and swept queries share).
// The walk over the axes, with the pairwise boolean it returns, is that header's too (S::axes of its list shapes; the swept queries
// run the same walk), and so is the kernel: this file keeps the two picks, the manifold and the query.  Each contact leaves as one
// 16-byte store.
//
// One square root and one division per PAIR instead of one per axis (DESIGN.md §5.11 has the proof).  A first pass estimates every
// axis's d as q = o * v_rsq_f32(len2) and keeps the smallest and the second smallest estimate.  With len2 in [2^-100, 2^100] and
// |o| < 2^60, q and the contract's d each lie within 2^-22 |t| + 2^-149 of the real quotient t, hence d in
// [q - 2^-20 |q| - 2^-147, q + 2^-20 |q| + 2^-147].  When the lower end of the runner-up's range is above the upper end of the
// best one's (evaluated with margins of 2^-19 |q| + 1e-36, which also cover their own rounding), every other axis's d is strictly
// larger than the best axis's, so the sequential rule picks that axis whatever the rounded values are, and its d and normal are
// computed once with the correctly rounded sqrt and divisions.  A pair with an axis outside those ranges, a NaN anywhere, or two
// estimates too close to call (ties: parallel edges, touching or equal shapes) runs the sequential rule itself in a second pass.
#include "c2d_pair_list.hpp"

namespace c2d {

static_assert(sizeof(c2d_contact) == 16 && offsetof(c2d_contact, axis) == 12 && offsetof(c2d_contact, hit) == 14 && offsetof(c2d_contact, flags) == 15,
              "the kernel stores a contact as four dwords");

constexpr uint32_t kContactNoAxis = 0xFFFFu;
constexpr uint32_t kManifoldNoFeature = 0xFFFFu;

static_assert(sizeof(c2d_manifold) == 32 && offsetof(c2d_manifold, x1) == 12 && offsetof(c2d_manifold, y1) == 16 && offsetof(c2d_manifold, feature) == 24 &&
                  offsetof(c2d_manifold, count) == 26 && offsetof(c2d_manifold, flags) == 27 && offsetof(c2d_manifold, reserved) == 28,
              "the kernel stores a manifold as two halves of four dwords");

// what a pick leaves behind: the contact without its `hit`
struct ContactValue {
    float depth, nx, ny;
    uint32_t axis, flags;
};

// The sequential rule itself: every axis pays the correctly rounded sqrt and division.
struct ExactPick {
    float d = __builtin_inff(), nx = 0.0f, ny = 0.0f, len = 1.0f;
    uint32_t axis = kContactNoAxis;
    bool pos = true;
    C2D_DEV void add(uint32_t axis_, float nx_, float ny_, float o1, float o2)
    {
        const bool p = o1 <= o2;
        const float o = p ? o1 : o2;
        const float len2 = nx_ * nx_ + ny_ * ny_;
        const float l = __builtin_sqrtf(len2);
        const float dd = o / l;
        if (len2 != 0.0f && !__builtin_isnan(dd) && (axis == kContactNoAxis || dd < d)) {
            d = dd; nx = nx_; ny = ny_; len = l; axis = axis_; pos = p;
        }
    }
    C2D_DEV ContactValue value() const
    {
        if (axis == kContactNoAxis) return ContactValue{__builtin_inff(), 0.0f, 0.0f, kContactNoAxis, (uint32_t)C2D_CONTACT_NO_AXIS};
        const float ux = nx / len, uy = ny / len;
        return ContactValue{d, pos ? ux : -ux, pos ? uy : -uy, axis, 0u};
    }
};

// The first pass: estimates only.  decided() says whether the estimates already name the axis the sequential rule picks.
struct FastPick {
    float q1 = __builtin_inff(), q2 = __builtin_inff();   // the smallest estimate and the smallest of all others
    float o = 0.0f, nx = 0.0f, ny = 0.0f, len2 = 1.0f;    // the axis of q1
    uint32_t axis = kContactNoAxis;
    bool pos = true, hard = false;
    C2D_DEV void add(uint32_t axis_, float nx_, float ny_, float o1, float o2)
    {
        const bool p = o1 <= o2;
        const float o_ = p ? o1 : o2;
        const float l2 = nx_ * nx_ + ny_ * ny_;
        const bool live = l2 != 0.0f;   // (a NaN is live, and hard)
        hard |= live && !(l2 >= 0x1p-100f && l2 <= 0x1p100f && __builtin_fabsf(o_) < 0x1p60f);
        const float q = live ? o_ * __builtin_amdgcn_rsqf(l2) : __builtin_inff();
        if (q < q1) {
            q2 = q1;
            q1 = q; o = o_; nx = nx_; ny = ny_; len2 = l2; axis = axis_; pos = p;
        } else {
            q2 = __builtin_fminf(q2, q);
        }
    }
    C2D_DEV bool decided() const
    {
        if (hard) return false;
        if (axis == kContactNoAxis || q2 == __builtin_inff()) return true;   // no live axis at all, or exactly one
        const float lo2 = q2 - __builtin_fabsf(q2) * 0x1p-19f - 1e-36f, hi1 = q1 + __builtin_fabsf(q1) * 0x1p-19f + 1e-36f;
        return lo2 > hi1;
    }
    C2D_DEV ContactValue value() const   // (decided() holds)
    {
        if (axis == kContactNoAxis) return ContactValue{__builtin_inff(), 0.0f, 0.0f, kContactNoAxis, (uint32_t)C2D_CONTACT_NO_AXIS};
        const float l = __builtin_sqrtf(len2);
        const float ux = nx / l, uy = ny / l;
        return ContactValue{o / l, pos ? ux : -ux, pos ? uy : -uy, axis, 0u};
    }
};

// ---- the manifold of one polygon pair on its winning axis (include/c2d.h "contact manifolds") ---------------------
// e, (nx, ny), len = sqrt(len2) and pos = (o1 <= o2) are the winning axis as the contact rule saw it.  Every vertex index is a
// compile-time slot: the deepest vertex, its two neighbours and the reference edge are carried through selects.  Slots >= k repeat
// vertex 0 (poly_load), so "next of k - 1" is slot k (slot 16 is slot 0), a padding slot never beats vertex 0 under the strict
// compare, and the interval of R over all 16 slots is the contact rule's own.  The record leaves as two dwordx4 halves:
// m0 = {x0, y0, d0, x1}, m1 = {y1, d1, feature | count << 16 | flags << 24, 0}.
C2D_DEV void poly_manifold(const PolyObj& A, const PolyObj& B, uint32_t e, float nx, float ny, float len, bool pos, uint4& m0, uint4& m1)
{
    constexpr int K = C2D_POLY_KMAX;
    const float inf = __builtin_inff();
    const bool ref_b = e >= (uint32_t)A.k;
    const int r = (int)e - (ref_b ? A.k : 0);
    const int kI = ref_b ? A.k : B.k;
    const bool up = ref_b != pos;   // sigma > 0: (R is A) == pos
    PolyObj R, I;
#pragma unroll
    for (int f = 0; f < K; f++) {
        R.x[f] = ref_b ? B.x[f] : A.x[f];
        R.y[f] = ref_b ? B.y[f] : A.y[f];
        I.x[f] = ref_b ? A.x[f] : B.x[f];
        I.y[f] = ref_b ? A.y[f] : B.y[f];
    }
    // step 1: the face value F, from R's interval; step 4: the reference edge's two vertices (slots r and r + 1)
    float mnr = inf, mxr = -inf;
    float rx0 = R.x[0], ry0 = R.y[0], rx1 = R.x[0], ry1 = R.y[0];
    const int r1 = (r + 1) & (K - 1);
#pragma unroll
    for (int f = 0; f < K; f++) {
        poly_minmax(nx, ny, R.x[f], R.y[f], mnr, mxr);
        if (f == r) { rx0 = R.x[f]; ry0 = R.y[f]; }
        if (f == r1) { rx1 = R.x[f]; ry1 = R.y[f]; }
    }
    const float face = up ? mxr : mnr;
    // step 2: the deepest vertex of I, first of equals, a NaN never replaces
    float pr[K];
#pragma unroll
    for (int f = 0; f < K; f++) pr[f] = nx * I.x[f] + ny * I.y[f];
    int w = 0;
    float pw = pr[0];
#pragma unroll
    for (int f = 1; f < K; f++) {
        const bool deeper = up ? pr[f] < pw : pr[f] > pw;
        w = deeper ? f : w;
        pw = deeper ? pr[f] : pw;
    }
    // step 3: its neighbours, and the other end u of the incident edge
    const int prv = w == 0 ? kI - 1 : w - 1, nxt = (w + 1) & (K - 1);
    float xw = I.x[0], yw = I.y[0], xn = I.x[0], yn = I.y[0], pn = pr[0], xp = I.x[0], yp = I.y[0], pp = pr[0];
#pragma unroll
    for (int f = 0; f < K; f++) {
        if (f == w) { xw = I.x[f]; yw = I.y[f]; }
        if (f == nxt) { xn = I.x[f]; yn = I.y[f]; pn = pr[f]; }
        if (f == prv) { xp = I.x[f]; yp = I.y[f]; pp = pr[f]; }
    }
    const bool back = up ? pp < pn : pp > pn;
    const float xu = back ? xp : xn, yu = back ? yp : yn;
    const uint32_t feature = (uint32_t)(back ? prv : w);
    // step 4: the slab of the reference edge
    const float tau0 = ny * rx0 - nx * ry0, tau1 = ny * rx1 - nx * ry1;
    const float lo = tau0 <= tau1 ? tau0 : tau1, hi = tau0 <= tau1 ? tau1 : tau0;
    // step 5: each end against the original other end
    const float tw = ny * xw - nx * yw, tu = ny * xu - nx * yu;
    const bool c0 = tw < lo || tw > hi, c1 = tu < lo || tu > hi;
    const float s0 = ((tw < lo ? lo : hi) - tw) / (tu - tw), s1 = ((tu < lo ? lo : hi) - tu) / (tw - tu);
    const float cx0 = xw + (xu - xw) * s0, cy0 = yw + (yu - yw) * s0;
    const float cx1 = xu + (xw - xu) * s1, cy1 = yu + (yw - yu) * s1;
    const bool single = kI == 1;
    const bool outside = !single && ((tw < lo && tu < lo) || (tw > hi && tu > hi));
    const bool two = !single && !outside;
    const float x0 = two && c0 ? cx0 : xw, y0 = two && c0 ? cy0 : yw;
    const float x1 = c1 ? cx1 : xu, y1 = c1 ? cy1 : yu;
    // step 6: the depths, from the final coordinates
    const float p0 = nx * x0 + ny * y0, p1 = nx * x1 + ny * y1;
    const float d0 = (up ? face - p0 : p0 - face) / len, d1 = (up ? face - p1 : p1 - face) / len;
    const uint32_t flags = (ref_b ? (uint32_t)C2D_MANIFOLD_REF_IS_B : 0u) | (two && c0 ? (uint32_t)C2D_MANIFOLD_P0_CLIPPED : 0u) |
                           (two && c1 ? (uint32_t)C2D_MANIFOLD_P1_CLIPPED : 0u) | (outside ? (uint32_t)C2D_MANIFOLD_OUTSIDE_SLAB : 0u);
    m0 = make_uint4(__float_as_uint(x0), __float_as_uint(y0), __float_as_uint(d0), two ? __float_as_uint(x1) : 0u);
    m1 = make_uint4(two ? __float_as_uint(y1) : 0u, two ? __float_as_uint(d1) : 0u, (single ? 0u : feature) | (two ? 2u << 16 : 1u << 16) | (flags << 24), 0u);
}

// The query of listed_pairs (c2d_pair_list.hpp; the W of its pair_list_kernel): the contact of one pair per lane.  kManifold
// (polygons): the manifold of the pair goes to man[p] as well, as two more 16-byte stores; without it the kernel has no such
// argument and the routine is the contact kernel as it was.
template <class S, bool kManifold>
struct ContactWork {
    uint4 word = make_uint4(0u, 0u, 0u, kContactNoAxis | ((uint32_t)C2D_CONTACT_BAD_PAIR << 24));   // depth 0, normal (0, 0), hit 0
    uint4 m0 = make_uint4(0u, 0u, 0u, 0u), m1 = make_uint4(0u, 0u, kManifoldNoFeature, 0u);          // no point, no feature
    C2D_DEV void pair(const typename S::Obj& a, const typename S::Obj& b, bool valid)
    {
        FastPick fast;
        const bool hit = S::axes(a, b, fast);
        ContactValue c;
        float wnx = 0.0f, wny = 0.0f, wlen = 1.0f;   // the winning axis as the rule saw it: raw normal, sqrt(len2), o1 <= o2
        bool wpos = true;
        if (fast.decided()) {
            c = fast.value();
            if constexpr (kManifold) {
                wnx = fast.nx; wny = fast.ny; wlen = __builtin_sqrtf(fast.len2); wpos = fast.pos;
            }
        } else {
            ExactPick exact;
            (void)S::axes(a, b, exact);
            c = exact.value();
            if constexpr (kManifold) {
                wnx = exact.nx; wny = exact.ny; wlen = exact.len; wpos = exact.pos;
            }
        }
        if (valid)
            word = make_uint4(__float_as_uint(c.depth), __float_as_uint(c.nx), __float_as_uint(c.ny), c.axis | (hit ? 1u << 16 : 0u) | (c.flags << 24));
        if constexpr (kManifold) {
            uint4 v0, v1;
            poly_manifold(a, b, c.axis, wnx, wny, wlen, wpos, v0, v1);   // (axis 0xFFFF: computes on axis (0, 0) and is dropped)
            if (valid && c.axis != kContactNoAxis) {
                m0 = v0;
                m1 = v1;
            }
        }
    }
    C2D_DEV void store(size_t p, c2d_contact* __restrict__ out, c2d_manifold* __restrict__ man = nullptr) const
    {
        reinterpret_cast<uint4*>(out)[p] = word;   // d_out is 16-byte aligned (checked on the host)
        if constexpr (kManifold) {
            reinterpret_cast<uint4*>(man)[2 * p] = m0;
            reinterpret_cast<uint4*>(man)[2 * p + 1] = m1;
        }
    }
};

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_poly_pair_contacts(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, const uint32_t* d_pairs, size_t n_pairs,
                           const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, c2d_contact* d_out, c2d_stream stream)
{
    return poly_pair_list_call(ctx, "c2d_poly_pair_contacts", a, b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const PolySetDev& A, const PolySetDev& B, int grid) {
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<PolyListShape, ContactWork<PolyListShape, false>, c2d_contact>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream, A, B, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_out, ctx->d_async_err);
                               });
}

int c2d_poly_pair_manifolds(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, const uint32_t* d_pairs, size_t n_pairs,
                            const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, c2d_contact* d_contacts, c2d_manifold* d_manifolds,
                            c2d_stream stream)
{
    return poly_pair_list_call(ctx, "c2d_poly_pair_manifolds", a, b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_contacts, d_manifolds},
                               [&](const PolySetDev& A, const PolySetDev& B, int grid) {
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<PolyListShape, ContactWork<PolyListShape, true>, c2d_contact, c2d_manifold>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream, A, B, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_contacts, d_manifolds, ctx->d_async_err);
                               });
}

int c2d_rect_pair_contacts(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b, const uint32_t* d_pairs,
                           size_t n_pairs, const unsigned long long* d_n_pairs, size_t row_base, size_t col_base, c2d_contact* d_out, c2d_stream stream)
{
    return rect_pair_list_call(ctx, "c2d_rect_pair_contacts", d_a, n_a, d_b, n_b, d_pairs, n_pairs, d_n_pairs, row_base, col_base, {d_out},
                               [&](const RectListSet& A, const RectListSet& B, int grid) {
                                   hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_list_kernel<RectListShape, ContactWork<RectListShape, false>, c2d_contact>),
                                                      dim3(grid), dim3(kPairListBlock), 0, (hipStream_t)stream, A, B, d_pairs, n_pairs, d_n_pairs,
                                                      row_base, col_base, d_out, ctx->d_async_err);
                               });
}

}  // extern "C"
