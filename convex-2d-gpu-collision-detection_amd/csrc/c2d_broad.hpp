// c2d_broad.hpp — the broad-phase pair search as one pipeline over a shape policy.
//
// The pipeline of c2d_broad.hip (boxes, grid, sort, count, scan, emit) knows three things about the objects it searches, and a
// shape policy S supplies them:
//   S::Set                              the device-side description of one set (a kernel argument)
//   S::Obj                              one object in registers
//   S::load(set, i, obj)                object i of the set
//   S::box(set, i, box)                 its conservative box (kBroadRegular), or kBroadWild: tested against everything, or
//                                       kBroadAbsent: in no pair at all
//   S::collide(a, b)                    the exact test of (A_i, B_j), per lane
// The shape-dependent kernels are templates in this header; the grid, the key pass, the radix sort, the tile scan, the scene header
// and the scratch layout are c2d_broad.hip's and exist once.  c2d_broad.hip instantiates the pipeline for rectangles,
// c2d_poly_broad.hip for convex polygons.
#pragma once

#include "c2d_cross.hpp"
#include "c2d_math.hpp"
#include "c2d_wave.hpp"

namespace c2d {

constexpr int kBroadBlock = 256;           // threads per block of the per-object and per-row kernels
constexpr int kHistBins = 1024;            // box extents by their float bits >> 21: exponent and two mantissa bits
constexpr uint32_t kAbsentKey = 0xffffffffu;   // sort key of an absent object of B: behind the wild ones
constexpr uint32_t kWildKey = 0xfffffffeu;     // sort key of a wild object of B: behind every cell key
constexpr int kShortHits = 16;             // hits a row may have for the short emit path (LDS sort)
constexpr int kMidHits = 512;              // hits a listed regular row may have for the wave path of the long emit kernel
constexpr uint32_t kCandidateCap = 1024;   // sorted entries a row may walk in the short path before it goes to the list
constexpr unsigned long long kUncounted = ~0ull;
constexpr int kLongGrid = 2048;            // blocks of the listed-row kernels (grid-stride over the list)
constexpr uint32_t kMaxCells = 65535;      // cells per axis: keys cy * gx + cx stay below kWildKey

enum { kBroadRegular = 0, kBroadWild = 1, kBroadAbsent = 2 };   // what S::box says of an object

// scene constants of one call, in the scratch header
struct BroadGrid {
    unsigned int hist[kHistBins];   // extent histogram of the objects that got a box
    unsigned int lo_x, lo_y, hi_x, hi_y;   // bounds of the boxes narrower than S, as order-preserving keys
    unsigned int n_reg_b;           // regular objects of B (the sorted keys below kWildKey)
    unsigned int n_long;            // rows in the long-row list
    float s;                        // cell size before the 65535 cap
    float pad_;
    double x0, y0, ix, iy;          // cell of v: floor((v - x0) * ix), clamped to [0, gx - 1]
    unsigned int gx, gy;
};

// the float next to f towards -inf / +inf (f is not NaN)
C2D_DEV float float_below(float f)
{
    const unsigned int b = __float_as_uint(f);
    return f == 0.0f ? __uint_as_float(0x80000001u) : __uint_as_float(f > 0.0f ? b - 1u : b + 1u);
}
C2D_DEV float float_above(float f)
{
    const unsigned int b = __float_as_uint(f);
    return f == 0.0f ? __uint_as_float(0x00000001u) : __uint_as_float(f > 0.0f ? b + 1u : b - 1u);
}
// d rounded to float downwards / upwards (beyond the float range: +-inf on the far side)
C2D_DEV float round_down(double d)
{
    const float f = (float)d;
    return (double)f > d ? float_below(f) : f;
}
C2D_DEV float round_up(double d)
{
    const float f = (float)d;
    return (double)f < d ? float_above(f) : f;
}

// The widening of an object's own interval on one of its axes a: W = |a|_1 (2^-21 C + 2^-66) + 2^-140 with C the object's largest
// |coordinate|.
C2D_DEV double broad_slab_widening(double n1, double C) { return n1 * (0x1p-21 * C + 0x1p-66) + 0x1p-140; }

// The box of the parallelogram U = { p : a_k . p in [slo_k, shi_k], k = 0, 1 } in double, rounded outward to float; false when the
// axes are parallel (U unbounded) or the box is not finite in float.
C2D_DEV bool broad_box_of_slabs(const double (&ax)[2], const double (&ay)[2], const double (&slo)[2], const double (&shi)[2], float4& box)
{
    const double det = ax[0] * ay[1] - ay[0] * ax[1];
    if (!(det != 0.0)) return false;
    const double adet = __builtin_fabs(det);
    // p = (x, y) with a_0 . p = s, a_1 . p = t:  x = (s ay1 - t ay0) / det,  y = (t ax0 - s ax1) / det.  Each is linear in (s, t),
    // so its range over the parallelogram is the sum of the ranges of its two terms; 2^-48 of the terms' size covers the
    // roundings of the products, the sum and the division (each 2^-53 relative).
    double xr[2], yr[2];
    {
        const double u0 = slo[0] * ay[1], u1 = shi[0] * ay[1], v0 = -(slo[1] * ay[0]), v1 = -(shi[1] * ay[0]);
        const double nlo = __builtin_fmin(u0, u1) + __builtin_fmin(v0, v1), nhi = __builtin_fmax(u0, u1) + __builtin_fmax(v0, v1);
        const double m = 0x1p-48 * (__builtin_fmax(__builtin_fabs(u0), __builtin_fabs(u1)) + __builtin_fmax(__builtin_fabs(v0), __builtin_fabs(v1))) / adet;
        xr[0] = (det > 0.0 ? nlo : nhi) / det - m;
        xr[1] = (det > 0.0 ? nhi : nlo) / det + m;
    }
    {
        const double u0 = slo[1] * ax[0], u1 = shi[1] * ax[0], v0 = -(slo[0] * ax[1]), v1 = -(shi[0] * ax[1]);
        const double nlo = __builtin_fmin(u0, u1) + __builtin_fmin(v0, v1), nhi = __builtin_fmax(u0, u1) + __builtin_fmax(v0, v1);
        const double m = 0x1p-48 * (__builtin_fmax(__builtin_fabs(u0), __builtin_fabs(u1)) + __builtin_fmax(__builtin_fabs(v0), __builtin_fabs(v1))) / adet;
        yr[0] = (det > 0.0 ? nlo : nhi) / det - m;
        yr[1] = (det > 0.0 ? nhi : nlo) / det + m;
    }
    box = make_float4(round_down(xr[0]), round_down(yr[0]), round_up(xr[1]), round_up(yr[1]));
    return __builtin_isfinite(box.x) && __builtin_isfinite(box.y) && __builtin_isfinite(box.z) && __builtin_isfinite(box.w);
}

// A wild object's box is four NaNs; an absent object's box is (NaN, 0, 0, 0): wild to every stage that only sorts and bounds boxes,
// and told apart where objects are tested.
C2D_DEV bool box_wild(const float4& b) { return __builtin_isnan(b.x); }
C2D_DEV bool box_absent(const float4& b) { return __builtin_isnan(b.x) && !__builtin_isnan(b.y); }
C2D_DEV bool boxes_meet(const float4& a, const float4& b) { return a.x <= b.z && b.x <= a.z && a.y <= b.w && b.y <= a.w; }
C2D_DEV float box_extent(const float4& b) { return __builtin_fmaxf(b.z - b.x, b.w - b.y); }

// the cell of coordinate v: monotone non-decreasing in v, which is all the query's correctness needs
C2D_DEV uint32_t cell_of(float v, double v0, double inv, uint32_t g)
{
    double t = ((double)v - v0) * inv;
    t = t > 0.0 ? __builtin_floor(t) : 0.0;
    const double top = (double)(g - 1);
    return (uint32_t)(t < top ? t : top);
}

// The cells whose sorted entries a query with the regular box `ba` has to look at: B_j overlaps ba only if cx(min x_j) is in
// [cx(min x_i) - 1, cx(max x_i)], and the same in y.  The - 1: a sorted box is filed under the cell of its low corner and spans at
// most two cells, and cell_of is monotone.  (gx, gy: the caller's copies of g->gx, g->gy.)
struct BroadCells { uint32_t cx0, cx1, cy0, cy1; };
C2D_DEV BroadCells broad_cell_range(const BroadGrid* g, uint32_t gx, uint32_t gy, float4 ba)
{
    uint32_t cx0 = cell_of(ba.x, g->x0, g->ix, gx), cx1 = cell_of(ba.z, g->x0, g->ix, gx);
    uint32_t cy0 = cell_of(ba.y, g->y0, g->iy, gy), cy1 = cell_of(ba.w, g->y0, g->iy, gy);
    cx0 = cx0 ? cx0 - 1u : 0u;
    cy0 = cy0 ? cy0 - 1u : 0u;
    return BroadCells{cx0, cx1, cy0, cy1};
}

// 1. boxes (NaN box = wild) and the extent histogram
template <class S>
__global__ __launch_bounds__(kBroadBlock) void broad_box_kernel(typename S::Set X, size_t n, float4* __restrict__ box, BroadGrid* __restrict__ g)
{
    __shared__ unsigned int hist[kHistBins];
    for (int b = threadIdx.x; b < kHistBins; b += kBroadBlock) hist[b] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBroadBlock) {
        float4 b;
        const int kind = S::box(X, i, b);
        if (kind == kBroadRegular) {
            atomicAdd(&hist[__float_as_uint(box_extent(b)) >> 21], 1u);
        } else {
            const float q = __builtin_nanf("");
            b = kind == kBroadAbsent ? make_float4(q, 0.0f, 0.0f, 0.0f) : make_float4(q, q, q, q);
        }
        box[i] = b;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kHistBins; b += kBroadBlock)
        if (hist[b]) atomicAdd(&g->hist[b], hist[b]);
}

template <class S>
struct BroadQuery {
    typename S::Set A, B;
    const float4* box_a;        // [n_a] (NaN: wild or absent)
    const float4* box_b;        // [n_b], index order
    const uint32_t* keys;       // [n_b] sorted keys: regular ones first, then kWildKey, then kAbsentKey
    const uint32_t* idx;        // [n_b] index of each sorted key
    const float4* sbox;         // [n_b] boxes in key order
    const BroadGrid* g;
    size_t n_a, n_b;
    int upper;
};

// first position in keys[0, n) with keys[pos] >= key
C2D_DEV uint32_t lower_bound_u32(const uint32_t* __restrict__ keys, uint32_t n, uint32_t key)
{
    uint32_t lo = 0, len = n;
    while (len > 0) {
        const uint32_t half = len >> 1;
        if (keys[lo + half] < key) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// The short query of regular row i: every sorted column in the cells that can hold an overlapping box, then every wild column.
// visit(j) is called for each colliding tested column (in key order, then wild columns in index order).  Returns false when the
// row walked more than kCandidateCap sorted entries (the caller then leaves the row to the list).
template <class S, class Visit>
C2D_DEV bool broad_row_query(const BroadQuery<S>& q, size_t i, const float4& ba, const typename S::Obj& ra, uint32_t n_reg, Visit visit)
{
    const BroadGrid* g = q.g;
    const uint32_t gx = g->gx, gy = g->gy;
    // broad_cell_range's cells, spelt out: through the helper this walk's registers come out renamed in every count and emit kernel
    uint32_t cx0 = cell_of(ba.x, g->x0, g->ix, gx), cx1 = cell_of(ba.z, g->x0, g->ix, gx);
    uint32_t cy0 = cell_of(ba.y, g->y0, g->iy, gy), cy1 = cell_of(ba.w, g->y0, g->iy, gy);
    cx0 = cx0 ? cx0 - 1u : 0u;
    cy0 = cy0 ? cy0 - 1u : 0u;
    uint32_t walked = 0;
    for (uint32_t cy = cy0; cy <= cy1; cy++) {
        const uint32_t k_lo = cy * gx + cx0, k_hi = cy * gx + cx1;
        for (uint32_t k = lower_bound_u32(q.keys, n_reg, k_lo); k < n_reg && q.keys[k] <= k_hi; k++) {
            if (++walked > kCandidateCap) return false;
            if (!boxes_meet(ba, q.sbox[k])) continue;
            const uint32_t j = q.idx[k];
            if (q.upper && (size_t)j <= i) continue;
            typename S::Obj rb;
            S::load(q.B, j, rb);
            if (S::collide(ra, rb)) visit(j);
        }
    }
    for (size_t k = n_reg; k < q.n_b && q.keys[k] != kAbsentKey; k++) {   // the wild tail ends where the absent objects begin
        const uint32_t j = q.idx[k];
        if (q.upper && (size_t)j <= i) continue;
        typename S::Obj rb;
        S::load(q.B, j, rb);
        if (S::collide(ra, rb)) visit(j);
    }
    return true;
}

// 7. per-row counts of regular rows; wild rows, rows over the candidate cap and rows with more than kShortHits hits go to the list.
//    An absent row has no pairs: its count is 0 and it is not listed.
template <class S>
__global__ __launch_bounds__(kBroadBlock) void broad_count_kernel(BroadQuery<S> q, unsigned long long* __restrict__ row_count,
                                                                  uint32_t* __restrict__ long_rows, BroadGrid* __restrict__ g)
{
    const uint32_t n_reg = g->n_reg_b;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < q.n_a; i += (size_t)gridDim.x * kBroadBlock) {
        const float4 ba = q.box_a[i];
        unsigned long long cnt = kUncounted;
        if (!box_wild(ba)) {
            typename S::Obj ra;
            S::load(q.A, i, ra);
            unsigned long long c = 0;
            if (broad_row_query<S>(q, i, ba, ra, n_reg, [&](uint32_t) { c++; })) cnt = c;
        } else if (box_absent(ba)) {
            cnt = 0;
        }
        row_count[i] = cnt;
        if (cnt == kUncounted || cnt > (unsigned long long)kShortHits) {
            const unsigned int slot = atomicAdd(&g->n_long, 1u);   // each row at most once: slot < n_a
            if ((size_t)slot < q.n_a) long_rows[slot] = (uint32_t)i;
        }
    }
}

// Result (i, j) in the listed-row path: boxes first where both objects are regular, the exact test otherwise.
template <class S>
C2D_DEV bool broad_pair(const BroadQuery<S>& q, const float4& ba, const typename S::Obj& ra, size_t j)
{
    const float4 bb = q.box_b[j];
    if (box_absent(bb)) return false;
    if (!box_wild(ba) && !box_wild(bb) && !boxes_meet(ba, bb)) return false;
    typename S::Obj rb;
    S::load(q.B, j, rb);
    return S::collide(ra, rb);
}

// 8. listed rows whose count is missing: one wave per row over all columns (upper: columns above the row)
template <class S>
__global__ __launch_bounds__(kBroadBlock) void broad_long_count_kernel(BroadQuery<S> q, unsigned long long* __restrict__ row_count,
                                                                       const uint32_t* __restrict__ long_rows, const BroadGrid* __restrict__ g)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_long = g->n_long;
    const size_t waves = (size_t)gridDim.x * (kBroadBlock / 64);
    for (size_t w = (size_t)blockIdx.x * (kBroadBlock / 64) + (threadIdx.x >> 6); w < n_long && w < q.n_a; w += waves) {
        const size_t i = long_rows[w];
        if (i >= q.n_a || row_count[i] != kUncounted) continue;
        const float4 ba = q.box_a[i];
        typename S::Obj ra;
        S::load(q.A, i, ra);
        unsigned long long c = 0;
        for (size_t j = (q.upper ? i + 1 : 0) + lane; j < q.n_b; j += 64) c += broad_pair<S>(q, ba, ra, j) ? 1u : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0) row_count[i] = c;
    }
}

// 10. short rows: repeat the query, sort the hits by column in LDS, write those below the capacity
template <class S>
__global__ __launch_bounds__(kBroadBlock) void broad_emit_kernel(BroadQuery<S> q, const unsigned long long* __restrict__ row_count,
                                                                 const unsigned long long* __restrict__ row_off, const BroadGrid* __restrict__ g,
                                                                 uint32_t* __restrict__ pairs, size_t capacity)
{
    __shared__ uint32_t hits[kShortHits][kBroadBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t n_reg = g->n_reg_b;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + t; i < q.n_a; i += (size_t)gridDim.x * kBroadBlock) {
        const unsigned long long cnt = row_count[i];
        const unsigned long long pos0 = row_off[i];
        const float4 ba = q.box_a[i];
        if (cnt == 0 || cnt > (unsigned long long)kShortHits || pos0 >= capacity || box_wild(ba)) continue;
        typename S::Obj ra;
        S::load(q.A, i, ra);
        uint32_t m = 0;
        const bool ok = broad_row_query<S>(q, i, ba, ra, n_reg, [&](uint32_t j) {
            if (m < (uint32_t)kShortHits) hits[m][t] = j;
            m++;
        });
        if (!ok) continue;   // over the candidate cap in the count pass too: a listed row
        if ((unsigned long long)m != cnt) continue;   // never (the count pass ran the same query); keeps the writes in the row's range
        for (uint32_t a = 1; a < m; a++) {   // insertion sort: at most kShortHits entries
            const uint32_t v = hits[a][t];
            uint32_t b = a;
            for (; b > 0 && hits[b - 1][t] > v; b--) hits[b][t] = hits[b - 1][t];
            hits[b][t] = v;
        }
        for (uint32_t a = 0; a < m && pos0 + a < capacity; a++) {
            pairs[2 * (pos0 + a)] = (uint32_t)i;
            pairs[2 * (pos0 + a) + 1] = hits[a][t];
        }
    }
}

// 11. listed rows.  A regular row with at most kMidHits hits whose query walks at most kCandidateCap sorted entries (the same
//     test as the short path's abort) repeats the grid query with one wave: lanes over the candidates, hits gathered in LDS by
//     ballot, each hit written at its rank among the row's hits.  Every other listed row (wild, crowded, or with more hits) walks all
//     columns in index order; a ballot orders each group of 64.
template <class S>
__global__ __launch_bounds__(kBroadBlock) void broad_long_emit_kernel(BroadQuery<S> q, const unsigned long long* __restrict__ row_count,
                                                                      const unsigned long long* __restrict__ row_off,
                                                                      const uint32_t* __restrict__ long_rows, const BroadGrid* __restrict__ g,
                                                                      uint32_t* __restrict__ pairs, size_t capacity)
{
    __shared__ uint32_t hits[kBroadBlock / 64][kMidHits];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_long = g->n_long, n_reg = g->n_reg_b, gx = g->gx, gy = g->gy;
    const size_t waves = (size_t)gridDim.x * (kBroadBlock / 64);
    const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
    for (size_t w = (size_t)blockIdx.x * (kBroadBlock / 64) + wave; w < n_long && w < q.n_a; w += waves) {
        const size_t i = long_rows[w];
        if (i >= q.n_a) continue;
        unsigned long long pos = row_off[i];
        const unsigned long long cnt = row_count[i];
        const unsigned long long end = pos + cnt;
        if (pos >= capacity) continue;
        const float4 ba = q.box_a[i];
        typename S::Obj ra;
        S::load(q.A, i, ra);
        bool done = false;
        if (!box_wild(ba) && cnt <= (unsigned long long)kMidHits) {
            const BroadCells c = broad_cell_range(g, gx, gy, ba);
            uint32_t lo[3], hi[3], walked = 0;   // a regular row spans at most two cells: at most three cell rows
            const uint32_t rows = c.cy1 - c.cy0 + 1u <= 3u ? c.cy1 - c.cy0 + 1u : 0u;
            if (rows == 0u) walked = kCandidateCap + 1u;
            for (uint32_t r = 0; r < rows; r++) {
                const uint32_t cy = c.cy0 + r;
                lo[r] = lower_bound_u32(q.keys, n_reg, cy * gx + c.cx0);
                hi[r] = lower_bound_u32(q.keys, n_reg, cy * gx + c.cx1 + 1u);
                walked += hi[r] - lo[r];
            }
            if (walked <= kCandidateCap) {
                uint32_t m = 0;
                for (uint32_t r = 0; r < rows; r++) {
                    for (uint32_t k0 = lo[r]; k0 < hi[r]; k0 += 64) {
                        const uint32_t k = k0 + lane;
                        bool hit = false;
                        uint32_t j = 0;
                        if (k < hi[r] && boxes_meet(ba, q.sbox[k])) {
                            j = q.idx[k];
                            if (!(q.upper && (size_t)j <= i)) {
                                typename S::Obj rb;
                                S::load(q.B, j, rb);
                                hit = S::collide(ra, rb);
                            }
                        }
                        const unsigned long long bal = __ballot(hit);
                        const uint32_t at = m + (uint32_t)__popcll(bal & below);
                        if (hit && at < (uint32_t)kMidHits) hits[wave][at] = j;
                        m += (uint32_t)__popcll(bal);
                    }
                }
                for (size_t k0 = n_reg; k0 < q.n_b; k0 += 64) {
                    const size_t k = k0 + lane;
                    bool hit = false;
                    uint32_t j = 0;
                    const bool live = k < q.n_b && q.keys[k] != kAbsentKey;
                    if (__ballot(live) == 0ull) break;   // (wave-uniform) only absent objects from here on
                    if (live) {
                        j = q.idx[k];
                        if (!(q.upper && (size_t)j <= i)) {
                            typename S::Obj rb;
                            S::load(q.B, j, rb);
                            hit = S::collide(ra, rb);
                        }
                    }
                    const unsigned long long bal = __ballot(hit);
                    const uint32_t at = m + (uint32_t)__popcll(bal & below);
                    if (hit && at < (uint32_t)kMidHits) hits[wave][at] = j;
                    m += (uint32_t)__popcll(bal);
                }
                wave_lds_sync();
                if ((unsigned long long)m == cnt) {   // always (the count pass ran the same query); the guard keeps writes in the row's range
                    for (uint32_t e = lane; e < m; e += 64) {
                        const uint32_t v = hits[wave][e];
                        uint32_t rank = 0;
                        for (uint32_t x = 0; x < m; x++) rank += hits[wave][x] < v ? 1u : 0u;
                        const unsigned long long p = pos + rank;
                        if (p < capacity) {
                            pairs[2 * p] = (uint32_t)i;
                            pairs[2 * p + 1] = v;
                        }
                    }
                    done = true;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (done) continue;
        for (size_t j0 = q.upper ? i + 1 : 0; j0 < q.n_b && pos < end && pos < capacity; j0 += 64) {
            const size_t j = j0 + lane;
            const bool hit = j < q.n_b && broad_pair<S>(q, ba, ra, j);
            const unsigned long long bal = __ballot(hit);
            const unsigned long long p = pos + (unsigned long long)__popcll(bal & below);
            if (hit && p < end && p < capacity) {
                pairs[2 * p] = (uint32_t)i;
                pairs[2 * p + 1] = (uint32_t)j;
            }
            pos += (unsigned long long)__popcll(bal);
        }
    }
}

// ---- host side: the shape-independent stages live in c2d_broad.hip ------------------------------------------------------

constexpr size_t kBroadIndexLimit = (size_t)1 << 32;   // the list's indices are u32

// the flags and the list arguments of a broad entry point (row_base = col_base = 0: the indices end at n_a, n_b)
inline int broad_check_list(c2d_ctx* ctx, const char* what, int flags, const uint32_t* d_pairs, size_t capacity, const unsigned long long* d_count,
                            size_t n_a, size_t n_b)
{
    if (int rc = cross_check_flags(ctx, what, flags)) return rc;
    return cross_check_list(ctx, what, d_pairs, capacity, d_count, n_a, n_b, kBroadIndexLimit, "n_a and n_b must stay at or below 2^32 (the list is u32)");
}

// the scratch of one call, carved (broad_layout: every size depends on n_a, n_b and whether B is A, never on the input's values)
struct BroadScratch {
    BroadGrid* g;
    float4 *box_a, *box_b, *sbox;
    uint32_t *keys0, *keys1, *vals0, *vals1, *long_rows, *hist, *hist_sums;
    unsigned long long *row_count, *row_off, *row_sums;
    size_t tiles_b, hist_n;
    const uint32_t *keys, *idx;   // the sorted keys and their indices (set by broad_grid_and_sort)
};

// The guard of the ctx workspace, then the scratch: grown when too small (refused with C2D_ERR_INVALID_ARG while `s` is being
// captured, before anything is enqueued), and carved into W.
int broad_scratch(c2d_ctx* ctx, hipStream_t s, const char* what, size_t n_a, size_t n_b, bool same, BroadScratch& W);
// the scene header of this call
int broad_begin(c2d_ctx* ctx, hipStream_t s, const BroadScratch& W);
// from the boxes to B's sorted keys: cell size, bounds, grid, keys (objects that span more than two cells become wild), the radix
// sort, B's boxes in key order
int broad_grid_and_sort(c2d_ctx* ctx, hipStream_t s, BroadScratch& W, size_t n_a, size_t n_b, bool same);
// exclusive scan of the row counts into W.row_off; the total is added to d_count
int broad_scan_and_total(c2d_ctx* ctx, hipStream_t s, const BroadScratch& W, size_t n_a, unsigned long long* d_count);

// The first half of every call that searches through the grid, for box policy S: the scratch behind the workspace guard, the scene
// header, the boxes of both sets (once when B is A) and B's sorted keys.  `use` is the caller's: it is armed here, once the scratch
// is held and before the first enqueue, and stamps when the caller calls done() behind its own last kernel, or leaves its scope on
// an error (a refusal of the scratch leaves it unarmed: nothing was queued).
template <class S>
int broad_prepare(c2d_ctx* ctx, hipStream_t s, const char* what, const typename S::Set& A, size_t n_a, const typename S::Set& B, size_t n_b, bool same,
                  BroadScratch& W, WorkspaceUse& use)
{
    if (int rc = broad_scratch(ctx, s, what, n_a, n_b, same, W)) return rc;
    use.arm();   // the kernels work through the scratch: stamp behind the last one
    if (int rc = broad_begin(ctx, s, W)) return rc;
    hipLaunchKernelGGL(broad_box_kernel<S>, dim3(grid_for(n_a, kBroadBlock, 8192)), dim3(kBroadBlock), 0, s, A, n_a, W.box_a, W.g);
    C2D_LAUNCH_CHECK(ctx);
    if (!same) {
        hipLaunchKernelGGL(broad_box_kernel<S>, dim3(grid_for(n_b, kBroadBlock, 8192)), dim3(kBroadBlock), 0, s, B, n_b, W.box_b, W.g);
        C2D_LAUNCH_CHECK(ctx);
    }
    return broad_grid_and_sort(ctx, s, W, n_a, n_b, same);
}

// One call of the pair search for shape S.  The caller has checked its arguments and holds the DeviceGuard.
template <class S>
int broad_run(c2d_ctx* ctx, hipStream_t s, const char* what, const typename S::Set& A, size_t n_a, const typename S::Set& B, size_t n_b, bool same,
              int flags, uint32_t* d_pairs, size_t capacity, unsigned long long* d_count)
{
    BroadScratch W;
    WorkspaceUse use(ctx, s);
    if (int rc = broad_prepare<S>(ctx, s, what, A, n_a, B, n_b, same, W, use)) return rc;
    const int grid_a = grid_for(n_a, kBroadBlock, 8192);

    BroadQuery<S> q{A, B, W.box_a, W.box_b, W.keys, W.idx, W.sbox, W.g, n_a, n_b, (flags & C2D_CROSS_UPPER) ? 1 : 0};
    hipLaunchKernelGGL(broad_count_kernel<S>, dim3(grid_a), dim3(kBroadBlock), 0, s, q, W.row_count, W.long_rows, W.g);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(broad_long_count_kernel<S>, dim3(kLongGrid), dim3(kBroadBlock), 0, s, q, W.row_count, (const uint32_t*)W.long_rows,
                       (const BroadGrid*)W.g);
    C2D_LAUNCH_CHECK(ctx);
    if (int rc = broad_scan_and_total(ctx, s, W, n_a, d_count)) return rc;
    if (capacity) {
        hipLaunchKernelGGL(broad_emit_kernel<S>, dim3(grid_a), dim3(kBroadBlock), 0, s, q, (const unsigned long long*)W.row_count,
                           (const unsigned long long*)W.row_off, (const BroadGrid*)W.g, d_pairs, capacity);
        C2D_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(broad_long_emit_kernel<S>, dim3(kLongGrid), dim3(kBroadBlock), 0, s, q, (const unsigned long long*)W.row_count,
                           (const unsigned long long*)W.row_off, (const uint32_t*)W.long_rows, (const BroadGrid*)W.g, d_pairs, capacity);
        C2D_LAUNCH_CHECK(ctx);
    }
    use.done();
    return C2D_OK;
}

}  // namespace c2d
