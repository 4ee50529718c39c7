// c2d_broad.hip — broad-phase rectangle pair search for gfx950 (MI355X): the pair list of c2d_sat_rect_cross_pairs, bit for bit,
// in roughly O(N log N + candidates) instead of N x M exact tests.
//
// Pipeline:
//   1. box:     one thread per object of A ∪ B computes a conservative box (broad_box: a box that the reference's test cannot
//               report a collision outside of) or marks the object wild; a histogram of box extents picks the cell size S.
//   2. grid:    the bounds of the ordinary boxes and S give a uniform grid of at most 65535 x 65535 cells.  An object whose box
//               spans more than two cells in x or y is wild as well.  B's regular objects get the key (cell row, cell column)
//               of their box's min corner, wild ones the key 0xffffffff; a stable LSD radix sort (four 8-bit passes) orders them.
//   3. count:   one thread per row i of A queries the cells that can hold an overlapping box (three cell rows, each one range of
//               the sorted keys), tests box overlap, then runs rect_collide (the reference's eight-axis test, c2d_math.hpp) on the
//               survivors, and tests every wild column.  Wild rows, rows that meet too many candidates and rows with more hits
//               than the short emit path holds go to a list that one wave per row serves over all columns in index order.
//   4. scan:    exclusive scan of the row counts; the total is added to d_count.
//   5. emit:    short rows repeat the query, sort their hits by column in LDS and write them; listed rows emit in column order
//               with a wave ballot.  Only positions below the capacity are written.
// The sort and the scan are this file's own kernels: a captured call is a graph of this file's kernels only.
#include "c2d_internal.hpp"
#include "c2d_math.hpp"


namespace c2d {

struct BroadPlanes { const float* p[8]; };

constexpr int kBroadBlock = 256;           // threads per block of the per-object and per-row kernels
constexpr int kHistBins = 1024;            // box extents by their float bits >> 21: exponent and two mantissa bits
constexpr uint32_t kWildKey = 0xffffffffu;
constexpr int kShortHits = 16;             // hits a row may have for the short emit path (LDS sort)
constexpr int kMidHits = 512;              // hits a listed regular row may have for the wave path of the long emit kernel
constexpr uint32_t kCandidateCap = 1024;   // sorted entries a row may walk in the short path before it goes to the list
constexpr unsigned long long kUncounted = ~0ull;
constexpr int kLongGrid = 2048;            // blocks of the listed-row kernels (grid-stride over the list)
constexpr uint32_t kMaxCells = 65535;      // cells per axis: keys cy * gx + cx stay below kWildKey

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

C2D_DEV unsigned int f2key(float f)
{
    const unsigned int b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
C2D_DEV float key2f(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

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

// The conservative box of one object, or false: the object is wild and is tested against everything.
// Let a_k = fl(v_{k+1} - v_k), k = 0, 1 (the object's first two axes as rect_collide computes them, taken as exact vectors),
// I_k = [min, max] of the exact a_k . v over its four vertices and C its largest |coordinate|.  The parallelogram
//     U = { p : a_k . p in I_k widened by W_k, k = 0, 1 },   W_k = |a_k|_1 (2^-21 C + 2^-66) + 2^-140,
// contains the object, and DESIGN.md §5.8 proves: if U_A and U_B of two regular objects are disjoint, the reference's test
// reports no collision for them (U's edge normals are exactly axes 0 and 1 of the test, and W_k covers both objects' rounding
// of the dot products, underflow included).  The box is box(U), computed in double and rounded outward to float.
// Wild: a non-finite coordinate, a |coordinate| of 2^60 or more (the rounding bound needs products far from overflow),
// |a_k|_1 below 2^-80 (the underflow term is bounded through it), parallel axes (U unbounded), or a box that is not finite.
C2D_DEV bool broad_box(const float (&r)[8], float4& box)
{
    float cmax = 0.0f;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        finite = finite && __builtin_isfinite(r[k]);
        cmax = __builtin_fmaxf(cmax, __builtin_fabsf(r[k]));
    }
    if (!finite || !(cmax < 0x1p60f)) return false;
    const double C = cmax;
    double ax[2], ay[2], slo[2], shi[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        ax[i] = (double)(r[2 * i + 2] - r[2 * i]);       // the float subtraction of rect_collide
        ay[i] = (double)(r[2 * i + 3] - r[2 * i + 1]);
        const double n1 = __builtin_fabs(ax[i]) + __builtin_fabs(ay[i]);
        if (!(n1 >= 0x1p-80)) return false;
        double lo = ax[i] * (double)r[0] + ay[i] * (double)r[1], hi = lo;   // products exact in double, one rounding each sum
#pragma unroll
        for (int v = 1; v < 4; v++) {
            const double p = ax[i] * (double)r[2 * v] + ay[i] * (double)r[2 * v + 1];
            lo = p < lo ? p : lo;
            hi = p > hi ? p : hi;
        }
        const double w = n1 * (0x1p-21 * C + 0x1p-66) + 0x1p-140;
        slo[i] = lo - w;
        shi[i] = hi + w;
    }
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

C2D_DEV bool box_wild(const float4& b) { return __builtin_isnan(b.x); }
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

C2D_DEV void load_rect(const BroadPlanes& P, size_t i, float (&r)[8])
{
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = P.p[k][i];
}

// 1. boxes (NaN box = wild) and the extent histogram
__global__ __launch_bounds__(kBroadBlock) void broad_box_kernel(BroadPlanes X, size_t n, float4* __restrict__ box, BroadGrid* __restrict__ g)
{
    __shared__ unsigned int hist[kHistBins];
    for (int b = threadIdx.x; b < kHistBins; b += kBroadBlock) hist[b] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBroadBlock) {
        float r[8];
        load_rect(X, i, r);
        float4 b;
        if (broad_box(r, b)) {
            atomicAdd(&hist[__float_as_uint(box_extent(b)) >> 21], 1u);
        } else {
            const float q = __builtin_nanf("");
            b = make_float4(q, q, q, q);
        }
        box[i] = b;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kHistBins; b += kBroadBlock)
        if (hist[b]) atomicAdd(&g->hist[b], hist[b]);
}

// 2. the cell size: the upper edge of the smallest extent bin with at most max(4, n / 65536) boxes above it.  Every box above S may
//    be wild, and every row tests every wild column: the limit keeps that cost to a few exact tests per row.
__global__ __launch_bounds__(kHistBins) void broad_scale_kernel(BroadGrid* __restrict__ g)
{
    __shared__ unsigned long long suf[kHistBins];
    __shared__ unsigned int best;
    const int b = threadIdx.x;
    suf[b] = g->hist[b];
    if (b == 0) best = kHistBins - 1;
    __syncthreads();
    for (int off = 1; off < kHistBins; off <<= 1) {   // inclusive suffix sums
        const unsigned long long o = b + off < kHistBins ? suf[b + off] : 0ull;
        __syncthreads();
        suf[b] += o;
        __syncthreads();
    }
    const unsigned long long total = suf[0];
    const unsigned long long above = b + 1 < kHistBins ? suf[b + 1] : 0ull;
    const unsigned long long limit = total >> 16 > 4ull ? total >> 16 : 4ull;
    if (above <= limit) atomicMin(&best, (unsigned int)b);
    __syncthreads();
    // (bins 1016..1020 hold extents near FLT_MAX and infinite ones: the edge stays finite)
    if (b == 0) g->s = __uint_as_float((best < 1018u ? best + 1u : 1019u) << 21);
}

// 3. bounds of the boxes narrower than S
__global__ __launch_bounds__(kBroadBlock) void broad_bounds_kernel(const float4* __restrict__ box, size_t n, BroadGrid* __restrict__ g)
{
    const float s = g->s;
    unsigned int lx = 0xffffffffu, ly = 0xffffffffu, hx = 0u, hy = 0u;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBroadBlock) {
        const float4 b = box[i];
        if (box_wild(b) || !(box_extent(b) < s)) continue;
        lx = min(lx, f2key(b.x));
        ly = min(ly, f2key(b.y));
        hx = max(hx, f2key(b.z));
        hy = max(hy, f2key(b.w));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lx = min(lx, (unsigned int)__shfl_down((int)lx, off, 64));
        ly = min(ly, (unsigned int)__shfl_down((int)ly, off, 64));
        hx = max(hx, (unsigned int)__shfl_down((int)hx, off, 64));
        hy = max(hy, (unsigned int)__shfl_down((int)hy, off, 64));
    }
    if ((threadIdx.x & 63u) == 0 && hx != 0u) {
        atomicMin(&g->lo_x, lx);
        atomicMin(&g->lo_y, ly);
        atomicMax(&g->hi_x, hx);
        atomicMax(&g->hi_y, hy);
    }
}

// 4. the grid: cells of size S, or larger where the bounds would need more than 65535 of them
__global__ void broad_grid_kernel(BroadGrid* __restrict__ g)
{
    if (threadIdx.x != 0) return;
    double x0 = 0.0, y0 = 0.0, ex = 0.0, ey = 0.0;
    if (g->hi_x != 0u) {
        x0 = key2f(g->lo_x);
        y0 = key2f(g->lo_y);
        ex = (double)key2f(g->hi_x) - x0;
        ey = (double)key2f(g->hi_y) - y0;
    }
    const double inv_s = 1.0 / (double)g->s;
    const double ix = ex * inv_s > (double)(kMaxCells - 1) ? (double)(kMaxCells - 1) / ex : inv_s;
    const double iy = ey * inv_s > (double)(kMaxCells - 1) ? (double)(kMaxCells - 1) / ey : inv_s;
    g->x0 = x0;
    g->y0 = y0;
    g->ix = ix;
    g->iy = iy;
    g->gx = (uint32_t)__builtin_floor(ex * ix) + 1u;
    g->gy = (uint32_t)__builtin_floor(ey * iy) + 1u;
}

// 5. an object whose box spans more than two cells in x or y becomes wild; B's objects get their sort key and index
__global__ __launch_bounds__(kBroadBlock) void broad_key_kernel(float4* __restrict__ box, size_t n, const BroadGrid* __restrict__ g,
                                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                unsigned int* __restrict__ n_reg)
{
    const double x0 = g->x0, y0 = g->y0, ix = g->ix, iy = g->iy;
    const uint32_t gx = g->gx, gy = g->gy;
    uint32_t regular = 0;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBroadBlock) {
        float4 b = box[i];
        uint32_t key = kWildKey;
        if (!box_wild(b)) {
            const uint32_t cx0 = cell_of(b.x, x0, ix, gx), cx1 = cell_of(b.z, x0, ix, gx);
            const uint32_t cy0 = cell_of(b.y, y0, iy, gy), cy1 = cell_of(b.w, y0, iy, gy);
            if (cx1 - cx0 > 1u || cy1 - cy0 > 1u) {
                const float q = __builtin_nanf("");
                box[i] = make_float4(q, q, q, q);
            } else {
                key = cy0 * gx + cx0;
                regular++;
            }
        }
        if (keys) {
            keys[i] = key;
            vals[i] = (uint32_t)i;
        }
    }
    if (keys) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) regular += __shfl_down(regular, off, 64);
        if ((threadIdx.x & 63u) == 0 && regular) atomicAdd(n_reg, regular);
    }
}

// 6b. B's boxes in key order
__global__ __launch_bounds__(kBroadBlock) void broad_gather_kernel(const float4* __restrict__ box, const uint32_t* __restrict__ sorted_idx,
                                                                   size_t n, float4* __restrict__ sbox)
{
    for (size_t k = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBroadBlock) sbox[k] = box[sorted_idx[k]];
}

struct BroadQuery {
    BroadPlanes A, B;
    const float4* box_a;        // [n_a] (NaN: wild)
    const float4* box_b;        // [n_b], index order
    const uint32_t* keys;       // [n_b] sorted keys: regular ones first, then kWildKey
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
template <class Visit>
C2D_DEV bool broad_row_query(const BroadQuery& q, size_t i, const float4& ba, const float (&ra)[8], uint32_t n_reg, Visit visit)
{
    const BroadGrid* g = q.g;
    const uint32_t gx = g->gx, gy = g->gy;
    // B_j overlaps ba only if cx(min x_j) is in [cx(min x_i) - 1, cx(max x_i)]: B_j spans at most two cells and cell_of is monotone
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
            float rb[8];
            load_rect(q.B, j, rb);
            if (rect_collide(ra, rb)) visit(j);
        }
    }
    for (size_t k = n_reg; k < q.n_b; k++) {
        const uint32_t j = q.idx[k];
        if (q.upper && (size_t)j <= i) continue;
        float rb[8];
        load_rect(q.B, j, rb);
        if (rect_collide(ra, rb)) visit(j);
    }
    return true;
}

// 7. per-row counts of regular rows; wild rows, rows over the candidate cap and rows with more than kShortHits hits go to the list
__global__ __launch_bounds__(kBroadBlock) void broad_count_kernel(BroadQuery q, unsigned long long* __restrict__ row_count,
                                                                  uint32_t* __restrict__ long_rows, BroadGrid* __restrict__ g)
{
    const uint32_t n_reg = g->n_reg_b;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < q.n_a; i += (size_t)gridDim.x * kBroadBlock) {
        const float4 ba = q.box_a[i];
        unsigned long long cnt = kUncounted;
        if (!box_wild(ba)) {
            float ra[8];
            load_rect(q.A, i, ra);
            unsigned long long c = 0;
            if (broad_row_query(q, i, ba, ra, n_reg, [&](uint32_t) { c++; })) cnt = c;
        }
        row_count[i] = cnt;
        if (cnt == kUncounted || cnt > (unsigned long long)kShortHits) {
            const unsigned int slot = atomicAdd(&g->n_long, 1u);   // each row at most once: slot < n_a
            if ((size_t)slot < q.n_a) long_rows[slot] = (uint32_t)i;
        }
    }
}

// Result (i, j) in the listed-row path: boxes first where both objects are regular, the exact test otherwise.
C2D_DEV bool broad_pair(const BroadQuery& q, const float4& ba, const float (&ra)[8], size_t j)
{
    const float4 bb = q.box_b[j];
    if (!box_wild(ba) && !box_wild(bb) && !boxes_meet(ba, bb)) return false;
    float rb[8];
    load_rect(q.B, j, rb);
    return rect_collide(ra, rb);
}

// 8. listed rows whose count is missing: one wave per row over all columns (upper: columns above the row)
__global__ __launch_bounds__(kBroadBlock) void broad_long_count_kernel(BroadQuery q, unsigned long long* __restrict__ row_count,
                                                                       const uint32_t* __restrict__ long_rows, const BroadGrid* __restrict__ g)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_long = g->n_long;
    const size_t waves = (size_t)gridDim.x * (kBroadBlock / 64);
    for (size_t w = (size_t)blockIdx.x * (kBroadBlock / 64) + (threadIdx.x >> 6); w < n_long; w += waves) {
        const size_t i = long_rows[w];
        if (row_count[i] != kUncounted) continue;
        const float4 ba = q.box_a[i];
        float ra[8];
        load_rect(q.A, i, ra);
        unsigned long long c = 0;
        for (size_t j = (q.upper ? i + 1 : 0) + lane; j < q.n_b; j += 64) c += broad_pair(q, ba, ra, j) ? 1u : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0) row_count[i] = c;
    }
}

// 9. the total of the scanned counts into d_count
__global__ void broad_total_kernel(const unsigned long long* __restrict__ row_count, const unsigned long long* __restrict__ row_off, size_t n,
                                   unsigned long long* __restrict__ d_count)
{
    if (threadIdx.x == 0) atomicAdd(d_count, row_off[n - 1] + row_count[n - 1]);
}

// 10. short rows: repeat the query, sort the hits by column in LDS, write those below the capacity
__global__ __launch_bounds__(kBroadBlock) void broad_emit_kernel(BroadQuery q, const unsigned long long* __restrict__ row_count,
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
        float ra[8];
        load_rect(q.A, i, ra);
        uint32_t m = 0;
        const bool ok = broad_row_query(q, i, ba, ra, n_reg, [&](uint32_t j) {
            if (m < (uint32_t)kShortHits) hits[m][t] = j;
            m++;
        });
        if (!ok) continue;   // over the candidate cap in the count pass too: a listed row
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
__global__ __launch_bounds__(kBroadBlock) void broad_long_emit_kernel(BroadQuery q, const unsigned long long* __restrict__ row_count,
                                                                      const unsigned long long* __restrict__ row_off,
                                                                      const uint32_t* __restrict__ long_rows, const BroadGrid* __restrict__ g,
                                                                      uint32_t* __restrict__ pairs, size_t capacity)
{
    __shared__ uint32_t hits[kBroadBlock / 64][kMidHits];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_long = g->n_long, n_reg = g->n_reg_b, gx = g->gx, gy = g->gy;
    const size_t waves = (size_t)gridDim.x * (kBroadBlock / 64);
    const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
    for (size_t w = (size_t)blockIdx.x * (kBroadBlock / 64) + wave; w < n_long; w += waves) {
        const size_t i = long_rows[w];
        unsigned long long pos = row_off[i];
        const unsigned long long cnt = row_count[i];
        const unsigned long long end = pos + cnt;
        if (pos >= capacity) continue;
        const float4 ba = q.box_a[i];
        float ra[8];
        load_rect(q.A, i, ra);
        bool done = false;
        if (!box_wild(ba) && cnt <= (unsigned long long)kMidHits) {
            uint32_t cx0 = cell_of(ba.x, g->x0, g->ix, gx), cx1 = cell_of(ba.z, g->x0, g->ix, gx);
            uint32_t cy0 = cell_of(ba.y, g->y0, g->iy, gy), cy1 = cell_of(ba.w, g->y0, g->iy, gy);
            cx0 = cx0 ? cx0 - 1u : 0u;
            cy0 = cy0 ? cy0 - 1u : 0u;
            uint32_t lo[3], hi[3], walked = 0;   // a regular row spans at most two cells: at most three cell rows
            const uint32_t rows = cy1 - cy0 + 1u <= 3u ? cy1 - cy0 + 1u : 0u;
            if (rows == 0u) walked = kCandidateCap + 1u;
            for (uint32_t r = 0; r < rows; r++) {
                const uint32_t cy = cy0 + r;
                lo[r] = lower_bound_u32(q.keys, n_reg, cy * gx + cx0);
                hi[r] = lower_bound_u32(q.keys, n_reg, cy * gx + cx1 + 1u);
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
                                float rb[8];
                                load_rect(q.B, j, rb);
                                hit = rect_collide(ra, rb);
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
                    if (k < q.n_b) {
                        j = q.idx[k];
                        if (!(q.upper && (size_t)j <= i)) {
                            float rb[8];
                            load_rect(q.B, j, rb);
                            hit = rect_collide(ra, rb);
                        }
                    }
                    const unsigned long long bal = __ballot(hit);
                    const uint32_t at = m + (uint32_t)__popcll(bal & below);
                    if (hit && at < (uint32_t)kMidHits) hits[wave][at] = j;
                    m += (uint32_t)__popcll(bal);
                }
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
            const bool hit = j < q.n_b && broad_pair(q, ba, ra, j);
            const unsigned long long bal = __ballot(hit);
            const unsigned long long p = pos + (unsigned long long)__popcll(bal & below);
            if (hit && p < capacity) {
                pairs[2 * p] = (uint32_t)i;
                pairs[2 * p + 1] = (uint32_t)j;
            }
            pos += (unsigned long long)__popcll(bal);
        }
    }
}

// ---- sort and scan ------------------------------------------------------------------------------------------------------
// Hand-written, so that every node of a captured call is one of this file's kernels ("Graph capture").
constexpr int kTileItems = 8;                                   // items per thread of the sort and scan tiles
constexpr int kTile = kBroadBlock * kTileItems;                 // 2048 items per block
constexpr int kRadixBits = 8;
constexpr int kRadixBins = 1 << kRadixBits;
constexpr int kRadixPasses = 32 / kRadixBits;

// scene header of one call: zeros, and the empty minimum for the bounds (a kernel, not memsets: see DESIGN.md §5.8)
__global__ __launch_bounds__(kBroadBlock) void broad_init_kernel(BroadGrid* __restrict__ g)
{
    unsigned int* w = reinterpret_cast<unsigned int*>(g);
    constexpr int words = (int)(sizeof(BroadGrid) / 4);
    for (int k = threadIdx.x; k < words; k += kBroadBlock) w[k] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        g->lo_x = 0xffffffffu;
        g->lo_y = 0xffffffffu;
    }
}

// block-wide exclusive sum of one value per thread; *total receives the block's sum
template <class T>
C2D_DEV T block_exclusive_sum(T v, T* total)
{
    __shared__ T wave_tot[kBroadBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += o;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kBroadBlock / 64; k++) {
        before += k < (int)wave ? wave_tot[k] : T(0);
        all += wave_tot[k];
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// scan 1/3: the sum of each tile of kTile items
template <class T>
__global__ __launch_bounds__(kBroadBlock) void scan_tile_sums_kernel(const T* __restrict__ in, size_t n, T* __restrict__ tile_sum)
{
    const size_t base = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kTileItems;
    T v = 0;
#pragma unroll
    for (int k = 0; k < kTileItems; k++) v += base + k < n ? in[base + k] : T(0);
    T total;
    (void)block_exclusive_sum(v, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// scan 2/3: one block, exclusive sum of the tile sums in place
template <class T>
__global__ __launch_bounds__(kBroadBlock) void scan_tiles_kernel(T* __restrict__ tile_sum, size_t tiles)
{
    T carry = 0;
    for (size_t c0 = 0; c0 < tiles; c0 += kBroadBlock) {
        const size_t c = c0 + threadIdx.x;
        const T v = c < tiles ? tile_sum[c] : T(0);
        T total;
        const T ex = block_exclusive_sum(v, &total);
        if (c < tiles) tile_sum[c] = carry + ex;
        carry += total;
    }
}

// scan 3/3: out[i] = sum of in[0, i) (out may alias in)
template <class T>
__global__ __launch_bounds__(kBroadBlock) void scan_apply_kernel(const T* in, size_t n, const T* __restrict__ tile_sum, T* out)
{
    const size_t base = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kTileItems;
    T v[kTileItems];
    T sum = 0;
#pragma unroll
    for (int k = 0; k < kTileItems; k++) {
        v[k] = base + k < n ? in[base + k] : T(0);
        sum += v[k];
    }
    T total;
    T run = tile_sum[blockIdx.x] + block_exclusive_sum(sum, &total);
#pragma unroll
    for (int k = 0; k < kTileItems; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

// radix pass 1/2: digit counts of each tile, digit-major: hist[d * tiles + tile]
__global__ __launch_bounds__(kBroadBlock) void radix_hist_kernel(const uint32_t* __restrict__ keys, size_t n, int shift,
                                                                 uint32_t* __restrict__ hist, size_t tiles)
{
    __shared__ uint32_t cnt[kRadixBins];
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kTile;
#pragma unroll
    for (int r = 0; r < kTileItems; r++) {
        const size_t i = base + (size_t)r * kBroadBlock + threadIdx.x;
        if (i < n) atomicAdd(&cnt[(keys[i] >> shift) & (kRadixBins - 1)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * tiles + blockIdx.x] = cnt[threadIdx.x];
}

// radix pass 2/2: stable scatter.  Rounds walk the tile in position order; inside a round the lanes of a wave that share a digit
// are found with eight ballots, and the waves of the block are ordered through per-wave digit counts in LDS.
__global__ __launch_bounds__(kBroadBlock) void radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                                    size_t n, int shift, const uint32_t* __restrict__ offs, size_t tiles,
                                                                    uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out)
{
    __shared__ uint32_t base[kRadixBins];
    __shared__ uint32_t wave_cnt[kBroadBlock / 64][kRadixBins];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
    base[threadIdx.x] = offs[(size_t)threadIdx.x * tiles + blockIdx.x];
    const size_t tile0 = (size_t)blockIdx.x * kTile;
#pragma unroll 1
    for (int r = 0; r < kTileItems; r++) {
#pragma unroll
        for (int w = 0; w < kBroadBlock / 64; w++) wave_cnt[w][threadIdx.x] = 0u;
        __syncthreads();
        const size_t i = tile0 + (size_t)r * kBroadBlock + threadIdx.x;
        const bool valid = i < n;
        const uint32_t key = valid ? keys_in[i] : 0u;
        const uint32_t d = (key >> shift) & (kRadixBins - 1);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < kRadixBits; b++) {
            const unsigned long long m = __ballot(valid && ((d >> b) & 1u));
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        if (valid && rank == 0) wave_cnt[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = base[d] + rank;
            for (uint32_t w = 0; w < wave; w++) pos += wave_cnt[w][d];
            keys_out[pos] = key;
            vals_out[pos] = vals_in[i];
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int w = 0; w < kBroadBlock / 64; w++) add += wave_cnt[w][threadIdx.x];
        base[threadIdx.x] += add;
        __syncthreads();
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------

constexpr size_t kBroadIndexLimit = (size_t)1 << 32;   // the list's indices are u32

static size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// Scratch of one call; every size depends on n_a, n_b and whether B is A, never on the input's values.
struct BroadLayout {
    size_t grid, box_a, box_b, keys0, keys1, vals0, vals1, sbox, count, off, rows, hist, hist_sums, row_sums, total;
    size_t tiles_b, hist_n;
};

static size_t tiles_of(size_t n) { return (n + kTile - 1) / kTile; }

static void broad_layout(size_t n_a, size_t n_b, bool same, BroadLayout& L)
{
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes ? bytes : 1); return at; };
    L.tiles_b = tiles_of(n_b);
    L.hist_n = (size_t)kRadixBins * L.tiles_b;
    L.grid = take(sizeof(BroadGrid));
    L.box_a = take(n_a * sizeof(float4));
    L.box_b = same ? L.box_a : take(n_b * sizeof(float4));
    L.keys0 = take(n_b * 4);
    L.keys1 = take(n_b * 4);
    L.vals0 = take(n_b * 4);
    L.vals1 = take(n_b * 4);
    L.sbox = take(n_b * sizeof(float4));
    L.count = take(n_a * 8);
    L.off = take(n_a * 8);
    L.rows = take(n_a * 4);
    L.hist = take(L.hist_n * 4);
    L.hist_sums = take(tiles_of(L.hist_n) * 4);
    L.row_sums = take(tiles_of(n_a) * 8);
    L.total = o;
}

// out = exclusive prefix sums of in[0, n) (out may be in), through tile_sum[tiles_of(n)]
template <class T>
static int exclusive_scan(c2d_ctx* ctx, hipStream_t s, const T* in, T* out, size_t n, T* tile_sum)
{
    const size_t tiles = tiles_of(n);
    hipLaunchKernelGGL(scan_tile_sums_kernel<T>, dim3((unsigned)tiles), dim3(kBroadBlock), 0, s, in, n, tile_sum);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(scan_tiles_kernel<T>, dim3(1), dim3(kBroadBlock), 0, s, tile_sum, tiles);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(scan_apply_kernel<T>, dim3((unsigned)tiles), dim3(kBroadBlock), 0, s, in, n, (const T*)tile_sum, out);
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_sat_rect_broad_pairs(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b, int flags,
                             uint32_t* d_pairs, size_t capacity, unsigned long long* d_count, c2d_stream stream)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (n_a == 0 || n_b == 0) return C2D_OK;
    if (!d_a || !d_b) return fail_arg(ctx, "c2d_sat_rect_broad_pairs: NULL argument");
    BroadPlanes A, B;
    bool same = n_a == n_b;
    for (int k = 0; k < 8; k++) {
        if (!d_a[k] || !d_b[k]) return fail_arg(ctx, "c2d_sat_rect_broad_pairs: NULL plane");
        A.p[k] = d_a[k];
        B.p[k] = d_b[k];
        same = same && d_a[k] == d_b[k];
    }
    if (flags & ~C2D_CROSS_UPPER) return fail_arg(ctx, "c2d_sat_rect_broad_pairs: unknown flag");
    if (!d_count) return fail_arg(ctx, "c2d_sat_rect_broad_pairs: d_count is required");
    if (!d_pairs && capacity) return fail_arg(ctx, "c2d_sat_rect_broad_pairs: NULL pair buffer");
    if (n_a > kBroadIndexLimit || n_b > kBroadIndexLimit)
        return fail_arg(ctx, "c2d_sat_rect_broad_pairs: n_a and n_b must stay at or below 2^32 (the list is u32)");
    DeviceGuard dg(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    BroadLayout L;
    broad_layout(n_a, n_b, same, L);
    if (int rc = workspace_acquire(ctx, s, true)) return rc;
    if (ctx->scratch_bytes < L.total) {
        if (stream_is_capturing(s))
            return fail_arg(ctx, "c2d_sat_rect_broad_pairs: the ctx scratch must grow, which cannot happen during graph capture "
                                 "(make the call once outside the capture first)");
        if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
        ctx->d_scratch = nullptr;
        ctx->scratch_bytes = 0;
        C2D_HIP(ctx, hipMalloc(&ctx->d_scratch, L.total));
        ctx->scratch_bytes = L.total;
    }
    char* base = static_cast<char*>(ctx->d_scratch);
    BroadGrid* g = reinterpret_cast<BroadGrid*>(base + L.grid);
    float4* box_a = reinterpret_cast<float4*>(base + L.box_a);
    float4* box_b = reinterpret_cast<float4*>(base + L.box_b);
    uint32_t* keys0 = reinterpret_cast<uint32_t*>(base + L.keys0);
    uint32_t* keys1 = reinterpret_cast<uint32_t*>(base + L.keys1);
    uint32_t* vals0 = reinterpret_cast<uint32_t*>(base + L.vals0);
    uint32_t* vals1 = reinterpret_cast<uint32_t*>(base + L.vals1);
    float4* sbox = reinterpret_cast<float4*>(base + L.sbox);
    unsigned long long* row_count = reinterpret_cast<unsigned long long*>(base + L.count);
    unsigned long long* row_off = reinterpret_cast<unsigned long long*>(base + L.off);
    uint32_t* long_rows = reinterpret_cast<uint32_t*>(base + L.rows);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + L.hist);
    uint32_t* hist_sums = reinterpret_cast<uint32_t*>(base + L.hist_sums);
    unsigned long long* row_sums = reinterpret_cast<unsigned long long*>(base + L.row_sums);

    WorkspaceUse use(ctx, s);   // the kernels work through the scratch: stamp behind the last one
    use.arm();
    hipLaunchKernelGGL(broad_init_kernel, dim3(1), dim3(kBroadBlock), 0, s, g);
    C2D_LAUNCH_CHECK(ctx);
    const int grid_a = grid_for(n_a, kBroadBlock, 8192), grid_b = grid_for(n_b, kBroadBlock, 8192);
    hipLaunchKernelGGL(broad_box_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, A, n_a, box_a, g);
    C2D_LAUNCH_CHECK(ctx);
    if (!same) {
        hipLaunchKernelGGL(broad_box_kernel, dim3(grid_b), dim3(kBroadBlock), 0, s, B, n_b, box_b, g);
        C2D_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(broad_scale_kernel, dim3(1), dim3(kHistBins), 0, s, g);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(broad_bounds_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, box_a, n_a, g);
    C2D_LAUNCH_CHECK(ctx);
    if (!same) {
        hipLaunchKernelGGL(broad_bounds_kernel, dim3(grid_b), dim3(kBroadBlock), 0, s, box_b, n_b, g);
        C2D_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(broad_grid_kernel, dim3(1), dim3(64), 0, s, g);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(broad_key_kernel, dim3(grid_b), dim3(kBroadBlock), 0, s, box_b, n_b, g, keys0, vals0, &g->n_reg_b);
    C2D_LAUNCH_CHECK(ctx);
    if (!same) {
        hipLaunchKernelGGL(broad_key_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, box_a, n_a, g, (uint32_t*)nullptr, (uint32_t*)nullptr,
                           (unsigned int*)nullptr);
        C2D_LAUNCH_CHECK(ctx);
    }
    // stable LSD radix sort of (key, index), four passes: the result is back in keys0 / vals0
    uint32_t *k_in = keys0, *k_out = keys1, *v_in = vals0, *v_out = vals1;
    for (int pass = 0; pass < kRadixPasses; pass++) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)L.tiles_b), dim3(kBroadBlock), 0, s, (const uint32_t*)k_in, n_b, pass * kRadixBits,
                           hist, L.tiles_b);
        C2D_LAUNCH_CHECK(ctx);
        if (int rc = exclusive_scan<uint32_t>(ctx, s, hist, hist, L.hist_n, hist_sums)) return rc;
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)L.tiles_b), dim3(kBroadBlock), 0, s, (const uint32_t*)k_in, (const uint32_t*)v_in,
                           n_b, pass * kRadixBits, (const uint32_t*)hist, L.tiles_b, k_out, v_out);
        C2D_LAUNCH_CHECK(ctx);
        uint32_t* t = k_in; k_in = k_out; k_out = t;
        t = v_in; v_in = v_out; v_out = t;
    }
    hipLaunchKernelGGL(broad_gather_kernel, dim3(grid_b), dim3(kBroadBlock), 0, s, box_b, (const uint32_t*)v_in, n_b, sbox);
    C2D_LAUNCH_CHECK(ctx);

    BroadQuery q{A, B, box_a, box_b, k_in, v_in, sbox, g, n_a, n_b, (flags & C2D_CROSS_UPPER) ? 1 : 0};
    hipLaunchKernelGGL(broad_count_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, q, row_count, long_rows, g);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(broad_long_count_kernel, dim3(kLongGrid), dim3(kBroadBlock), 0, s, q, row_count, (const uint32_t*)long_rows,
                       (const BroadGrid*)g);
    C2D_LAUNCH_CHECK(ctx);
    if (int rc = exclusive_scan<unsigned long long>(ctx, s, row_count, row_off, n_a, row_sums)) return rc;
    hipLaunchKernelGGL(broad_total_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)row_count, (const unsigned long long*)row_off,
                       n_a, d_count);
    C2D_LAUNCH_CHECK(ctx);
    if (capacity) {
        hipLaunchKernelGGL(broad_emit_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, q, (const unsigned long long*)row_count,
                           (const unsigned long long*)row_off, (const BroadGrid*)g, d_pairs, capacity);
        C2D_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(broad_long_emit_kernel, dim3(kLongGrid), dim3(kBroadBlock), 0, s, q, (const unsigned long long*)row_count,
                           (const unsigned long long*)row_off, (const uint32_t*)long_rows, (const BroadGrid*)g, d_pairs, capacity);
        C2D_LAUNCH_CHECK(ctx);
    }
    use.done();
    return C2D_OK;
}

}  // extern "C"
