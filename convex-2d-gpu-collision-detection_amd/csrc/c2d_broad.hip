// c2d_broad.hip — broad-phase rectangle pair search for gfx950 (MI355X): the pair list of c2d_sat_rect_cross_pairs, bit for bit,
// in roughly O(N log N + candidates) instead of N x M exact tests.
//
// Pipeline:
//   1. box:     one thread per object of A ∪ B computes a conservative box (broad_box: a box that the reference's test cannot
//               report a collision outside of) or marks the object wild; a histogram of box extents picks the cell size S.
//   2. grid:    the bounds of the ordinary boxes and S give a uniform grid of at most 65535 x 65535 cells.  An object whose box
//               spans more than two cells in x or y is wild as well.  B's regular objects get the key (cell row, cell column)
//               of their box's min corner, wild ones the key 0xfffffffe; a stable LSD radix sort (four 8-bit passes) orders them.
//   3. count:   one thread per row i of A queries the cells that can hold an overlapping box (three cell rows, each one range of
//               the sorted keys), tests box overlap, then runs rect_collide (the reference's eight-axis test, c2d_math.hpp) on the
//               survivors, and tests every wild column.  Wild rows, rows that meet too many candidates and rows with more hits
//               than the short emit path holds go to a list that one wave per row serves over all columns in index order.
//   4. scan:    exclusive scan of the row counts; the total is added to d_count.
//   5. emit:    short rows repeat the query, sort their hits by column in LDS and write them; listed rows emit in column order
//               with a wave ballot.  Only positions below the capacity are written.
// The sort and the scan are this file's own kernels: a captured call is a graph of this file's kernels only.
//
// The kernels that touch an object (box, count, emit, the listed-row pair) are templates over a shape policy in c2d_broad.hpp;
// this file holds the shape-independent stages, which exist once, and the rectangle policy.  c2d_poly_broad.hip runs the same
// pipeline over convex polygons.
#include "c2d_broad.hpp"


namespace c2d {

struct BroadPlanes { const float* p[8]; };

C2D_DEV unsigned int f2key(float f)
{
    const unsigned int b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
C2D_DEV float key2f(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

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
        const double w = broad_slab_widening(n1, C);
        slo[i] = lo - w;
        shi[i] = hi + w;
    }
    return broad_box_of_slabs(ax, ay, slo, shi, box);   // (c2d_broad.hpp: shared with the polygon box)
}

C2D_DEV void load_rect(const BroadPlanes& P, size_t i, float (&r)[8])
{
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = P.p[k][i];
}

// the rectangle policy of the pipeline (c2d_broad.hpp): eight vertex planes, broad_box, rect_collide; no rectangle is absent
struct RectShape {
    using Set = BroadPlanes;
    struct Obj { float r[8]; };
    static C2D_DEV void load(const Set& X, size_t i, Obj& o) { load_rect(X, i, o.r); }
    static C2D_DEV int box(const Set& X, size_t i, float4& b)
    {
        float r[8];
        load_rect(X, i, r);
        return broad_box(r, b) ? kBroadRegular : kBroadWild;
    }
    static C2D_DEV bool collide(const Obj& a, const Obj& b) { return rect_collide(a.r, b.r); }
};

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

// 5. an object whose box spans more than two cells in x or y becomes wild; B's objects get their sort key and index (absent ones
//    the last key of all, behind the wild ones)
__global__ __launch_bounds__(kBroadBlock) void broad_key_kernel(float4* __restrict__ box, size_t n, const BroadGrid* __restrict__ g,
                                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                unsigned int* __restrict__ n_reg)
{
    const double x0 = g->x0, y0 = g->y0, ix = g->ix, iy = g->iy;
    const uint32_t gx = g->gx, gy = g->gy;
    uint32_t regular = 0;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBroadBlock) {
        float4 b = box[i];
        uint32_t key = box_absent(b) ? kAbsentKey : kWildKey;
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
// 9. the total of the scanned counts into d_count
__global__ void broad_total_kernel(const unsigned long long* __restrict__ row_count, const unsigned long long* __restrict__ row_off, size_t n,
                                   unsigned long long* __restrict__ d_count)
{
    if (threadIdx.x == 0) atomicAdd(d_count, row_off[n - 1] + row_count[n - 1]);
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

int broad_scratch(c2d_ctx* ctx, hipStream_t s, const char* what, size_t n_a, size_t n_b, bool same, BroadScratch& W)
{
    BroadLayout L;
    broad_layout(n_a, n_b, same, L);
    if (int rc = workspace_acquire(ctx, s, true)) return rc;
    if (ctx->scratch_bytes < L.total) {
        if (stream_is_capturing(s)) {
            char msg[224];
            std::snprintf(msg, sizeof msg, "%s: the ctx scratch must grow, which cannot happen during graph capture "
                                           "(make the call once outside the capture first)", what);
            return fail_arg(ctx, msg);
        }
        if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
        ctx->d_scratch = nullptr;
        ctx->scratch_bytes = 0;
        C2D_HIP(ctx, hipMalloc(&ctx->d_scratch, L.total));
        ctx->scratch_bytes = L.total;
    }
    char* base = static_cast<char*>(ctx->d_scratch);
    W.g = reinterpret_cast<BroadGrid*>(base + L.grid);
    W.box_a = reinterpret_cast<float4*>(base + L.box_a);
    W.box_b = reinterpret_cast<float4*>(base + L.box_b);
    W.keys0 = reinterpret_cast<uint32_t*>(base + L.keys0);
    W.keys1 = reinterpret_cast<uint32_t*>(base + L.keys1);
    W.vals0 = reinterpret_cast<uint32_t*>(base + L.vals0);
    W.vals1 = reinterpret_cast<uint32_t*>(base + L.vals1);
    W.sbox = reinterpret_cast<float4*>(base + L.sbox);
    W.row_count = reinterpret_cast<unsigned long long*>(base + L.count);
    W.row_off = reinterpret_cast<unsigned long long*>(base + L.off);
    W.long_rows = reinterpret_cast<uint32_t*>(base + L.rows);
    W.hist = reinterpret_cast<uint32_t*>(base + L.hist);
    W.hist_sums = reinterpret_cast<uint32_t*>(base + L.hist_sums);
    W.row_sums = reinterpret_cast<unsigned long long*>(base + L.row_sums);
    W.tiles_b = L.tiles_b;
    W.hist_n = L.hist_n;
    W.keys = nullptr;
    W.idx = nullptr;
    return C2D_OK;
}

int broad_begin(c2d_ctx* ctx, hipStream_t s, const BroadScratch& W)
{
    hipLaunchKernelGGL(broad_init_kernel, dim3(1), dim3(kBroadBlock), 0, s, W.g);
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}

int broad_grid_and_sort(c2d_ctx* ctx, hipStream_t s, BroadScratch& W, size_t n_a, size_t n_b, bool same)
{
    BroadGrid* g = W.g;
    const int grid_a = grid_for(n_a, kBroadBlock, 8192), grid_b = grid_for(n_b, kBroadBlock, 8192);
    hipLaunchKernelGGL(broad_scale_kernel, dim3(1), dim3(kHistBins), 0, s, g);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(broad_bounds_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, W.box_a, n_a, g);
    C2D_LAUNCH_CHECK(ctx);
    if (!same) {
        hipLaunchKernelGGL(broad_bounds_kernel, dim3(grid_b), dim3(kBroadBlock), 0, s, W.box_b, n_b, g);
        C2D_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(broad_grid_kernel, dim3(1), dim3(64), 0, s, g);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(broad_key_kernel, dim3(grid_b), dim3(kBroadBlock), 0, s, W.box_b, n_b, g, W.keys0, W.vals0, &g->n_reg_b);
    C2D_LAUNCH_CHECK(ctx);
    if (!same) {
        hipLaunchKernelGGL(broad_key_kernel, dim3(grid_a), dim3(kBroadBlock), 0, s, W.box_a, n_a, g, (uint32_t*)nullptr, (uint32_t*)nullptr,
                           (unsigned int*)nullptr);
        C2D_LAUNCH_CHECK(ctx);
    }
    // stable LSD radix sort of (key, index), four passes: the result is back in keys0 / vals0
    uint32_t *k_in = W.keys0, *k_out = W.keys1, *v_in = W.vals0, *v_out = W.vals1;
    for (int pass = 0; pass < kRadixPasses; pass++) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)W.tiles_b), dim3(kBroadBlock), 0, s, (const uint32_t*)k_in, n_b, pass * kRadixBits,
                           W.hist, W.tiles_b);
        C2D_LAUNCH_CHECK(ctx);
        if (int rc = exclusive_scan<uint32_t>(ctx, s, W.hist, W.hist, W.hist_n, W.hist_sums)) return rc;
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)W.tiles_b), dim3(kBroadBlock), 0, s, (const uint32_t*)k_in, (const uint32_t*)v_in,
                           n_b, pass * kRadixBits, (const uint32_t*)W.hist, W.tiles_b, k_out, v_out);
        C2D_LAUNCH_CHECK(ctx);
        uint32_t* t = k_in; k_in = k_out; k_out = t;
        t = v_in; v_in = v_out; v_out = t;
    }
    hipLaunchKernelGGL(broad_gather_kernel, dim3(grid_b), dim3(kBroadBlock), 0, s, W.box_b, (const uint32_t*)v_in, n_b, W.sbox);
    C2D_LAUNCH_CHECK(ctx);
    W.keys = k_in;
    W.idx = v_in;
    return C2D_OK;
}

int broad_scan_and_total(c2d_ctx* ctx, hipStream_t s, const BroadScratch& W, size_t n_a, unsigned long long* d_count)
{
    if (int rc = exclusive_scan<unsigned long long>(ctx, s, W.row_count, W.row_off, n_a, W.row_sums)) return rc;
    hipLaunchKernelGGL(broad_total_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)W.row_count, (const unsigned long long*)W.row_off,
                       n_a, d_count);
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
    if (int rc = broad_check_list(ctx, "c2d_sat_rect_broad_pairs", flags, d_pairs, capacity, d_count, n_a, n_b)) return rc;
    DeviceGuard dg(ctx->device);
    return broad_run<RectShape>(ctx, (hipStream_t)stream, "c2d_sat_rect_broad_pairs", A, n_a, B, n_b, same, flags, d_pairs, capacity, d_count);
}

}  // extern "C"
