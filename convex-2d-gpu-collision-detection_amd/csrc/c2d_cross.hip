// c2d_cross.hip — all-pairs rectangle SAT for gfx950 (MI355X): every rectangle of a set A against every rectangle of a set B.
//
// The pairwise kernels (c2d_sat.hip) read 64 bytes per pair and are HBM-bound.  Here the input is N + M rectangles, so the
// kernel is VALU-bound: every quantity of convex_collide (reference utils.cu:159-184) that depends on ONE rectangle only is
// computed once per rectangle instead of once per pair — its edge axes 0 and 1, the projections of its own vertices onto them
// (extremes and the projection of vertex 0), the two terms of the parallel-axis certificate and its coordinate bound.  What is
// left per pair is the sixteen cross projections (A's vertices onto B's axes 0, 1 and B's onto A's), their extremes, the
// comparisons and the certificate.
//
// Mapping: a block of 256 lanes owns 256 consecutive rows of A, one per lane, with the lane's hoisted quantities in VGPRs;
// the block stages 256 consecutive columns of B, with theirs, in LDS.  The inner loop walks the columns with a wave-uniform
// index, so every LDS read is a broadcast (one address per wave: no bank conflicts), and a lane gathers the 64 results of one
// mask word in registers and stores the word with one 8-byte store.  The certificate and its fall-back are those of the pairwise
// path, bit for bit: a pair whose certificate fails ("thin") is evaluated with all eight axes (rect_collide), for the wave
// that holds it.  With C2D_CROSS_UPPER a wave skips the arithmetic of every mask word that lies on or below the diagonal for
// all of its rows and writes zeros there.
//
// The pair list runs the mask kernel over row passes of A into ctx scratch, counts each row's bits, scans the counts on the
// device (the running base of earlier passes stays on the device) and emits the pairs whose position is below the capacity.
#include "c2d_cross.hpp"
#include "c2d_math.hpp"
#include "c2d_count.hpp"
#include "c2d_wave.hpp"

namespace c2d {

struct CrossPlanes { const float* p[8]; };

constexpr int kCrossBlock = 256;      // rows of A per block: one per lane
constexpr int kCrossCols = 256;       // columns of B per block: four mask words
constexpr int kSideVecs = 6;          // one rectangle's hoisted quantities: 24 floats, six 16-byte LDS reads

// The quantities of convex_collide and of the parallel-axis certificates (c2d_math.hpp) that depend on one rectangle only.
// Every projection is computed by the same IEEE operations, in the same order, as rect_collide computes it inside a pair.
struct RectSide {
    float v[8];              // the vertices x0,y0,...,x3,y3
    float ax[2], ay[2];      // edge axes 0 and 1
    float lo[2], hi[2];      // min4 / max4 of the rectangle's own projections onto its axes 0 and 1
    float first[2];          // projection of its vertex 0 onto its axes 0 and 1 (the NaN rule, first_projections_ordered)
    float s1[2], s2[2];      // certificate terms of axis i: |a|_1 and |a + b|_1, b = edge i + 2
    float cmax;              // max |coordinate| (fmax drops NaNs, as the pairwise chain does)
};

C2D_DEV void rect_side(const float (&r)[8], RectSide& q)
{
#pragma unroll
    for (int k = 0; k < 8; k++) q.v[k] = r[k];
    float cmax = __builtin_fabsf(r[0]);
#pragma unroll
    for (int k = 1; k < 8; k++) cmax = __builtin_fmaxf(cmax, __builtin_fabsf(r[k]));
    q.cmax = cmax;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const float ax = r[2 * i + 2] - r[2 * i], ay = r[2 * i + 3] - r[2 * i + 1];
        const float bx = r[(2 * i + 6) & 7] - r[2 * i + 4], by = r[(2 * i + 7) & 7] - r[2 * i + 5];
        const float p0 = dot2(ax, r[0], ay, r[1]), p1 = dot2(ax, r[2], ay, r[3]);
        const float p2 = dot2(ax, r[4], ay, r[5]), p3 = dot2(ax, r[6], ay, r[7]);
        q.ax[i] = ax;
        q.ay[i] = ay;
        q.lo[i] = min4(p0, p1, p2, p3);
        q.hi[i] = max4(p0, p1, p2, p3);
        q.first[i] = p0;
        q.s1[i] = __builtin_fabsf(ax) + __builtin_fabsf(ay);
        q.s2[i] = __builtin_fabsf(ax + bx) + __builtin_fabsf(ay + by);
    }
    // The certificate's error bound is a rounding bound: it holds while no product or difference overflows.  A coordinate of
    // 3e38 or inf does not break it with a NaN (that reads thin by itself) but with infinite overlaps that pass an infinite
    // `need` — 75 pairs of tests/test_gpu_sat_cross.py::test_non_finite_vertices were certified "collide" and separate on an
    // axis of edge 2 or 3.  The pairwise kernels never meet this in their tests (the wave-wide fall-back re-evaluates every pair
    // of a wave that holds one thin pair, and injected NaNs make almost every wave thin); here the fall-back is per pair, so the
    // certificate is kept to its domain: with every |coordinate| below 2^61, |axis| <= 2^62, |projection| <= 2^124 and every
    // overlap stays below 2^126.  A rectangle beyond that (or with NaN for every coordinate) gets s1[0] = NaN, so every pair it is
    // in reads thin (its `need` on that axis is NaN) and goes to rect_collide.  No per-pair cost.
    if (!(cmax < 0x1p61f)) q.s1[0] = __builtin_nanf("");
}

C2D_DEV void side_pack(const RectSide& q, f32x4 (&o)[kSideVecs])
{
    o[0] = f32x4{q.v[0], q.v[1], q.v[2], q.v[3]};
    o[1] = f32x4{q.v[4], q.v[5], q.v[6], q.v[7]};
    o[2] = f32x4{q.ax[0], q.ay[0], q.ax[1], q.ay[1]};
    o[3] = f32x4{q.lo[0], q.hi[0], q.lo[1], q.hi[1]};
    o[4] = f32x4{q.first[0], q.first[1], q.s1[0], q.s1[1]};
    o[5] = f32x4{q.s2[0], q.s2[1], q.cmax, 0.0f};
}

C2D_DEV void side_unpack(const f32x4 (&o)[kSideVecs], RectSide& q)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        q.v[k] = o[0][k];
        q.v[4 + k] = o[1][k];
    }
    q.ax[0] = o[2][0]; q.ay[0] = o[2][1]; q.ax[1] = o[2][2]; q.ay[1] = o[2][3];
    q.lo[0] = o[3][0]; q.hi[0] = o[3][1]; q.lo[1] = o[3][2]; q.hi[1] = o[3][3];
    q.first[0] = o[4][0]; q.first[1] = o[4][1]; q.s1[0] = o[4][2]; q.s1[1] = o[4][3];
    q.s2[0] = o[5][0]; q.s2[1] = o[5][1]; q.cmax = o[5][2];
}

// Axes 0, 1 of both rectangles from hoisted sides, axes 2, 3 by the parallel-axis certificates (c2d_math.hpp, where the
// soundness argument is written).  The certificate's bound C is the pair's own max |coordinate|: fmax(A.cmax, B.cmax) is the
// value of an fmax chain over the sixteen coordinates (max is associative on numbers, |x| has no -0, and both forms drop a NaN
// unless every operand is one).  A pair with a rectangle outside the certificate's domain (a |coordinate| of 2^61 or more, see
// rect_side) always reads thin.  `sep` needs no argument (it is rect_collide's own test on four of its eight axes).
C2D_DEV bool cross_collide_certified(const RectSide& A, const RectSide& B, bool& thin)
{
    const float cmax = __builtin_fmaxf(A.cmax, B.cmax);
    const float c2 = (2.0f + 0x1p-7f) * cmax, c3 = (8.0f + 0x1p-5f) * 0x1p-24f * cmax;
    bool sep = false, uneasy = false;
#pragma unroll
    for (int i = 0; i < 2; i++) {   // A's axes: A's projections hoisted, B's computed
        const float ax = A.ax[i], ay = A.ay[i];
        const float p20 = dot2(ax, B.v[0], ay, B.v[1]), p21 = dot2(ax, B.v[2], ay, B.v[3]);
        const float p22 = dot2(ax, B.v[4], ay, B.v[5]), p23 = dot2(ax, B.v[6], ay, B.v[7]);
        const float min1 = A.lo[i], max1 = A.hi[i];
        const float min2 = min4(p20, p21, p22, p23), max2 = max4(p20, p21, p22, p23);
        sep |= ((max1 < min2) || (max2 < min1)) && first_projections_ordered(A.first[i], p20);
        const float need = fma_(A.s1[i], c3, A.s2[i] * c2) + 1e-36f;
        uneasy |= !((max2 - min1 >= need) && (max1 - min2 >= need));
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {   // B's axes: B's projections hoisted, A's computed
        const float ax = B.ax[i], ay = B.ay[i];
        const float p10 = dot2(ax, A.v[0], ay, A.v[1]), p11 = dot2(ax, A.v[2], ay, A.v[3]);
        const float p12 = dot2(ax, A.v[4], ay, A.v[5]), p13 = dot2(ax, A.v[6], ay, A.v[7]);
        const float min1 = min4(p10, p11, p12, p13), max1 = max4(p10, p11, p12, p13);
        const float min2 = B.lo[i], max2 = B.hi[i];
        sep |= ((max1 < min2) || (max2 < min1)) && first_projections_ordered(p10, B.first[i]);
        const float need = fma_(B.s1[i], c3, B.s2[i] * c2) + 1e-36f;
        uneasy |= !((max2 - min1 >= need) && (max1 - min2 >= need));
    }
    thin = !sep && uneasy;
    return !sep;
}

// Result (i, j) for the lane's row i and the wave-uniform column held in `col`, fast path and wave-wide fall-back.
C2D_DEV uint32_t cross_pair(const RectSide& a, const f32x4 (&col)[kSideVecs])
{
    RectSide b;
    side_unpack(col, b);
    bool thin;
    bool hit = cross_collide_certified(a, b, thin);
    if (__ballot(thin) != 0ull) {
        float r1[8], r2[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            r1[k] = launder(a.v[k], Laundered{});   // (as collide_pairs of c2d_sat.hip: nothing of the fast path is kept alive)
            r2[k] = launder(b.v[k], Laundered{});
        }
        const bool full = rect_collide(r1, r2);
        hit = thin ? full : hit;
    }
    return hit ? 1u : 0u;
}

// One launch covers row tiles [row_tile0, row_tile0 + gridDim.x / col_tiles) and column tiles [col_tile0, col_tile0 + col_tiles)
// (one-dimensional grid: the count's wave numbering is blockIdx.x).  Row i of A is global row row_base + i, column j of B global
// column col_base + j; diag = row_base - col_base.  With `upper`, bit j of row i is tested only if col_base + j > row_base + i.
__global__ __launch_bounds__(kCrossBlock) void cross_mask_kernel(CrossPlanes A, size_t n_a, CrossPlanes B, size_t n_b, size_t row_tile0,
                                                                  size_t col_tile0, uint32_t col_tiles, long long diag, int upper,
                                                                  unsigned long long* __restrict__ mask, size_t ld_words,
                                                                  unsigned long long* __restrict__ d_count, CountWs words)
{
    __shared__ f32x4 tile[kCrossCols][kSideVecs];   // 24 KiB
    const uint32_t lane = threadIdx.x;
    const size_t rt = row_tile0 + blockIdx.x / col_tiles;
    const size_t j0 = (col_tile0 + blockIdx.x % col_tiles) * (size_t)kCrossCols;
    {
        const size_t j = j0 + lane;
        float r[8];
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] = j < n_b ? B.p[k][j] : 0.0f;
        RectSide q;
        rect_side(r, q);
        f32x4 o[kSideVecs];
        side_pack(q, o);
#pragma unroll
        for (int k = 0; k < kSideVecs; k++) tile[lane][k] = o[k];
    }
    const size_t i = rt * kCrossBlock + lane;
    RectSide a;
    {
        float r[8];
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] = i < n_a ? A.p[k][i] : 0.0f;
        rect_side(r, a);
    }
    __syncthreads();
    const size_t words_b = (n_b + 63) / 64;
    const size_t wave_row0 = rt * kCrossBlock + (lane & ~63u);
    uint32_t my_count = 0;
#pragma unroll 1
    for (int w = 0; w < kCrossCols / 64; w++) {
        const size_t word = j0 / 64 + (size_t)w;
        if (word >= words_b) break;
        const size_t jb = j0 + 64 * (size_t)w;
        const uint32_t nj = (uint32_t)(n_b - jb < 64 ? n_b - jb : 64);
        // upper: every column of the word on or below the diagonal for every row of the wave -> no arithmetic
        const bool skip = upper && (long long)(jb + 63) - (long long)wave_row0 <= diag;
        unsigned long long bits = 0;
        if (!skip) {
            uint32_t half[2] = {0u, 0u};
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t end = nj > 32u * h ? (nj - 32u * h < 32u ? nj - 32u * h : 32u) : 0u;
                const f32x4 (*cols)[kSideVecs] = tile + 64 * w + 32 * h;
                for (uint32_t b = 0; b < end; b++) half[h] |= cross_pair(a, cols[b]) << b;
            }
            bits = ((unsigned long long)half[1] << 32) | half[0];
            if (upper) {   // tested: bit b with col_base + jb + b > row_base + i, i.e. b > t
                const long long t = (long long)i + diag - (long long)jb;
                bits = t < 0 ? bits : (t >= 63 ? 0ull : bits & (~0ull << (t + 1)));
            }
        }
        if (i < n_a) {
            mask[i * ld_words + word] = bits;
            my_count += (uint32_t)__popcll(bits);
        }
    }
    if (d_count) wave_count_arrive(my_count, d_count, words);
}

// ---- pair list ----------------------------------------------------------------------------------------------------------
constexpr int kListBlock = 256;   // rows per chunk of the list kernels; four waves

// wave-wide inclusive sum of v (u64) over lanes 0..lane
C2D_DEV unsigned long long wave_inclusive_sum(unsigned long long v)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v += o;
    }
    return v;
}

// Chunk c = rows [256c, 256c + 256) of the pass: the set bits of every row (a wave per row, lanes over the words), then the
// exclusive prefix of the row counts inside the chunk (row_off) and the chunk's total (chunk_sum).
__global__ __launch_bounds__(kListBlock) void cross_row_counts_kernel(const unsigned long long* __restrict__ mask, size_t rows, size_t words,
                                                                       unsigned long long* __restrict__ row_off,
                                                                       unsigned long long* __restrict__ chunk_sum)
{
    __shared__ unsigned long long cnt[kListBlock];
    __shared__ unsigned long long wave_tot[kListBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t r0 = (size_t)blockIdx.x * kListBlock;
    for (uint32_t k = wave; k < (uint32_t)kListBlock; k += kListBlock / 64) {
        const size_t r = r0 + k;
        unsigned long long c = 0;
        if (r < rows)
            for (size_t w = lane; w < words; w += 64) c += (unsigned long long)__popcll(mask[r * words + w]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0) cnt[k] = c;
    }
    __syncthreads();
    const unsigned long long mine = cnt[threadIdx.x];
    const unsigned long long incl = wave_inclusive_sum(mine);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned long long before = 0;
    for (uint32_t k = 0; k < wave; k++) before += wave_tot[k];
    const size_t r = r0 + threadIdx.x;
    if (r < rows) row_off[r] = before + incl - mine;
    if (threadIdx.x == kListBlock - 1) chunk_sum[blockIdx.x] = before + incl;
}

// One block: chunk_sum[] -> exclusive prefix plus *base (the pairs of earlier passes); *base += the pass's total.
__global__ __launch_bounds__(kListBlock) void cross_scan_chunks_kernel(unsigned long long* __restrict__ chunk_sum, size_t n_chunks,
                                                                        unsigned long long* __restrict__ base)
{
    __shared__ unsigned long long wave_tot[kListBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = *base;
    for (size_t c0 = 0; c0 < n_chunks; c0 += kListBlock) {
        const size_t c = c0 + threadIdx.x;
        const unsigned long long mine = c < n_chunks ? chunk_sum[c] : 0ull;
        const unsigned long long incl = wave_inclusive_sum(mine);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, all = 0;
        for (uint32_t k = 0; k < kListBlock / 64; k++) {
            before += k < wave ? wave_tot[k] : 0ull;
            all += wave_tot[k];
        }
        if (c < n_chunks) chunk_sum[c] = carry + before + incl - mine;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *base = carry;
}

// Chunk c of the pass: each wave writes the pairs of its rows in row-major order, (row0 + r, col_base + j) at position
// chunk_sum[c] + row_off[r] + (set bits before it in the row); only positions below `capacity` are written.
__global__ __launch_bounds__(kListBlock) void cross_emit_kernel(const unsigned long long* __restrict__ mask, size_t rows, size_t words,
                                                                 const unsigned long long* __restrict__ row_off,
                                                                 const unsigned long long* __restrict__ chunk_sum, uint32_t row0,
                                                                 uint32_t col_base, uint32_t* __restrict__ pairs, size_t capacity)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t r0 = (size_t)blockIdx.x * kListBlock;
    const unsigned long long chunk_base = chunk_sum[blockIdx.x];
    for (uint32_t k = wave; k < (uint32_t)kListBlock; k += kListBlock / 64) {
        const size_t r = r0 + k;
        if (r >= rows) break;
        unsigned long long pos0 = chunk_base + row_off[r];
        for (size_t w0 = 0; w0 < words && pos0 < capacity; w0 += 64) {
            const size_t w = w0 + lane;
            unsigned long long m = w < words ? mask[r * words + w] : 0ull;
            const unsigned long long pc = (unsigned long long)__popcll(m);
            const unsigned long long incl = wave_inclusive_sum(pc);
            unsigned long long pos = pos0 + incl - pc;
            while (m != 0ull && pos < capacity) {
                const uint32_t b = (uint32_t)__builtin_ctzll(m);
                pairs[2 * pos] = row0 + (uint32_t)r;
                pairs[2 * pos + 1] = col_base + (uint32_t)(64 * w + b);
                pos++;
                m &= m - 1;
            }
            pos0 += __shfl(incl, 63, 64);
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------

constexpr size_t kPairScratchMaskBytes = (size_t)256 << 20;   // mask rows of one pass of the pair list

static bool cross_planes(const float* const d[8], CrossPlanes& P)
{
    for (int k = 0; k < 8; k++) {
        if (!d[k]) return false;
        P.p[k] = d[k];
    }
    return true;
}

// Shared argument checks of both forms; C2D_OK or the status to return.
static int cross_check(c2d_ctx* ctx, const char* what, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b,
                size_t row_base, size_t col_base, int flags, CrossPlanes& A, CrossPlanes& B)
{
    if (!d_a || !d_b) return cross_fail(ctx, what, "NULL argument");
    if (!cross_planes(d_a, A) || !cross_planes(d_b, B)) return cross_fail(ctx, what, "NULL plane");
    return cross_check_flags_bases(ctx, what, n_a, n_b, row_base, col_base, flags);
}

// The mask of rows [0, n_a) x columns [0, n_b) into `mask` (row stride ld_words), in launches of at most kMaxGrid blocks.
static int cross_mask_launch(c2d_ctx* ctx, hipStream_t s, const CrossPlanes& A, size_t n_a, const CrossPlanes& B, size_t n_b, size_t row_base,
                      size_t col_base, bool upper, unsigned long long* mask, size_t ld_words, unsigned long long* d_count)
{
    const size_t row_tiles = (n_a + kCrossBlock - 1) / kCrossBlock, col_tiles = (n_b + kCrossCols - 1) / kCrossCols;
    const long long diag = (long long)row_base - (long long)col_base;
    return for_each_tile_launch(row_tiles, col_tiles, (size_t)kMaxGrid, [&](size_t r0, size_t c0, size_t rows, size_t cols) {
        const size_t grid = rows * cols;
        hipLaunchKernelGGL(cross_mask_kernel, dim3((unsigned)grid), dim3(kCrossBlock), 0, s, A, n_a, B, n_b, r0, c0, (uint32_t)cols, diag,
                           upper ? 1 : 0, mask, ld_words, d_count, workspace_count_ticket(ctx, s, grid * (kCrossBlock / 64), d_count != nullptr));
        C2D_LAUNCH_CHECK(ctx);
        return (int)C2D_OK;
    });
}

// The pair list of any N x M mask producer (declared in c2d_cross.hpp; the polygon form, c2d_poly_cross.hip, is the second
// caller): `pass` queues the counting mask kernel(s) of rows [r0, r0 + rows) of A into `mask` (row stride `words`); the row
// counts, the chunk scan with the running base on the device and the emit follow each pass.
int cross_list_run(c2d_ctx* ctx, hipStream_t s, const char* what, size_t n_a, size_t n_b, size_t row_base, size_t col_base, uint32_t* d_pairs,
                   size_t capacity, unsigned long long* d_count, const CrossMaskPass& pass)
{
    if (int rc = cross_check_list(ctx, what, d_pairs, capacity, d_count, row_base + n_a, col_base + n_b, kIndexLimit,
                                  "global indices must stay below 2^32 (the list is u32)"))
        return rc;
    // scratch: [rows_pass][words] mask | [rows_pass] row offsets | [chunks] chunk sums | running base
    const size_t words = (n_b + 63) / 64;
    size_t rows_pass = kPairScratchMaskBytes / (words * 8);
    rows_pass = rows_pass >= (size_t)kListBlock ? rows_pass / kListBlock * kListBlock : (rows_pass ? rows_pass : 1);
    if (rows_pass > n_a) rows_pass = n_a;
    const size_t chunks = (rows_pass + kListBlock - 1) / kListBlock;
    const size_t off_rows = (rows_pass * words * 8 + 255) / 256 * 256;
    const size_t off_chunks = off_rows + (rows_pass * 8 + 255) / 256 * 256;
    const size_t off_base = off_chunks + (chunks * 8 + 255) / 256 * 256;
    const size_t need = off_base + 256;
    if (int rc = workspace_acquire(ctx, s, true)) return rc;
    if (ctx->scratch_bytes < need) {
        if (stream_is_capturing(s))
            return cross_fail(ctx, what, "the ctx scratch must grow, which cannot happen during graph capture (make the call once outside the capture first)");
        if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
        ctx->d_scratch = nullptr;
        ctx->scratch_bytes = 0;
        C2D_HIP(ctx, hipMalloc(&ctx->d_scratch, need));
        ctx->scratch_bytes = need;
    }
    char* scratch = static_cast<char*>(ctx->d_scratch);
    unsigned long long* d_mask = reinterpret_cast<unsigned long long*>(scratch);
    unsigned long long* d_row_off = reinterpret_cast<unsigned long long*>(scratch + off_rows);
    unsigned long long* d_chunk = reinterpret_cast<unsigned long long*>(scratch + off_chunks);
    unsigned long long* d_base = reinterpret_cast<unsigned long long*>(scratch + off_base);
    WorkspaceUse use(ctx, s);   // the list kernels read the scratch behind the counting mask kernel: stamp behind the last one
    C2D_HIP(ctx, hipMemsetAsync(d_base, 0, 8, s));
    use.arm();
    for (size_t r0 = 0; r0 < n_a; r0 += rows_pass) {
        const size_t rows = n_a - r0 < rows_pass ? n_a - r0 : rows_pass;
        const size_t n_chunks = (rows + kListBlock - 1) / kListBlock;
        if (int rc = pass(r0, rows, d_mask, words)) return rc;
        hipLaunchKernelGGL(cross_row_counts_kernel, dim3((unsigned)n_chunks), dim3(kListBlock), 0, s, d_mask, rows, words, d_row_off, d_chunk);
        C2D_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(cross_scan_chunks_kernel, dim3(1), dim3(kListBlock), 0, s, d_chunk, n_chunks, d_base);
        C2D_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(cross_emit_kernel, dim3((unsigned)n_chunks), dim3(kListBlock), 0, s, d_mask, rows, words, d_row_off, d_chunk,
                           (uint32_t)(row_base + r0), (uint32_t)col_base, d_pairs, capacity);
        C2D_LAUNCH_CHECK(ctx);
    }
    use.done();
    return C2D_OK;
}

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_sat_rect_cross_mask(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b, size_t row_base,
                            size_t col_base, int flags, unsigned long long* d_mask, size_t ld_words, unsigned long long* d_count,
                            c2d_stream stream)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (n_a == 0 || n_b == 0) return C2D_OK;
    CrossPlanes A, B;
    if (int rc = cross_check(ctx, "c2d_sat_rect_cross_mask", d_a, n_a, d_b, n_b, row_base, col_base, flags, A, B)) return rc;
    if (int rc = cross_check_mask(ctx, "c2d_sat_rect_cross_mask", d_mask, ld_words, n_b)) return rc;
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = workspace_acquire(ctx, s, d_count != nullptr)) return rc;
    return cross_mask_launch(ctx, s, A, n_a, B, n_b, row_base, col_base, (flags & C2D_CROSS_UPPER) != 0, d_mask, ld_words, d_count);
}

int c2d_sat_rect_cross_pairs(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b, size_t row_base,
                             size_t col_base, int flags, uint32_t* d_pairs, size_t capacity, unsigned long long* d_count,
                             c2d_stream stream)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (n_a == 0 || n_b == 0) return C2D_OK;
    CrossPlanes A, B;
    if (int rc = cross_check(ctx, "c2d_sat_rect_cross_pairs", d_a, n_a, d_b, n_b, row_base, col_base, flags, A, B)) return rc;
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const bool upper = (flags & C2D_CROSS_UPPER) != 0;
    return cross_list_run(ctx, s, "c2d_sat_rect_cross_pairs", n_a, n_b, row_base, col_base, d_pairs, capacity, d_count,
                          [&](size_t r0, size_t rows, unsigned long long* d_mask, size_t words) {
                              CrossPlanes Ar;
                              for (int k = 0; k < 8; k++) Ar.p[k] = A.p[k] + r0;
                              return cross_mask_launch(ctx, s, Ar, rows, B, n_b, row_base + r0, col_base, upper, d_mask, words, d_count);
                          });
}

}  // extern "C"
