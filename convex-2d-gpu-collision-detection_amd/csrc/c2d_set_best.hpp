// c2d_set_best.hpp — the best-key queries by a visit to all of B, as one frame: c2d_ray.hip (the polygon a ray
// touches first), c2d_clearance.hip (the polygon nearest to a query polygon), c2d_cast.hip (the polygon a moving polygon touches
// first).  The same queries through the grid are c2d_grid_best.hpp's.
//
// Mapping: queries over lanes, polygons of B wave-uniform.  A block of kSetBlock lanes owns kSetBlock queries, in registers, and a
// strip of consecutive column tiles of B (c2d_ray_strips.hpp): block b is row tile b / strips, strip b % strips.  Per tile it stages
// kSetCols polygons in LDS — per live edge one 16-byte entry {x0, y0, ex, ey}, the edge vector made once per polygon by the
// contracts' own two subtractions, and the count; a query adds what it wants per edge and per polygon — and walks them in index
// order: the polygon index is wave-uniform, so every loop runs to that polygon's own count and every LDS read is a broadcast.  A lane
// keeps a running (value bits, index) best under strict <, so the first of equal polygons stays.
//
// Three launches on the stream, no scratch, nothing read back (set_best_run):
//   1. init      set_best_init_kernel: every record's first eight bytes = kSetNoKey, "nothing yet"
//   2. main      the query's own kernel: per query and strip the smallest (value, j) as a 64-bit key, the value's bits in the high
//                word and col_base + j in the low word (every query's value is ordered as its bits are).  The strips of a row tile
//                meet in an atomic minimum on those eight bytes (set_best_publish), which does not depend on who arrives first.
//   3. finalise  the query's own kernel, one lane per query: the whole record from the key, the winner alone recomputed by the
//                contract's own sequence.
// What is here is what the three queries use with the machine code they had as three files written from one another
// (profiles/set_best_refactor_isa.txt).  The tile loop, the staging and — for the two polygon queries — the query polygon, the hoist,
// the first-axis pick and the finalise skeleton stay spelt out in each kernel: moved into a routine, each of them changed the code of
// the kernel it was taken from (the same file lists what was tried).
#pragma once

#include "c2d_poly_pair.hpp"
#include "c2d_ray_strips.hpp"

namespace c2d {

constexpr int kSetBlock = 256;   // queries per block: one per lane
constexpr int kSetCols = 64;     // polygons of B per staged tile
constexpr int kSetK = C2D_POLY_KMAX;
// The first eight bytes of a record between the passes: (bits of the value) << 32 | (col_base + j) of the best so far; all ones:
// nothing yet (no candidate has that key: no query's value is a NaN).
constexpr unsigned long long kSetNoKey = ~0ull;

template <int kWords>   // a record in 64-bit words
__global__ __launch_bounds__(kSetBlock) void set_best_init_kernel(size_t n, unsigned long long* __restrict__ out)
{
    const size_t step = (size_t)gridDim.x * kSetBlock;
    for (size_t i = (size_t)blockIdx.x * kSetBlock + threadIdx.x; i < n; i += step) out[kWords * i] = kSetNoKey;
}

// 1. every record's key = kSetNoKey.  Each stride is instantiated in its query's own file (2: c2d_ray.hip, 3: c2d_cast.hip,
// 4: c2d_clearance.hip); the grid files only call it, for a call with an empty B.
template <int kWords>
int set_best_launch_init(c2d_ctx* ctx, hipStream_t s, size_t n, void* d_out)
{
    hipLaunchKernelGGL(set_best_init_kernel<kWords>, dim3(grid_for(n, kSetBlock, 1 << 16)), dim3(kSetBlock), 0, s, n, static_cast<unsigned long long*>(d_out));
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}
extern template int set_best_launch_init<2>(c2d_ctx*, hipStream_t, size_t, void*);
extern template int set_best_launch_init<3>(c2d_ctx*, hipStream_t, size_t, void*);
extern template int set_best_launch_init<4>(c2d_ctx*, hipStream_t, size_t, void*);

// The three launches of a call with n queries against n_b polygons: init, main unless B is empty, finalise.
// main(blocks, col_tiles, strips) launches the query's main kernel on `blocks` blocks of kSetBlock lanes and finalise() its last
// pass; both return C2D_OK or the refusal.
template <int kWords, class Main, class Finalise>
int set_best_run(c2d_ctx* ctx, hipStream_t s, size_t n, size_t n_b, void* d_out, Main main, Finalise finalise)
{
    if (int rc = set_best_launch_init<kWords>(ctx, s, n, d_out)) return rc;
    if (n_b != 0) {
        const size_t row_tiles = (n + kSetBlock - 1) / kSetBlock, col_tiles = (n_b + kSetCols - 1) / kSetCols;
        const int cus = ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 1;
        const size_t strips = ray_strip_count(row_tiles, col_tiles, (size_t)cus * 8);   // eight blocks of 256 fill a CU
        // row_tiles <= 2^24; with more than one strip, row_tiles * strips <= 8 * cus
        if (int rc = main((unsigned)(row_tiles * strips), col_tiles, (uint32_t)strips)) return rc;
    }
    return finalise();
}

// the key (bits, col_base + j) into the atomic minimum on the first eight bytes of record i
template <class Out>
C2D_DEV void set_best_publish(uint32_t bits, uint32_t col_base, uint32_t j, Out* out, size_t i)
{
    constexpr size_t kWords = sizeof(Out) / 8;
    const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned long long)(col_base + j);
    __hip_atomic_fetch_min(reinterpret_cast<unsigned long long*>(out) + kWords * i, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the query polygon turned by one slot: slot r takes slot r + 1, slot 15 takes slot 0
C2D_DEV void set_best_turn(float (&x)[kSetK], float (&y)[kSetK])
{
    const float fx = x[0], fy = y[0];
#pragma unroll
    for (int r = 0; r + 1 < kSetK; r++) {
        x[r] = x[r + 1];
        y[r] = y[r + 1];
    }
    x[kSetK - 1] = fx;
    y[kSetK - 1] = fy;
}

}  // namespace c2d
