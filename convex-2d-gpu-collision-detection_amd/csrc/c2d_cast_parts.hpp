// c2d_cast_parts.hpp — what the two cast reductions share (c2d_cast.hip: all of B per query; c2d_cast_grid.hip: the polygons whose
// swept boxes meet the query's, through the grid): the 64-bit key a query's record starts as, and the first and last launch of
// c2d_cast.hip, whose kernels stay in that file.
#pragma once

#include "c2d_sweep_rule.hpp"

namespace c2d {

// The first eight bytes of a record between the passes: (bits of toi) << 32 | (col_base + j) of the best so far; all ones: nothing
// yet (no hit has that key: toi <= 1).
constexpr unsigned long long kCastNoKey = ~0ull;

// every record's key = kCastNoKey
int cast_launch_init(c2d_ctx* ctx, hipStream_t s, size_t n_a, c2d_cast* d_out);
// every record from its key: the winner's record recomputed by the sweep kernel's own routines with the call's motion planes, the
// miss record for kCastNoKey, the BAD_PAIR record for a query with a vertex count outside 1..rows (reported through the asynchronous
// error word)
int cast_launch_finalise(c2d_ctx* ctx, hipStream_t s, const PolySetDev& A, const PolySetDev& B, const float* d_a_dx, const float* d_a_dy,
                         const float* d_b_dx, const float* d_b_dy, size_t col_base, c2d_cast* d_out);

}  // namespace c2d
