// c2d_clearance_parts.hpp — what the two clearance reductions share (c2d_clearance.hip: all of B per query; c2d_clearance_grid.hip:
// the polygons within a distance, through the grid): the 64-bit key a query's record starts as, and the first and last launch of
// c2d_clearance.hip, whose kernels stay in that file.
#pragma once

#include "c2d_poly_pair.hpp"

namespace c2d {

// The first eight bytes of a record between the passes: (bits of dist) << 32 | (col_base + j) of the best so far; all ones: nothing yet.
constexpr unsigned long long kClrNoKey = ~0ull;

// every record's key = kClrNoKey
int clearance_launch_init(c2d_ctx* ctx, hipStream_t s, size_t n_a, c2d_clearance* d_out);
// every record from its key: the winner's record recomputed by the distance kernel's own routines, the NONE record for kClrNoKey,
// the BAD_PAIR record for a query with a vertex count outside 1..rows (reported through the asynchronous error word)
int clearance_launch_finalise(c2d_ctx* ctx, hipStream_t s, const PolySetDev& A, const PolySetDev& B, size_t col_base, c2d_clearance* d_out);

}  // namespace c2d
