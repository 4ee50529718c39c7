// c2d_cast_parts.hpp — what the two cast reductions share beyond the frame of c2d_set_best.hpp (c2d_cast.hip: all of B per query;
// c2d_cast_grid.hip: the polygons whose swept boxes meet the query's, through the grid): the last launch of c2d_cast.hip, whose kernel
// stays in that file.  A record's key starts as kSetNoKey (set_best_launch_init<3>); no hit has that key: toi <= 1.
#pragma once

#include "c2d_set_best.hpp"
#include "c2d_sweep_rule.hpp"

namespace c2d {

// every record from its key: the winner's record recomputed by the sweep kernel's own routines with the call's motion planes, the
// miss record for kSetNoKey, the BAD_PAIR record for a query with a vertex count outside 1..rows (reported through the asynchronous
// error word)
int cast_launch_finalise(c2d_ctx* ctx, hipStream_t s, const PolySetDev& A, const PolySetDev& B, const float* d_a_dx, const float* d_a_dy,
                         const float* d_b_dx, const float* d_b_dy, size_t col_base, c2d_cast* d_out);

}  // namespace c2d
