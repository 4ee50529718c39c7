// c2d_clearance_parts.hpp — what the two clearance reductions share beyond the frame of c2d_set_best.hpp (c2d_clearance.hip: all of B
// per query; c2d_clearance_grid.hip: the polygons within a distance, through the grid): the last launch of c2d_clearance.hip, whose
// kernel stays in that file.  A record's key starts as kSetNoKey (set_best_launch_init<4>).
#pragma once

#include "c2d_set_best.hpp"

namespace c2d {

// every record from its key: the winner's record recomputed by the distance kernel's own routines, the NONE record for kSetNoKey,
// the BAD_PAIR record for a query with a vertex count outside 1..rows (reported through the asynchronous error word)
int clearance_launch_finalise(c2d_ctx* ctx, hipStream_t s, const PolySetDev& A, const PolySetDev& B, size_t col_base, c2d_clearance* d_out);

}  // namespace c2d
