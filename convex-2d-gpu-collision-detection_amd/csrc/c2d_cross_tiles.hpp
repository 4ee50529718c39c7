// c2d_cross_tiles.hpp — how an N x M mask is cut into kernel launches.  Plain C++ with no HIP in it, so that the split can be
// tested on a CPU (tests/test_cross_tiles_cpu.py): its over-limit branches need more than 2^24 blocks to run in the library.
#pragma once

#include <cstddef>

namespace c2d {

// A mask kernel takes a one-dimensional grid of rows x cols blocks: row tiles [r0, r0 + rows) times column tiles [c0, c0 + cols),
// column tile fastest.  This walks row_tiles x col_tiles in launches of at most max_grid blocks: column strips of at most max_grid
// tiles (c0 ascending), inside a strip as many whole rows of it as fit (r0 ascending).  Calls launch(r0, c0, rows, cols) for
// each, stops at the first non-zero return and returns it; 0 when every launch was made.  max_grid >= 1.
template <class F>
int for_each_tile_launch(size_t row_tiles, size_t col_tiles, size_t max_grid, F&& launch)
{
    const size_t col_step = col_tiles < max_grid ? col_tiles : max_grid;
    for (size_t c0 = 0; c0 < col_tiles; c0 += col_step) {
        const size_t cols = col_tiles - c0 < col_step ? col_tiles - c0 : col_step;
        const size_t row_step = max_grid / cols;
        for (size_t r0 = 0; r0 < row_tiles; r0 += row_step) {
            const size_t rows = row_tiles - r0 < row_step ? row_tiles - r0 : row_step;
            if (int rc = launch(r0, c0, rows, cols)) return rc;
        }
    }
    return 0;
}

}  // namespace c2d
