// c2d_ray_strips.hpp — how the columns of a ray query (c2d_ray.hip) are dealt to the grid.  Plain C++ (under hipcc the functions are also
// marked for the device: the kernel asks for its own strip), so that the rule can be tested on a CPU (tests/test_ray_strips_cpu.py).
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define C2D_RAY_HD __host__ __device__
#else
#define C2D_RAY_HD
#endif

namespace c2d {

// A block of the ray kernel owns one row tile (256 rays) and one STRIP of consecutive column tiles of B, which it walks one tile at
// a time; the strips of a row tile are combined per ray by an atomic minimum.  With many row tiles one strip per row tile fills
// the device and no two blocks meet on a ray.  With few, B is cut so that about `target` blocks run (the caller passes at least
// twice the CU count): min(col_tiles, max(1, target / row_tiles)).  One row tile against two or more column tiles therefore takes
// several strips whenever target >= 2, and a B that fits one tile always takes one.  row_tiles, col_tiles >= 1.
C2D_RAY_HD inline size_t ray_strip_count(size_t row_tiles, size_t col_tiles, size_t target)
{
    size_t want = target / row_tiles;
    if (want < 1) want = 1;
    return col_tiles < want ? col_tiles : want;
}

// The column tiles [first, first + count) of strip s of `strips` (1 <= strips <= col_tiles, s < strips): consecutive, every tile in
// exactly one strip, sizes that differ by at most one (the first col_tiles % strips strips are the longer ones), none empty.
C2D_RAY_HD inline void ray_strip_tiles(size_t col_tiles, size_t strips, size_t s, size_t& first, size_t& count)
{
    const size_t base = col_tiles / strips, extra = col_tiles % strips;
    first = s * base + (s < extra ? s : extra);
    count = base + (s < extra ? 1 : 0);
}

}  // namespace c2d
