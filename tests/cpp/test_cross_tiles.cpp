// test_cross_tiles.cpp — the cut of an N x M mask into launches (csrc/c2d_cross_tiles.hpp) on a CPU: the branches that split a
// mask need more than 2^24 blocks in the library, so they are driven here with small grid limits.  Built with
// -fsanitize=address,undefined by tests/test_cross_tiles_cpu.py; exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "c2d_cross_tiles.hpp"

struct Launch {
    size_t r0, c0, rows, cols;
    bool operator==(const Launch& o) const { return r0 == o.r0 && c0 == o.c0 && rows == o.rows && cols == o.cols; }
};

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            std::fprintf(stderr, "%s:%d: %s  (row_tiles %zu, col_tiles %zu, max_grid %zu)\n", __FILE__, __LINE__, #cond, row_tiles, \
                         col_tiles, max_grid);                                                                                   \
            std::exit(1);                                                                                                        \
        }                                                                                                                        \
    } while (0)

// the double loop of the two mask launchers as it stood before the split became a function, transcribed
static std::vector<Launch> loops_before(size_t row_tiles, size_t col_tiles, size_t kMaxGrid)
{
    std::vector<Launch> out;
    const size_t col_step = col_tiles < (size_t)kMaxGrid ? col_tiles : (size_t)kMaxGrid;
    for (size_t c0 = 0; c0 < col_tiles; c0 += col_step) {
        const size_t cols = col_tiles - c0 < col_step ? col_tiles - c0 : col_step;
        const size_t row_step = (size_t)kMaxGrid / cols;
        for (size_t r0 = 0; r0 < row_tiles; r0 += row_step) {
            const size_t rows = row_tiles - r0 < row_step ? row_tiles - r0 : row_step;
            out.push_back(Launch{r0, c0, rows, cols});
        }
    }
    return out;
}

static std::vector<Launch> launches_of(size_t row_tiles, size_t col_tiles, size_t max_grid)
{
    std::vector<Launch> out;
    const int rc = c2d::for_each_tile_launch(row_tiles, col_tiles, max_grid, [&](size_t r0, size_t c0, size_t rows, size_t cols) {
        out.push_back(Launch{r0, c0, rows, cols});
        return 0;
    });
    CHECK(rc == 0);
    return out;
}

int main()
{
    const size_t grids[] = {1, 2, 3, 7, 16, 64};
    size_t split = 0;
    for (size_t max_grid : grids)
        for (size_t row_tiles = 1; row_tiles <= 40; row_tiles++)
            for (size_t col_tiles = 1; col_tiles <= 40; col_tiles++) {
                const std::vector<Launch> got = launches_of(row_tiles, col_tiles, max_grid);
                std::vector<int> covered(row_tiles * col_tiles, 0);
                for (size_t k = 0; k < got.size(); k++) {
                    const Launch& l = got[k];
                    CHECK(l.rows >= 1 && l.cols >= 1);
                    CHECK(l.rows * l.cols <= max_grid);
                    CHECK(l.cols <= max_grid);
                    CHECK(l.r0 + l.rows <= row_tiles && l.c0 + l.cols <= col_tiles);
                    for (size_t r = l.r0; r < l.r0 + l.rows; r++)
                        for (size_t c = l.c0; c < l.c0 + l.cols; c++) covered[r * col_tiles + c]++;
                    if (k) {   // c0 ascending, then r0 ascending
                        const Launch& p = got[k - 1];
                        CHECK(l.c0 > p.c0 || (l.c0 == p.c0 && l.r0 > p.r0));
                    }
                }
                for (int c : covered) CHECK(c == 1);
                CHECK(got == loops_before(row_tiles, col_tiles, max_grid));
                split += got.size() > 1;
            }
    {
        const size_t row_tiles = 0, col_tiles = 0, max_grid = 0;   // (for CHECK's message)
        CHECK(split > 0);
    }
    // the library's limit: a mask of up to 40 x 40 tiles is one launch of all of it
    for (size_t row_tiles = 1; row_tiles <= 40; row_tiles++)
        for (size_t col_tiles = 1; col_tiles <= 40; col_tiles++) {
            const size_t max_grid = (size_t)1 << 24;
            const std::vector<Launch> got = launches_of(row_tiles, col_tiles, max_grid);
            CHECK(got.size() == 1 && (got[0] == Launch{0, 0, row_tiles, col_tiles}));
            CHECK(got == loops_before(row_tiles, col_tiles, max_grid));
        }
    // a callback's non-zero return stops the walk and comes back
    {
        const size_t row_tiles = 9, col_tiles = 5, max_grid = 3;
        const size_t all = launches_of(row_tiles, col_tiles, max_grid).size();
        for (size_t stop_at = 0; stop_at < all; stop_at++) {
            size_t calls = 0;
            const int rc = c2d::for_each_tile_launch(row_tiles, col_tiles, max_grid, [&](size_t, size_t, size_t, size_t) {
                return calls++ == stop_at ? -7 - (int)stop_at : 0;
            });
            CHECK(rc == -7 - (int)stop_at);
            CHECK(calls == stop_at + 1);
        }
    }
    std::puts("ok");
    return 0;
}
