// test_ray_strips.cpp — how a ray query deals the column tiles of B to the grid (csrc/c2d_ray_strips.hpp) on a CPU.  Built with
// -fsanitize=address,undefined by tests/test_ray_strips_cpu.py; exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "c2d_ray_strips.hpp"

#define CHECK(cond)                                                                                                                        \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            std::fprintf(stderr, "%s:%d: %s  (row_tiles %zu, col_tiles %zu, target %zu)\n", __FILE__, __LINE__, #cond, row_tiles, col_tiles, \
                         target);                                                                                                          \
            std::exit(1);                                                                                                                  \
        }                                                                                                                                  \
    } while (0)

int main()
{
    const size_t targets[] = {2, 3, 8, 64, 512, 2048};   // at least twice a CU count of 1 .. 1024
    size_t several = 0, capped = 0;
    for (size_t target : targets)
        for (size_t row_tiles = 1; row_tiles <= 70; row_tiles++)
            for (size_t col_tiles = 1; col_tiles <= 70; col_tiles++) {
                const size_t strips = c2d::ray_strip_count(row_tiles, col_tiles, target);
                CHECK(strips >= 1 && strips <= col_tiles);                        // never more strips than column tiles
                if (col_tiles == 1) CHECK(strips == 1);                           // a B that fits one tile takes one strip
                if (row_tiles == 1 && col_tiles >= 2) CHECK(strips >= 2);         // few rays: B is cut
                if (row_tiles >= target) CHECK(strips == 1);                      // many rays fill the device on their own
                size_t want = target / row_tiles;
                want = want < 1 ? 1 : want;
                CHECK(strips == (col_tiles < want ? col_tiles : want));           // min(col_tiles, max(1, target / row_tiles))
                if (strips > 1) CHECK(row_tiles * strips <= target);              // the cut never asks for more blocks than the target
                // every column tile in exactly one strip, the strips consecutive and none empty, sizes within one of each other
                std::vector<int> covered(col_tiles, 0);
                size_t next = 0, smallest = col_tiles, largest = 0;
                for (size_t s = 0; s < strips; s++) {
                    size_t first = ~(size_t)0, count = 0;
                    c2d::ray_strip_tiles(col_tiles, strips, s, first, count);
                    CHECK(first == next && count >= 1 && first + count <= col_tiles);
                    for (size_t c = first; c < first + count; c++) covered[c]++;
                    next = first + count;
                    smallest = count < smallest ? count : smallest;
                    largest = count > largest ? count : largest;
                }
                CHECK(next == col_tiles && largest - smallest <= 1);
                for (int c : covered) CHECK(c == 1);
                several += strips > 1;
                capped += strips == col_tiles && col_tiles > 1;
            }
    {
        const size_t row_tiles = 0, col_tiles = 0, target = 0;   // (for CHECK's message)
        CHECK(several > 0 && capped > 0);
    }
    // sizes the library meets: 2^24 row tiles, 2^26 column tiles; nothing overflows, the last strip ends at the last tile
    {
        const size_t row_tiles = 16, col_tiles = ((size_t)1 << 26) + 3, target = 2048;
        const size_t strips = c2d::ray_strip_count(row_tiles, col_tiles, target);
        CHECK(strips == 128);
        size_t first, count, end = 0;
        for (size_t s = 0; s < strips; s++) {
            c2d::ray_strip_tiles(col_tiles, strips, s, first, count);
            CHECK(first == end);
            end = first + count;
        }
        CHECK(end == col_tiles);
        CHECK(c2d::ray_strip_count((size_t)1 << 24, col_tiles, target) == 1);
    }
    std::puts("ok");
    return 0;
}
