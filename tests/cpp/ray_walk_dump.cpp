// Prints what csrc/c2d_ray_walk.hpp enumerates for given grids and rays (built and run by tests/test_ray_grid_walk_cases_cpu.py with the
// address and undefined-behaviour sanitizers), so that the Python model of the walk (tests/ray_grid_model.py) can be compared with the
// header itself.  Input, from the file named on the command line or from stdin, every real number as a C hexadecimal float:
//   x0 y0 ix iy gx gy G n      one grid and the number of rays that follow
//   ox oy dx dy                n times (binary32 values)
// repeated until the input ends.  Output, one line per ray: "-" for a ray that is not walked, otherwise
//   W row0 row1 col0 col1 col0 col1 ...      W as a hexadecimal float, one (col0, col1) per key row of [row0, row1]
#include <cstdint>
#include <cstdio>
#include <string>

#include "c2d_ray_walk.hpp"

using namespace c2d;

int main(int argc, char** argv)
{
    FILE* in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    WalkGrid g;
    unsigned long n;
    std::string line;
    for (;;) {
        const int got = std::fscanf(in, "%la %la %la %la %u %u %la %lu", &g.x0, &g.y0, &g.ix, &g.iy, &g.gx, &g.gy, &g.G, &n);
        if (got == EOF) break;
        if (got != 8 || g.gx == 0 || g.gy == 0) { std::fprintf(stderr, "bad grid line\n"); return 2; }
        for (unsigned long i = 0; i < n; i++) {
            float q[4];
            if (std::fscanf(in, "%a %a %a %a", &q[0], &q[1], &q[2], &q[3]) != 4) { std::fprintf(stderr, "bad ray line\n"); return 2; }
            RayWalk w;
            if (!ray_walk_begin(g, ray_d(q[0], q[1], q[2], q[3]), w)) { std::puts("-"); continue; }
            if (w.row0 > w.row1 || w.row1 >= g.gy) { std::fprintf(stderr, "bad rows\n"); return 1; }
            char buf[64];
            line.clear();
            std::snprintf(buf, sizeof buf, "%a %u %u", w.W, w.row0, w.row1);
            line += buf;
            for (uint32_t R = w.row0; R <= w.row1; R++) {
                uint32_t c0, c1;
                ray_walk_row(g, w, R, c0, c1);
                if (c0 > c1 || c1 >= g.gx) { std::fprintf(stderr, "bad columns\n"); return 1; }
                std::snprintf(buf, sizeof buf, " %u %u", c0, c1);
                line += buf;
            }
            std::puts(line.c_str());
        }
    }
    if (in != stdin) std::fclose(in);
    return 0;
}
