// CPU test of csrc/c2d_ray_walk.hpp (built by tests/test_ray_walk_cpu.py with the address and undefined-behaviour sanitizers): the
// header's proof obligation — for a regular box inside the grid's bounds, ray_meets implies that the box's key lies in an enumerated
// range — on random grids (tiny ones, clamped edges, the 65 535-cell cap) and random segments (d = 0, axis-parallel, many cells long,
// end points on cell borders, wholly outside the bounds), and that the enumeration stays within 5 T + 9 cells, T being the cells the
// widened segment truly crosses: per key row the walk looks at the columns the segment spans in that row and the next (at most the
// cells crossed there), one more on the low side and at most one more per end for rounding; it looks at one row more than the
// segment crosses on the low side and at most one more per end for rounding.  A walk that degenerates to the box area fails that.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "c2d_ray_walk.hpp"

using namespace c2d;

static std::mt19937_64 rng(0xC2D17u);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static int pick(int n) { return (int)(rng() % (uint64_t)n); }

struct Grid {
    WalkGrid g;
    float lo_x, lo_y, hi_x, hi_y;   // the bounds
    double s;                       // the cell-size pick: boxes inside the bounds have an extent below it
};

// a grid as c2d_broad.hip's broad_grid_kernel makes it from bounds and a cell size
static Grid make_grid(float lo_x, float lo_y, float hi_x, float hi_y, float s)
{
    Grid G;
    const double kMax = 65535.0;
    const double ex = (double)hi_x - lo_x, ey = (double)hi_y - lo_y, inv_s = 1.0 / (double)s;
    G.g.x0 = lo_x;
    G.g.y0 = lo_y;
    G.g.ix = ex * inv_s > kMax - 1 ? (kMax - 1) / ex : inv_s;
    G.g.iy = ey * inv_s > kMax - 1 ? (kMax - 1) / ey : inv_s;
    G.g.gx = (uint32_t)std::floor(ex * G.g.ix) + 1u;
    G.g.gy = (uint32_t)std::floor(ey * G.g.iy) + 1u;
    G.g.G = std::fmax(std::fmax(std::fabs((double)lo_x), std::fabs((double)hi_x)), std::fmax(std::fabs((double)lo_y), std::fabs((double)hi_y)));
    G.lo_x = lo_x; G.lo_y = lo_y; G.hi_x = hi_x; G.hi_y = hi_y;
    G.s = s;
    return G;
}

static Grid random_grid(int kind)
{
    const double scale = std::ldexp(1.0, pick(61) - 30);
    const float s = (float)(scale * uni(0.5, 2.0));
    double cells_x, cells_y;
    switch (kind % 5) {
    case 0: cells_x = uni(0.0, 1.0); cells_y = uni(0.0, 1.0); break;            // a single cell, or nearly
    case 1: cells_x = uni(1.0, 40.0); cells_y = uni(1.0, 40.0); break;          // small: the crossing count is checked here
    case 2: cells_x = uni(1.0, 60.0); cells_y = uni(0.0, 2.0); break;           // a strip
    case 3: cells_x = uni(100.0, 60000.0); cells_y = uni(100.0, 60000.0); break;
    default: cells_x = uni(7e4, 1e7); cells_y = uni(10.0, 1e6); break;          // over the cap: larger cells
    }
    const double off = pick(3) == 0 ? 0.0 : uni(-1.0, 1.0) * s * std::ldexp(1.0, pick(24));
    const float lo_x = (float)off, lo_y = (float)(off * uni(-1.0, 1.0));
    const float hi_x = (float)(lo_x + cells_x * s), hi_y = (float)(lo_y + cells_y * s);
    return make_grid(lo_x, lo_y, hi_x, hi_y, s);
}

static uint32_t cx(const Grid& G, double v) { return walk_cell(v, G.g.x0, G.g.ix, G.g.gx); }
static uint32_t cy(const Grid& G, double v) { return walk_cell(v, G.g.y0, G.g.iy, G.g.gy); }

static float clampf(double v, float lo, float hi)
{
    float f = (float)v;
    return f < lo ? lo : (f > hi ? hi : f);
}

struct Seg { float ox, oy, dx, dy; };

static Seg random_segment(const Grid& G, int kind)
{
    const double w = (double)G.hi_x - G.lo_x, h = (double)G.hi_y - G.lo_y, cell_x = 1.0 / G.g.ix, cell_y = 1.0 / G.g.iy;
    const double span = std::fmax(std::fmax(w, h), G.s);
    double ox = G.lo_x + uni(-0.2, 1.2) * w, oy = G.lo_y + uni(-0.2, 1.2) * h;
    double len = G.s * std::ldexp(1.0, pick(12) - 4) * uni(0.5, 1.0), ang = uni(0.0, 6.283185307179586);
    double dx = len * std::cos(ang), dy = len * std::sin(ang);
    switch (kind % 8) {
    case 0: dx = dy = 0.0; break;                                               // a point
    case 1: dy = 0.0; break;                                                    // axis-parallel
    case 2: dx = 0.0; break;
    case 3: dx = uni(-1.5, 1.5) * w; dy = uni(-1.5, 1.5) * h; break;            // across the whole grid and beyond
    case 4:                                                                     // end points on cell borders
        ox = G.g.x0 + std::floor(uni(0.0, (double)G.g.gx)) * cell_x;
        oy = G.g.y0 + std::floor(uni(0.0, (double)G.g.gy)) * cell_y;
        dx = std::floor(uni(-3.0, 4.0)) * cell_x;
        dy = std::floor(uni(-3.0, 4.0)) * cell_y;
        break;
    case 5: ox = G.lo_x + (pick(2) ? -1.0 : 2.0) * span * uni(1.0, 50.0); break;   // wholly outside the bounds
    case 6: dy = dy * 1e-6; break;                                              // nearly flat
    default: break;
    }
    return Seg{(float)ox, (float)oy, (float)dx, (float)dy};
}

// the cells [R][c] the walk enumerates
struct Range { uint32_t row, c0, c1; };

static bool enumerate(const Grid& G, const Seg& sg, std::vector<Range>& out, RayWalk& w)
{
    out.clear();
    const RayD r = ray_d(sg.ox, sg.oy, sg.dx, sg.dy);
    if (!ray_walk_begin(G.g, r, w)) return false;
    if (w.row0 > w.row1 || w.row1 >= G.g.gy) { std::printf("bad rows\n"); std::exit(1); }
    for (uint32_t R = w.row0; R <= w.row1; R++) {
        uint32_t c0, c1;
        ray_walk_row(G.g, w, R, c0, c1);
        if (c0 > c1 || c1 >= G.g.gx) { std::printf("bad columns\n"); std::exit(1); }
        out.push_back(Range{R, c0, c1});
    }
    return true;
}

// does the segment, widened by W on every side, touch cell (R, c)?  The cell's rectangle comes from cell()'s own inverse; the first
// and the last cell of an axis reach to infinity (cell() clamps).
static bool truly_crosses(const Grid& G, const Seg& sg, double W, uint32_t R, uint32_t c)
{
    const long double inf = INFINITY;
    const long double xl = c == 0 ? -inf : (long double)G.g.x0 + (long double)c / G.g.ix - W;
    const long double xh = c + 1 >= G.g.gx ? inf : (long double)G.g.x0 + (long double)(c + 1) / G.g.ix + W;
    const long double yl = R == 0 ? -inf : (long double)G.g.y0 + (long double)R / G.g.iy - W;
    const long double yh = R + 1 >= G.g.gy ? inf : (long double)G.g.y0 + (long double)(R + 1) / G.g.iy + W;
    long double t0 = 0.0L, t1 = 1.0L;
    const long double o[2] = {sg.ox, sg.oy}, d[2] = {sg.dx, sg.dy}, lo[2] = {xl, yl}, hi[2] = {xh, yh};
    for (int a = 0; a < 2; a++) {
        if (d[a] == 0.0L) {
            if (o[a] < lo[a] || o[a] > hi[a]) return false;
        } else {
            long double ta = (lo[a] - o[a]) / d[a], tb = (hi[a] - o[a]) / d[a];
            if (ta > tb) { const long double t = ta; ta = tb; tb = t; }
            t0 = ta > t0 ? ta : t0;
            t1 = tb < t1 ? tb : t1;
        }
    }
    return t0 <= t1;
}

int main()
{
    long met_boxes = 0, counted = 0, listed = 0, tested_boxes = 0;
    double worst = 0.0;
    std::vector<Range> ranges;
    for (int gi = 0; gi < 200; gi++) {
        const Grid G = random_grid(gi);
        // cell() is monotone, and the bounds' corners are the first and the last cell
        if (cx(G, G.lo_x) != 0 || cy(G, G.lo_y) != 0 || cx(G, G.hi_x) != G.g.gx - 1 || cy(G, G.hi_y) != G.g.gy - 1) { std::printf("grid corners\n"); return 1; }
        for (int si = 0; si < 60; si++) {
            const Seg sg = random_segment(G, si + gi);
            RayWalk w;
            if (!enumerate(G, sg, ranges, w)) { listed++; continue; }
            const RayD r = ray_d(sg.ox, sg.oy, sg.dx, sg.dy);
            // boxes near the segment: around a point of it, moved by up to a few cells or by a few widenings, an extent below the pick
            for (int bi = 0; bi < 200; bi++) {
                const double t = pick(4) == 0 ? (double)pick(2) : uni(0.0, 1.0);
                const double reach = pick(2) ? G.s * uni(0.0, 2.5) : w.W * uni(0.0, 1.5);
                const double px = (double)sg.ox + t * sg.dx + uni(-1.0, 1.0) * reach, py = (double)sg.oy + t * sg.dy + uni(-1.0, 1.0) * reach;
                const double ext_x = pick(5) == 0 ? 0.0 : G.s * uni(0.0, 1.0), ext_y = pick(5) == 0 ? 0.0 : G.s * uni(0.0, 1.0);
                float xl = clampf(px - ext_x * uni(0.0, 1.0), G.lo_x, G.hi_x), yl = clampf(py - ext_y * uni(0.0, 1.0), G.lo_y, G.hi_y);
                float xh = clampf((double)xl + ext_x, xl, G.hi_x), yh = clampf((double)yl + ext_y, yl, G.hi_y);
                if (!(std::fmax(xh - xl, yh - yl) < (float)G.s)) continue;                      // not inside the bounds pass's pick
                const uint32_t kx = cx(G, xl), ky = cy(G, yl);
                if (cx(G, xh) - kx > 1u || cy(G, yh) - ky > 1u) continue;                       // spans more than two cells: wild, not regular
                tested_boxes++;
                if (!ray_meets(r, xl, xh, yl, yh)) continue;
                met_boxes++;
                bool found = false;
                for (const Range& q : ranges) found = found || (q.row == ky && q.c0 <= kx && kx <= q.c1);
                if (!found) {
                    std::printf("MISSED: grid %d (%u x %u) segment %d (%a %a %a %a) box (%a %a %a %a) key (%u, %u)\n", gi, G.g.gx, G.g.gy, si,
                                sg.ox, sg.oy, sg.dx, sg.dy, xl, xh, yl, yh, ky, kx);
                    return 1;
                }
            }
            // the size of the enumeration against the cells truly crossed (small grids: every cell is looked at)
            if (G.g.gx <= 64 && G.g.gy <= 64) {
                long T = 0, E = 0;
                for (uint32_t R = 0; R < G.g.gy; R++)
                    for (uint32_t c = 0; c < G.g.gx; c++) T += truly_crosses(G, sg, w.W, R, c) ? 1 : 0;
                for (const Range& q : ranges) E += (long)(q.c1 - q.c0) + 1;
                if (T < 1) { std::printf("no cell crossed\n"); return 1; }
                if (E > 5 * T + 9) {
                    std::printf("TOO WIDE: grid %d (%u x %u) segment %d (%a %a %a %a): %ld cells enumerated, %ld crossed\n", gi, G.g.gx, G.g.gy, si,
                                sg.ox, sg.oy, sg.dx, sg.dy, E, T);
                    return 1;
                }
                worst = std::fmax(worst, (double)E / (double)T);
                counted++;
            }
        }
    }
    // non-finite and huge rays are not walked
    {
        const Grid G = make_grid(0.0f, 0.0f, 10.0f, 10.0f, 1.0f);
        RayWalk w;
        const float bad[][4] = {{NAN, 0, 1, 0}, {0, INFINITY, 1, 0}, {0, 0, INFINITY, 0}, {0, 0, 1, -INFINITY}, {0x1p60f, 0, 1, 0}, {0, 0, 0, 0x1p61f}, {3e38f, 0, 3e38f, 0}};
        for (const auto& q : bad)
            if (ray_walk_begin(G.g, ray_d(q[0], q[1], q[2], q[3]), w)) { std::printf("a bad ray was walked\n"); return 1; }
        if (!ray_walk_begin(G.g, ray_d(0x1p59f, 0, 0x1p58f, 0), w)) { std::printf("a large finite ray was not walked\n"); return 1; }
        // ray_meets: a NaN or an infinity anywhere meets
        if (!ray_meets(ray_d(NAN, 0, 1, 0), 5, 6, 5, 6) || !ray_meets(ray_d(0, 0, INFINITY, 0), 5, 6, 5, 6) || !ray_meets(ray_d(0, 0, 1, 0), 5, INFINITY, 5, 6)) {
            std::printf("a non-finite input did not meet\n");
            return 1;
        }
        if (ray_meets(ray_d(0, 0, 1, 0), 5, 6, 5, 6) || !ray_meets(ray_d(0, 0, 10, 10), 5, 6, 5, 6)) { std::printf("ray_meets on a plain case\n"); return 1; }
    }
    if (met_boxes < 100000 || counted < 1000 || tested_boxes - met_boxes < 100000) { std::printf("vacuous: %ld met of %ld boxes, %ld counted\n", met_boxes, tested_boxes, counted); return 1; }
    std::printf("ok: %ld boxes met of %ld, %ld segments counted (worst %.2f enumerated per crossed cell), %ld not walked\n", met_boxes, tested_boxes, counted, worst, listed);
    return 0;
}
