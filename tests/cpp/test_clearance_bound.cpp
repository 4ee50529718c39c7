// test_clearance_bound.cpp — the certified bound of the clearance query (csrc/c2d_clearance_bound.hpp) on a CPU.  Built with
// -ffp-contract=off and -fsanitize=address,undefined by tests/test_clearance_bound_cpu.py, which feeds it the vertex boxes of pairs
// and judges the bounds against the numpy reference of the distance contract.
// usage: test_clearance_bound <in> <out>     in: per pair ten floats (A's xlo, xhi, ylo, yhi, c; then B's); out: one float lb2 per pair
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "c2d_clearance_bound.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<float> rows;
    float buf[10 * 1024];
    size_t got;
    while ((got = std::fread(buf, sizeof(float), 10 * 1024, in)) > 0) rows.insert(rows.end(), buf, buf + got);
    std::fclose(in);
    if (rows.size() % 10 != 0) return 4;
    std::vector<float> out(rows.size() / 10);
    for (size_t p = 0; p < out.size(); p++) {
        const float* r = &rows[10 * p];
        const c2d::ClearanceBox a{r[0], r[1], r[2], r[3], r[4]}, b{r[5], r[6], r[7], r[8], r[9]};
        out[p] = c2d::clearance_lb2(a, b);
        if (!(out[p] >= 0.0f)) return 5;   // never negative, never NaN
    }
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const size_t put = std::fwrite(out.data(), sizeof(float), out.size(), o);
    std::fclose(o);
    if (put != out.size()) return 7;
    std::printf("ok %zu\n", out.size());
    return 0;
}
