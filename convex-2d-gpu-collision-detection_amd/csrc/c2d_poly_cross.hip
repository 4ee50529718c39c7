// c2d_poly_cross.hip — all-pairs convex polygon SAT for gfx950 (MI355X): every polygon of a set A against every polygon of a set B.
//
// Result (i, j) is the boolean of the pairwise polygon kernel (c2d_poly.hip, c2d_sat_poly_pairs_rows) on the pair (A_i, B_j), bit
// for bit: true normals (-e.y, e.x) of all edges of both polygons, unfused projections nx * x + ny * y, strict <, padding slots never
// interpreted, and the NaN rule of first_projections_ordered.  The pairwise kernel evaluates up to (ka + kb)^2 projections for a pair
// that collides.  Here everything that depends on ONE polygon is computed once per polygon, by the same IEEE operations as inside a
// pair: its neutral padding (slots >= k repeat vertex 0), its edge normals, and for each of its own normals the min / max of its OWN
// vertices' projections with the NaN rule of its own first projection folded in (a NaN projection of vertex 0 makes the interval
// (-inf, +inf), with which neither comparison of utils.cu:178 can hold: the axis does not separate, exactly as the unordered compare
// decides it).  Per pair there remain the 2 ka kb cross projections and the comparisons.
//
// Mapping: a block of 256 lanes owns 256 consecutive rows of A, one per lane: the lane's padded vertices (32 VGPRs) and the
// intervals of its own vertices on its own 16 normals (32 VGPRs).  The block stages 64 columns of B at a time in LDS, each as a
// record of 104 floats: padded vertices, normals, own intervals, the vertex mean, and a 16-entry table "direction sector -> the
// edge whose normal points best that way".  The column index is wave-uniform.
//   phase 1, one pair per lane: the direction from B_j's vertex mean to A_i's picks a sector (fast arithmetic: it only chooses
//     WHICH canonical axis is tried), the table gives an edge of B_j, and that one axis is evaluated canonically: B_j's interval
//     comes from the record, A_i's vertices are projected from registers.  The result is an OR over axes, so an axis that separates
//     decides the pair.
//   phase 2, the pairs of the column that the first axis did not decide, in one of two forms chosen per wave and column:
//     few of them (fewer than kPcSerialMin): 32 lanes per pair, two pairs side by side: the owner lane parks its vertices and
//     intervals in a 256-byte LDS slot of its wave; lane (side, a) owns axis a of A_i (side 0) or of B_j (side 1), takes that axis'
//     own interval from the slot or the record and projects the OTHER polygon's vertices: 16 projections per lane where the
//     pairwise kernel makes 32.
//     many of them: every lane evaluates its own pair in full from registers (its axes and intervals, B_j's vertices from eight
//     broadcast reads; then B_j's axes and intervals from the record): no parking, and no lane idles.  Parking costs sixteen
//     16-byte LDS stores per pair and made the lanes-over-axes form LDS-bound on a dense scene (0.59 x the pairwise kernel,
//     1.67 x with this form: profiles/r09_poly_cross_bench.txt).
// A lane builds one 64-bit mask word per 64 columns and stores it with one 8-byte store.  With C2D_CROSS_UPPER untested pairs are
// never evaluated, and a block skips every word that lies on or below the diagonal for all of its rows.
//
// The pair list is the rectangle list's machinery (cross_list_run, c2d_cross.hpp) over this mask kernel.
#include "c2d_cross.hpp"
#include "c2d_math.hpp"
#include "c2d_count.hpp"
#include "c2d_wave.hpp"
#include "c2d_poly_pair.hpp"   // PolySetDev, poly_set_check

namespace c2d {

constexpr int kPcBlock = 256;     // rows of A per block: one per lane
constexpr int kPcCols = 256;      // columns of B per block: four mask words, staged 64 at a time
constexpr int kPcSub = 64;
constexpr int kPcK = C2D_POLY_KMAX;
static_assert(kPcK == 16, "the record layout and the lane roles of phase 2 are written for 16 vertex slots");

// one staged column of B (floats): vertices (x, y) interleaved | nx | ny | lo | hi | sector table (16 bytes) | mean x, y | count
constexpr int kRecV = 0, kRecNx = 32, kRecNy = 48, kRecLo = 64, kRecHi = 80, kRecTab = 96, kRecCx = 100, kRecCy = 101, kRecK = 102;
constexpr int kRecFloats = 104;   // 416 bytes: 16-byte aligned records
constexpr int kRecBad = 0x100;    // bit of the count word: the column's vertex count is out of range
// one parked row of A (floats): vertices (x, y) interleaved | lo | hi
constexpr int kParkLo = 32, kParkHi = 48, kParkFloats = 64;
// phase 2: a column with at least this many undecided rows in a wave is evaluated one pair per lane, below it two pairs per trip
// with lanes over axes (a full per-lane evaluation costs about what eight trips cost)
constexpr int kPcSerialMin = 16;

// Direction -> one of 16 sectors: the octant (signs, |dy| > |dx|) and which side of 22.5 degrees inside it.  Heuristic only: any
// input, NaN included, gives a number in 0..15.
C2D_DEV uint32_t pc_sector(float dx, float dy)
{
    const float fx = __builtin_fabsf(dx), fy = __builtin_fabsf(dy);
    const bool swap = fy > fx;
    const float big = swap ? fy : fx, small = swap ? fx : fy;
    const bool far = small > 0.41421356f * big;
    return (__float_as_uint(dx) >> 31) | ((__float_as_uint(dy) >> 31) << 1) | (swap ? 4u : 0u) | (far ? 8u : 0u);
}

// the middle direction of sector s (11.25 or 33.75 degrees inside its octant)
C2D_DEV void pc_sector_dir(uint32_t s, float& u, float& v)
{
    const float c = (s & 8u) ? 0.83146961f : 0.98078528f, sn = (s & 8u) ? 0.55557023f : 0.19509032f;
    u = (s & 4u) ? sn : c;
    v = (s & 4u) ? c : sn;
    u = (s & 1u) ? -u : u;
    v = (s & 2u) ? -v : v;
}

// One launch covers row tiles [row_tile0, row_tile0 + gridDim.x / col_tiles) and column tiles [col_tile0, col_tile0 + col_tiles)
// (one-dimensional grid: the count's wave numbering is blockIdx.x).  Row i of A is global row row_base + i, column j of B global
// column col_base + j; diag = row_base - col_base.  With `upper`, bit j of row i is tested only if col_base + j > row_base + i.
__global__ __launch_bounds__(kPcBlock) void poly_cross_mask_kernel(PolySetDev A, PolySetDev B, size_t row_tile0, size_t col_tile0, uint32_t col_tiles,
                                                                    long long diag, int upper, unsigned long long* __restrict__ mask, size_t ld_words,
                                                                    unsigned long long* __restrict__ d_count, CountWs words,
                                                                    uint32_t* __restrict__ async_err)
{
    __shared__ __attribute__((aligned(16))) float s_rec[kPcSub][kRecFloats];                 // 26 KiB
    __shared__ __attribute__((aligned(16))) float s_park[kPcBlock / 64][2][kParkFloats];     // 2 KiB: two slots per wave
    const uint32_t lane = threadIdx.x, wl = lane & 63u, wave = lane >> 6;
    const size_t rt = row_tile0 + blockIdx.x / col_tiles;
    const size_t j0 = (col_tile0 + blockIdx.x % col_tiles) * (size_t)kPcCols;
    const float inf = __builtin_inff();

    // ---- the lane's row of A: count, padded vertices, vertex mean, own intervals -------------------------------------------
    const size_t i = rt * kPcBlock + lane;
    const bool row_valid = i < A.n;
    int ka = row_valid ? (A.k ? (int)A.k[i] : A.rows) : 1;
    const bool bad_a = ka < 1 || ka > A.rows;   // out of range: clamped (memory safety), reported, every pair of the row reads 0
    ka = ka < 1 ? 1 : (ka > A.rows ? A.rows : ka);
    if (__ballot(bad_a) != 0ull && wl == 0) __hip_atomic_fetch_or(async_err, C2D_ASYNC_ERR_POLY_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int kmax_a = (int)wave_max_u32((uint32_t)ka);   // wave-uniform loop bound: slots above it repeat vertex 0 in every lane
    float ax[kPcK], ay[kPcK];
#pragma unroll
    for (int r = 0; r < kPcK; r++) {
        ax[r] = 0.0f;
        ay[r] = 0.0f;
        if (r < kmax_a && row_valid && r < ka) {   // r < ka <= A.rows: inside the planes
            ax[r] = A.vx[(size_t)r * A.stride + i];
            ay[r] = A.vy[(size_t)r * A.stride + i];
        }
    }
    float sax = ax[0], say = ay[0];
#pragma unroll
    for (int r = 1; r < kPcK; r++) {
        const bool used = r < ka;
        ax[r] = used ? ax[r] : ax[0];   // neutral padding: a repeated vertex adds a zero-length edge and repeats a projection
        ay[r] = used ? ay[r] : ay[0];
        if (r < kmax_a) { sax += ax[r]; say += ay[r]; }
    }
    const float inv_ka = __builtin_amdgcn_rcpf((float)ka);
    const float cax = (sax - (float)(kmax_a - ka) * ax[0]) * inv_ka, cay = (say - (float)(kmax_a - ka) * ay[0]) * inv_ka;
    // Own intervals.  An axis a >= kmax_a is the zero vector for every lane of the wave: its projections are +-0 or NaN, so it
    // never separates ((-inf, +inf) says the same).  Vertex slots >= kmax_a repeat vertex 0: no new projection value.
    float alo[kPcK], ahi[kPcK];
#pragma unroll
    for (int a = 0; a < kPcK; a++) {
        alo[a] = -inf;
        ahi[a] = inf;
        if (a < kmax_a) {
            const int a1 = (a + 1) & (kPcK - 1);
            const float nx = -(ay[a1] - ay[a]), ny = ax[a1] - ax[a];
            float mn = inf, mx = -inf;
#pragma unroll
            for (int r = 0; r < kPcK; r++)
                if (r < kmax_a) poly_minmax(nx, ny, ax[r], ay[r], mn, mx);
            const bool nan0 = __builtin_isnan(nx * ax[0] + ny * ay[0]);
            alo[a] = nan0 ? -inf : mn;
            ahi[a] = nan0 ? inf : mx;
        }
    }

    const size_t words_b = (B.n + 63) / 64;
    uint32_t my_count = 0;
#pragma unroll 1
    for (int w = 0; w < kPcCols / kPcSub; w++) {
        const size_t word = j0 / 64 + (size_t)w;
        if (word >= words_b) break;   // (block-uniform)
        const size_t jb = j0 + (size_t)kPcSub * w;
        const uint32_t nj = (uint32_t)(B.n - jb < (size_t)kPcSub ? B.n - jb : (size_t)kPcSub);
        // upper: bit b of row i is tested iff col_base + jb + b > row_base + i, i.e. b > t
        const long long t = (long long)i + diag - (long long)jb;
        const long long t_block = (long long)(rt * kPcBlock) + diag - (long long)jb;   // the block's first row: the smallest t
        unsigned long long bits = 0;
        if (!(upper && t_block >= 63)) {   // (block-uniform) else: every column on or below the diagonal for every row of the block
            // ---- stage 64 columns: padded vertices and the count ---------------------------------------------------------
            __syncthreads();   // the previous sub-tile's readers are done
            {
                const uint32_t c = lane & 63u, g = lane >> 6;
                const size_t j = jb + c;
                const bool valid = c < nj;
                int kb = valid ? (B.k ? (int)B.k[j] : B.rows) : 1;
                const bool bad_b = kb < 1 || kb > B.rows;
                kb = kb < 1 ? 1 : (kb > B.rows ? B.rows : kb);
                if (__ballot(bad_b) != 0ull && wl == 0)
                    __hip_atomic_fetch_or(async_err, C2D_ASYNC_ERR_POLY_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const float v0x = valid ? B.vx[j] : 0.0f, v0y = valid ? B.vy[j] : 0.0f;
#pragma unroll
                for (int m = 0; m < kPcK / 4; m++) {
                    const int r = (int)g + 4 * m;
                    float x = v0x, y = v0y;
                    if (valid && r < kb) {   // r < kb <= B.rows: inside the planes
                        x = B.vx[(size_t)r * B.stride + j];
                        y = B.vy[(size_t)r * B.stride + j];
                    }
                    *reinterpret_cast<float2*>(&s_rec[c][kRecV + 2 * r]) = make_float2(x, y);
                }
                if (g == 0) s_rec[c][kRecK] = __int_as_float(kb | (bad_b ? kRecBad : 0));
            }
            __syncthreads();
            // ---- hoist: lane (column c, axis a) -> normal and own interval; lane (c, 0) also the vertex mean -----------------
#pragma unroll 1
            for (int m = 0; m < kPcSub * kPcK / kPcBlock; m++) {
                const uint32_t item = lane + (uint32_t)kPcBlock * m, c = item >> 4, a = item & 15u;
                float* rec = s_rec[c];
                const float2* V = reinterpret_cast<const float2*>(rec + kRecV);
                const f32x4* V4 = reinterpret_cast<const f32x4*>(rec + kRecV);
                const float2 e0 = V[a], e1 = V[(a + 1u) & 15u];
                const float nx = -(e1.y - e0.y), ny = e1.x - e0.x;
                float mn = inf, mx = -inf, sx = 0.0f, sy = 0.0f;
#pragma unroll
                for (int r2 = 0; r2 < kPcK / 2; r2++) {
                    const f32x4 q = V4[r2];
                    poly_minmax(nx, ny, q.x, q.y, mn, mx);
                    poly_minmax(nx, ny, q.z, q.w, mn, mx);
                    sx += q.x + q.z;
                    sy += q.y + q.w;
                }
                const bool nan0 = __builtin_isnan(nx * V[0].x + ny * V[0].y);
                rec[kRecNx + a] = nx;
                rec[kRecNy + a] = ny;
                rec[kRecLo + a] = nan0 ? -inf : mn;
                rec[kRecHi + a] = nan0 ? inf : mx;
                if (a == 0) {   // mean of the real vertices: the sums hold (16 - k) extra copies of vertex 0
                    const int kb = __float_as_int(rec[kRecK]) & 0xff;
                    const float inv = __builtin_amdgcn_rcpf((float)kb), extra = (float)(kPcK - kb);
                    rec[kRecCx] = (sx - extra * V[0].x) * inv;
                    rec[kRecCy] = (sy - extra * V[0].y) * inv;
                }
            }
            __syncthreads();
            // ---- sector table: lane (column c, sector s) -> the edge whose normal points best into the sector ----------------
#pragma unroll 1
            for (int m = 0; m < kPcSub * kPcK / kPcBlock; m++) {
                const uint32_t item = lane + (uint32_t)kPcBlock * m, c = item >> 4, sct = item & 15u;
                float* rec = s_rec[c];
                const float2* V = reinterpret_cast<const float2*>(rec + kRecV);
                float u, v;
                pc_sector_dir(sct, u, v);
                {   // clockwise polygons have inward-pointing (-ey, ex): the preferred direction flips (sign of the first corner)
                    const float2 p0 = V[0], p1 = V[1], p2 = V[2];
                    const float cr = (p1.x - p0.x) * (p2.y - p0.y) - (p1.y - p0.y) * (p2.x - p0.x);
                    const uint32_t sgn = __float_as_uint(cr) & 0x80000000u;
                    u = __uint_as_float(__float_as_uint(u) ^ sgn);
                    v = __uint_as_float(__float_as_uint(v) ^ sgn);
                }
                float best = -inf;
                uint32_t best_e = 0;
#pragma unroll
                for (int e = 0; e < kPcK; e++) {
                    const float nx = rec[kRecNx + e], ny = rec[kRecNy + e];
                    const float sc = fma_(nx, u, ny * v) * __builtin_amdgcn_rsqf(fma_(nx, nx, ny * ny));   // zero edge: NaN, never better
                    const bool better = sc > best;
                    best = better ? sc : best;
                    best_e = better ? (uint32_t)e : best_e;
                }
                reinterpret_cast<uint8_t*>(rec + kRecTab)[sct] = (uint8_t)best_e;
            }
            __syncthreads();
            // ---- the pairs: a wave whose 64 rows are all on or below the diagonal of this word has nothing to test -----------
            const long long t_wave = (long long)(rt * kPcBlock + (lane & ~63u)) + diag - (long long)jb;
            if (!(upper && t_wave >= 63)) {
                const bool row_live = row_valid && !bad_a;
                const int t_lane = upper ? (int)(t < -1 ? -1 : (t > 64 ? 64 : t)) : -1;   // the pair of bit b is tested iff b > t_lane
#pragma unroll 1
                for (uint32_t b = 0; b < nj; b++) {
                    const float* rec = s_rec[b];
                    const int kinfo = __builtin_amdgcn_readfirstlane(__float_as_int(rec[kRecK]));
                    if (kinfo & kRecBad) continue;   // (wave-uniform) a column with a count out of range: every bit 0
                    // phase 1: one axis of B_j, chosen by the direction from B_j's vertex mean to A_i's
                    const uint32_t sct = pc_sector(cax - rec[kRecCx], cay - rec[kRecCy]);
                    const uint32_t e = reinterpret_cast<const uint8_t*>(rec + kRecTab)[sct];
                    const float nx = rec[kRecNx + e], ny = rec[kRecNy + e], lo = rec[kRecLo + e], hi = rec[kRecHi + e];
                    float mn = inf, mx = -inf;
#pragma unroll
                    for (int r = 0; r < kPcK; r++)
                        if (r < kmax_a) poly_minmax(nx, ny, ax[r], ay[r], mn, mx);
                    // (B_j's own first projection is folded into lo / hi; A_i's is checked here: first_projections_ordered)
                    const bool sep = ((hi < mn) || (mx < lo)) && !__builtin_isnan(nx * ax[0] + ny * ay[0]);
                    bool coll = row_live && (int)b > t_lane && !sep;
                    // phase 2: the pairs the first axis did not decide, two per trip, 32 lanes each
                    unsigned long long todo = __ballot(coll);
                    const int kb = kinfo & 0xff;
                    if (__popcll(todo) >= kPcSerialMin) {
                        // phase 2, crowded column: every lane evaluates its own pair in full, in registers.  A's axes with their
                        // own intervals against B_j's vertices (eight broadcast reads), then B_j's axes with theirs from the record
                        // against A_i's vertices.  Axes >= the counts are zero vectors (never separate); vertex slots >= the counts
                        // repeat vertex 0.  No parking, no lane idles while most of the wave is undecided.
                        float bx[kPcK], by[kPcK];
                        const f32x4* B4 = reinterpret_cast<const f32x4*>(rec + kRecV);
#pragma unroll
                        for (int r2 = 0; r2 < kPcK / 2; r2++) {
                            const f32x4 q = B4[r2];
                            bx[2 * r2] = q.x; by[2 * r2] = q.y; bx[2 * r2 + 1] = q.z; by[2 * r2 + 1] = q.w;
                        }
                        bool sep2 = false;
#pragma unroll
                        for (int a = 0; a < kPcK; a++) {
                            if (a < kmax_a) {
                                const int a1 = (a + 1) & (kPcK - 1);
                                const float qnx = -(ay[a1] - ay[a]), qny = ax[a1] - ax[a];
                                float qmn = inf, qmx = -inf;
#pragma unroll
                                for (int r = 0; r < kPcK; r++)
                                    if (r < kb) poly_minmax(qnx, qny, bx[r], by[r], qmn, qmx);
                                sep2 |= ((ahi[a] < qmn) || (qmx < alo[a])) && !__builtin_isnan(qnx * bx[0] + qny * by[0]);
                            }
                        }
#pragma unroll 1
                        for (int eb = 0; eb < kb; eb++) {
                            const float qnx = rec[kRecNx + eb], qny = rec[kRecNy + eb], qlo = rec[kRecLo + eb], qhi = rec[kRecHi + eb];
                            float qmn = inf, qmx = -inf;
#pragma unroll
                            for (int r = 0; r < kPcK; r++)
                                if (r < kmax_a) poly_minmax(qnx, qny, ax[r], ay[r], qmn, qmx);
                            sep2 |= ((qhi < qmn) || (qmx < qlo)) && !__builtin_isnan(qnx * ax[0] + qny * ay[0]);
                        }
                        coll = coll && !sep2;
                    } else if (todo) {
                        const int kq = (kmax_a > kb ? kmax_a : kb);   // both loops run to the larger count: padding is neutral
                        const uint32_t side = (wl >> 4) & 1u, a = wl & 15u;
                        while (todo) {
                            const int o0 = __ffsll((long long)todo) - 1;
                            todo &= todo - 1;
                            const int o1 = todo ? __ffsll((long long)todo) - 1 : -1;
                            todo &= todo - (todo ? 1ull : 0ull);
                            if ((int)wl == o0 || (int)wl == o1) {
                                f32x4* S4 = reinterpret_cast<f32x4*>(s_park[wave][(int)wl == o1 ? 1 : 0]);
#pragma unroll
                                for (int r = 0; r < kPcK / 2; r++) S4[r] = f32x4{ax[2 * r], ay[2 * r], ax[2 * r + 1], ay[2 * r + 1]};
#pragma unroll
                                for (int r = 0; r < kPcK / 4; r++) {
                                    S4[kParkLo / 4 + r] = f32x4{alo[4 * r], alo[4 * r + 1], alo[4 * r + 2], alo[4 * r + 3]};
                                    S4[kParkHi / 4 + r] = f32x4{ahi[4 * r], ahi[4 * r + 1], ahi[4 * r + 2], ahi[4 * r + 3]};
                                }
                            }
                            wave_lds_sync();
                            const float* P = s_park[wave][(wl >> 5) != 0u && o1 >= 0 ? 1 : 0];   // (without a second pair both halves test the first)
                            const float2* PV = reinterpret_cast<const float2*>(P);
                            const float2 e0 = PV[a], e1 = PV[(a + 1u) & 15u];
                            // side 0: axis a of A_i, own interval parked, B_j's vertices projected; side 1: axis a of B_j, A_i's vertices
                            const float qnx = side ? rec[kRecNx + a] : -(e1.y - e0.y), qny = side ? rec[kRecNy + a] : e1.x - e0.x;
                            const float qlo = side ? rec[kRecLo + a] : P[kParkLo + a], qhi = side ? rec[kRecHi + a] : P[kParkHi + a];
                            const f32x4* Q4 = reinterpret_cast<const f32x4*>(side ? P : rec + kRecV);
                            const f32x4 q0 = Q4[0];
                            const float first = qnx * q0.x + qny * q0.y;
                            float qmn = inf, qmx = -inf;
                            for (int r2 = 0; 2 * r2 < kq; r2++) {
                                const f32x4 q = Q4[r2];
                                poly_minmax(qnx, qny, q.x, q.y, qmn, qmx);
                                poly_minmax(qnx, qny, q.z, q.w, qmn, qmx);
                            }
                            const unsigned long long bal = __ballot(((qhi < qmn) || (qmx < qlo)) && !__builtin_isnan(first));
                            coll = (int)wl == o0 ? (uint32_t)bal == 0u : coll;
                            coll = (int)wl == o1 ? (uint32_t)(bal >> 32) == 0u : coll;
                            wave_lds_sync();   // the slots are rewritten by the next trip
                        }
                    }
                    bits |= coll ? (1ull << b) : 0ull;
                }
            }
        }
        if (row_valid) {
            mask[i * ld_words + word] = bits;
            my_count += (uint32_t)__popcll(bits);
        }
    }
    if (d_count) wave_count_arrive(my_count, d_count, words);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// Shared argument checks of both forms; C2D_OK or the status to return.
static int poly_cross_check(c2d_ctx* ctx, const char* what, const c2d_poly_set* a, const c2d_poly_set* b, size_t row_base, size_t col_base, int flags,
                            PolySetDev& A, PolySetDev& B)
{
    if (int rc = poly_set_check(ctx, what, "a", a, A)) return rc;
    if (int rc = poly_set_check(ctx, what, "b", b, B)) return rc;
    return cross_check_flags_bases(ctx, what, A.n, B.n, row_base, col_base, flags);
}

// The mask of rows [0, A.n) x columns [0, B.n) into `mask` (row stride ld_words), in launches of at most kMaxGrid blocks.
static int cross_mask_launch(c2d_ctx* ctx, hipStream_t s, const PolySetDev& A, const PolySetDev& B, size_t row_base, size_t col_base, bool upper,
                             unsigned long long* mask, size_t ld_words, unsigned long long* d_count)
{
    const size_t row_tiles = (A.n + kPcBlock - 1) / kPcBlock, col_tiles = (B.n + kPcCols - 1) / kPcCols;
    const long long diag = (long long)row_base - (long long)col_base;
    return for_each_tile_launch(row_tiles, col_tiles, (size_t)kMaxGrid, [&](size_t r0, size_t c0, size_t rows, size_t cols) {
        const size_t grid = rows * cols;
        hipLaunchKernelGGL(poly_cross_mask_kernel, dim3((unsigned)grid), dim3(kPcBlock), 0, s, A, B, r0, c0, (uint32_t)cols, diag, upper ? 1 : 0, mask,
                           ld_words, d_count, workspace_count_ticket(ctx, s, grid * (kPcBlock / 64), d_count != nullptr), ctx->d_async_err);
        C2D_LAUNCH_CHECK(ctx);
        return (int)C2D_OK;
    });
}

}  // namespace c2d

using namespace c2d;

extern "C" {

int c2d_sat_poly_cross_mask(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, size_t row_base, size_t col_base, int flags,
                            unsigned long long* d_mask, size_t ld_words, unsigned long long* d_count, c2d_stream stream)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!a || !b) return fail_arg(ctx, "c2d_sat_poly_cross_mask: NULL set");
    if (a->n == 0 || b->n == 0) return C2D_OK;
    PolySetDev A, B;
    if (int rc = poly_cross_check(ctx, "c2d_sat_poly_cross_mask", a, b, row_base, col_base, flags, A, B)) return rc;
    if (int rc = cross_check_mask(ctx, "c2d_sat_poly_cross_mask", d_mask, ld_words, B.n)) return rc;
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = workspace_acquire(ctx, s, d_count != nullptr)) return rc;
    return cross_mask_launch(ctx, s, A, B, row_base, col_base, (flags & C2D_CROSS_UPPER) != 0, d_mask, ld_words, d_count);
}

int c2d_sat_poly_cross_pairs(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b, size_t row_base, size_t col_base, int flags,
                             uint32_t* d_pairs, size_t capacity, unsigned long long* d_count, c2d_stream stream)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!a || !b) return fail_arg(ctx, "c2d_sat_poly_cross_pairs: NULL set");
    if (a->n == 0 || b->n == 0) return C2D_OK;
    PolySetDev A, B;
    if (int rc = poly_cross_check(ctx, "c2d_sat_poly_cross_pairs", a, b, row_base, col_base, flags, A, B)) return rc;
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const bool upper = (flags & C2D_CROSS_UPPER) != 0;
    return cross_list_run(ctx, s, "c2d_sat_poly_cross_pairs", A.n, B.n, row_base, col_base, d_pairs, capacity, d_count,
                          [&](size_t r0, size_t rows, unsigned long long* d_mask, size_t words) {
                              PolySetDev Ar = A;   // rows [r0, r0 + rows): a pointer offset with the same stride
                              Ar.vx += r0;
                              Ar.vy += r0;
                              if (Ar.k) Ar.k += r0;
                              Ar.n = rows;
                              return cross_mask_launch(ctx, s, Ar, B, row_base + r0, col_base, upper, d_mask, words, d_count);
                          });
}

}  // extern "C"
