/*
 * c2d.h — C-ABI of the MI355X-native batched 2D SAT collision engine (libc2d.so).
 *
 * This is the drop-in boundary of the hot path.  The reference exposes no FFI
 * (SURVEY.md §8b): its boundary is the set of __device__/__global__ functions in
 * utils.cu plus the host loops in the three main()s.  Every entry point below
 * names the reference interface it replaces (file:line under /root/reference).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no C++/torch types;
 *   - return an int status (C2D_OK == 0, negative on error), never exit();
 *     the reference prints and exit()s (utils.cu:59-72);
 *   - buffers are caller-owned; pointers named d_* / "device" are HIP device
 *     pointers on the context's device, everything else is host memory;
 *   - work is enqueued on the caller's stream (a hipStream_t passed as void*,
 *     NULL = the default stream) and is asynchronous unless stated otherwise;
 *   - a c2d_ctx is bound to one device and owns a small device workspace (partial
 *     counts, adaptive-loop lists): use one ctx per device and per host thread.  Calls
 *     that use the workspace (c2d_mc_scenes; the SAT entry points when d_count != NULL)
 *     are ordered by their stream; issuing one on stream B while an earlier one on
 *     stream A has not finished returns C2D_ERR_UNSUPPORTED (use one ctx per stream).
 *     Streams stay the caller's: c2d keeps no stream handle beyond the call it was given to
 *     (the guard reads completion stamps that the kernels raise themselves, never the
 *     runtime's view of a remembered stream), so a stream may be destroyed by any means at
 *     any time after its calls were issued.  A NEW stream that the runtime creates at a
 *     destroyed stream's address is another stream to the guard, not the old one: it compares
 *     hipStreamGetId where the runtime has it (HIP >= 7.1).  On an older runtime — the HIP 7.0
 *     a PyTorch process holds — streams have no number: c2d_stream_destroy forgets the address
 *     of a stream it destroys with calls in flight, but a stream destroyed by OTHER means with
 *     c2d calls still in flight, whose address the runtime gives to a new stream that is used
 *     with the same ctx at once, passes for the old one there: drain such a stream first (or
 *     destroy it through c2d_stream_destroy).  While a stream is being captured into a
 *     graph the guard stands aside: the order of a graph's replays against other work on the
 *     same ctx is the caller's to arrange.  A launch that fails after it took its place in the
 *     guard's bookkeeping takes itself out again (the failing call drains its stream).
 *
 * Arithmetic contract (DESIGN.md §"Canonical arithmetic"): IEEE binary32,
 * round-to-nearest-even, no multiply-add contraction except where the spec
 * says fma; sin/cos/log are the c2d polynomial forms (bit-reproducible on any
 * IEEE machine), sqrt and divide are correctly rounded.  Booleans and hit
 * counts are therefore bit-exact against the CPU oracle in oracle/.
 *
 * Non-finite inputs.  The SAT entry points (c2d_sat_rect_pairs_*, c2d_sat_poly_pairs*,
 * c2d_rects_from_poses) are defined for EVERY bit pattern and follow the reference there
 * too: thrust::minmax_element (utils.cu:176-177) is comparison based, so on each axis a NaN
 * projection of a polygon's FIRST vertex stays that polygon's extreme — both comparisons
 * of utils.cu:178 are then false and the axis does not separate — while a NaN projection of
 * a later vertex is skipped; infinities are ordered like numbers.  Consequence: a pair with
 * a NaN in vertex 0 of either polygon reads "collide".  The Monte-Carlo entry points
 * (c2d_mc_pair, c2d_mc_scenes, c2d_sample_scenes) take table-driven scene parameters and
 * require them to be finite and below 1e15 in magnitude, and every length either zero or at
 * least 1e-15 (a product of two smaller lengths is denormal, and the shortcuts' margins are
 * relative rounding bounds); outside that domain a call still terminates and stays memory-safe,
 * and its hit counts follow the same rules (every certain-miss shortcut is switched off for
 * such a scene).
 */
#ifndef C2D_H_
#define C2D_H_

#include <stddef.h>
#include <stdint.h>

#include "utils.h"

#ifdef __cplusplus
extern "C" {
#endif

#define C2D_VERSION_MAJOR 0
#define C2D_VERSION_MINOR 6

/* ---- status codes ------------------------------------------------------ */
#define C2D_OK 0
#define C2D_ERR_INVALID_ARG (-1)  /* NULL pointer, bad size, bad vertex count ...        */
#define C2D_ERR_HIP (-2)          /* a HIP runtime call failed; see c2d_last_error()     */
#define C2D_ERR_NO_DEVICE (-3)    /* no usable gfx950 device / device index out of range */
#define C2D_ERR_NOMEM (-4)        /* device or host allocation failed                    */
#define C2D_ERR_UNSUPPORTED (-5)  /* argument combination outside the documented domain  */
#define C2D_ERR_DIST (-6)         /* RCCL / multi-GPU set-up or collective failed        */

typedef struct c2d_ctx c2d_ctx;
typedef void* c2d_stream; /* hipStream_t */

/* Fixed sampling schedule of the adaptive Monte-Carlo loop
 * (reference compute_collision_probability.cu:283-287, generate_dataset.cu:427-431):
 * batches of 1000 samples while n_samples < 20000, then batches of 100000. */
#define C2D_MC_SMALL_BATCH 1000
#define C2D_MC_LARGE_BATCH 100000
#define C2D_MC_SWITCH_AT 20000

typedef struct c2d_device_info {
    char name[128];
    char arch[64];
    int device;
    int compute_units;
    int wavefront_size;
    int lds_bytes_per_cu;
    size_t hbm_bytes;
    char pci_bus_id[32]; /* "0000:8b:00.0" (hipDeviceGetPCIBusId): which card of the node this ctx sits on */
} c2d_device_info;

/* ---- library / context --------------------------------------------------- */
int c2d_version(void); /* MAJOR*1000 + MINOR */
const char* c2d_status_string(int status);
/* Last error text of this ctx (HIP error string and call site); "" if none. */
const char* c2d_last_error(const c2d_ctx* ctx);
int c2d_device_count(int* count);
/* Replaces the implicit device-0 + default-stream set-up of the reference mains
 * (compute_collision_probability.cu:212-251). */
int c2d_ctx_create(int device, c2d_ctx** out);
int c2d_ctx_destroy(c2d_ctx* ctx);
/* c2d_device_info may grow at its end (0.5 added pci_bus_id), so it is filled through a call that is told how large the
 * CALLER's struct is: c2d_ctx_info_sized writes the first min(out_bytes, sizeof(c2d_device_info)) bytes of the current layout
 * and nothing beyond out_bytes.  Sources compiled against this header get it through the c2d_ctx_info macro below, with the
 * size of the struct they were compiled with.  The EXPORTED symbol c2d_ctx_info stays for binaries built against the 0.4
 * header, which declared the struct without pci_bus_id: it writes that layout only (C2D_DEVICE_INFO_BYTES_0_4 bytes: everything
 * up to and including hbm_bytes), never past the end of an old caller's struct. */
#define C2D_DEVICE_INFO_BYTES_0_4 (offsetof(c2d_device_info, hbm_bytes) + sizeof(size_t))
int c2d_ctx_info(const c2d_ctx* ctx, c2d_device_info* out);
int c2d_ctx_info_sized(const c2d_ctx* ctx, c2d_device_info* out, size_t out_bytes);
#define c2d_ctx_info(ctx, out) c2d_ctx_info_sized((ctx), (out), sizeof(c2d_device_info))
/* Argument errors that only the device can see (today: a polygon vertex count outside
 * 1..C2D_POLY_KMAX) are reported asynchronously: the kernel records them in a pinned word
 * of the ctx and the first c2d_stream_synchronize — or this call, for callers that
 * synchronise by other means — after the kernel finished returns C2D_ERR_INVALID_ARG once
 * (c2d_last_error() says what) and clears the record.  Returns C2D_OK if nothing is pending. */
int c2d_ctx_check_async(c2d_ctx* ctx);

/* ---- memory / stream plumbing ---------------------------------------------
 * Replace cudaMalloc / cudaMemcpy / cudaFree / cudaDeviceSynchronize in the
 * reference mains (compute_collision_probability.cu:212-248, :314-334, :367-377;
 * generate_dataset.cu:371-405, :461-482, :512-522).  Copies are asynchronous
 * on `stream`; call c2d_stream_synchronize before touching the host buffer. */
int c2d_malloc(c2d_ctx* ctx, void** d_ptr, size_t bytes);
int c2d_free(c2d_ctx* ctx, void* d_ptr);
/* Page-locked host memory: copies to / from it really are asynchronous (a copy that involves pageable
 * memory is staged by the runtime and may hold the calling thread until it is done), which is what lets a
 * driver overlap the host side of one batch with the GPU side of the next (csrc/host/driver_common.hpp). */
int c2d_malloc_host(c2d_ctx* ctx, void** h_ptr, size_t bytes);
int c2d_free_host(c2d_ctx* ctx, void* h_ptr);
int c2d_memset(c2d_ctx* ctx, void* d_ptr, int value, size_t bytes, c2d_stream stream);
int c2d_memcpy_h2d(c2d_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, c2d_stream stream);
int c2d_memcpy_d2h(c2d_ctx* ctx, void* h_dst, const void* d_src, size_t bytes, c2d_stream stream);
int c2d_stream_create(c2d_ctx* ctx, c2d_stream* out);
int c2d_stream_destroy(c2d_ctx* ctx, c2d_stream stream);
int c2d_stream_synchronize(c2d_ctx* ctx, c2d_stream stream);

/* ---- geometry ---------------------------------------------------------------
 *
 * c2d_rects_from_poses: batched create_rect (utils.cu:119-130) followed by
 * rot_trans_rectangle (utils.cu:132-142): rectangle i has size w[i] x h[i],
 * is rotated by theta[i] about its centre and translated to (cx[i], cy[i]).
 * Inputs are 5 device planes f32[n]; output is 8 device planes f32[n] in the
 * reference's flat order x0,y0,x1,y1,x2,y2,x3,y3. */
int c2d_rects_from_poses(c2d_ctx* ctx, const float* d_cx, const float* d_cy, const float* d_w,
                         const float* d_h, const float* d_theta, size_t n,
                         float* const d_out_planes[8], c2d_stream stream);

/* c2d_sat_rect_pairs_verts: batched rectangle-rectangle SAT — the arithmetic
 * of convex_collide (utils.cu:159-184) applied to n independent pairs: 8 axes
 * (the edge vectors of both rectangles, utils.cu:170-171), all 4+4 vertices
 * projected with an unfused dot product (utils.cu:172-175), separated iff
 * max1 < min2 || max2 < min1 (strict, utils.cu:178), no early result change.
 * The reference only calls convex_collide from inside its MC kernel
 * (compute_collision_probability.cu:138); this entry point is that function
 * over SoA arrays.
 *   d_planes[0..7]  : rectangle 1, planes x0,y0,x1,y1,x2,y2,x3,y3, each f32[n]
 *   d_planes[8..15] : rectangle 2, same order
 *   d_out           : u8[n], 1 = collide, 0 = separated
 *   d_count         : optional (may be NULL) device uint64 that is *incremented*
 *                     by the number of colliding pairs (atomically; zero it first).
 * Any alignment is accepted; planes and d_out aligned to 16 B / 4 B take the
 * wide-load path. */
int c2d_sat_rect_pairs_verts(c2d_ctx* ctx, const float* const d_planes[16], size_t n,
                             uint8_t* d_out, unsigned long long* d_count, c2d_stream stream);

/* c2d_sat_rect_pairs_verts_mask: the same test with a bit mask as output, for callers that only
 * need collide / no-collide: bit (i & 63) of d_mask[i >> 6] is the result of pair i (1 = collide);
 * d_mask is a device u64[(n + 63) / 64], 8-byte aligned; the unused high bits of the last word are 0.
 * 64.125 instead of 65 bytes of traffic per pair. */
int c2d_sat_rect_pairs_verts_mask(c2d_ctx* ctx, const float* const d_planes[16], size_t n,
                                  unsigned long long* d_mask, unsigned long long* d_count,
                                  c2d_stream stream);

/* c2d_sat_rect_pairs_aos: the same test on the reference's own argument layout,
 * convex_collide(float* r1, float* r2) (utils.cu:159) with flat float[8]
 * rectangles, batched: d_r1 and d_r2 are f32[n][8] (16-byte aligned), pair i is
 * (d_r1 + 8*i, d_r2 + 8*i).  Same 65 B/pair as the plane format. */
int c2d_sat_rect_pairs_aos(c2d_ctx* ctx, const float* d_r1, const float* d_r2, size_t n,
                           uint8_t* d_out, unsigned long long* d_count, c2d_stream stream);

/* c2d_sat_rect_pairs_pose: the same test on pose-format input: for each pair,
 * the result is that of building both rectangles exactly as c2d_rects_from_poses would
 * (utils.cu:119-142) and testing them (utils.cu:159-184) — for every bit pattern.  The kernel
 * reaches it from the closed-form gap of the two rectangles wherever that gap exceeds a proven
 * rounding margin, and by that very vertex arithmetic elsewhere.
 *   d_pose_planes[0..4] : rectangle 1: cx, cy, w, h, theta   (f32[n] each)
 *   d_pose_planes[5..9] : rectangle 2: cx, cy, w, h, theta */
int c2d_sat_rect_pairs_pose(c2d_ctx* ctx, const float* const d_pose_planes[10], size_t n,
                            uint8_t* d_out, unsigned long long* d_count, c2d_stream stream);

/* c2d_sat_rect_pairs_verts_host / _pose_host: the same tests for batches that live in HOST memory — what the
 * reference does around its kernel with one blocking cudaMemcpy after the other
 * (compute_collision_probability.cu:270-274 up, :314-318 down) — as ONE synchronous call: whole planes go up,
 * the test runs, the booleans and the count come back, in chunks of 2^24 pairs so that a batch of any size
 * needs at most 1 GB of device memory (kept by the ctx from the first call on).  It runs at the rate of the
 * host-to-device link, which carries 64 and 40 bytes per pair and is 95 % of the call (pipelined forms were
 * measured and are slower: csrc/c2d_host.hip).  h_planes / h_pose_planes: host planes as for the device entry
 * points, pageable or page-locked; h_out: host u8[n]; h_count: optional host word that receives the number of
 * colliding pairs.  Uses the ctx's count workspace like the device entry points.  Returns when h_out is complete. */
int c2d_sat_rect_pairs_verts_host(c2d_ctx* ctx, const float* const h_planes[16], size_t n, uint8_t* h_out,
                                  unsigned long long* h_count);
int c2d_sat_rect_pairs_pose_host(c2d_ctx* ctx, const float* const h_pose_planes[10], size_t n, uint8_t* h_out,
                                 unsigned long long* h_count);

/* ---- all pairs of two rectangle sets (N x M) ---------------------------------
 * Additions to 0.6 (c2d_version() stays 6): a caller can detect them by symbol lookup (dlsym).
 *
 * Which of the n_a rectangles of set A overlap which of the n_b rectangles of set B: result (i, j) is
 * convex_collide(A_i, B_j) (utils.cu:159-184), exactly the boolean c2d_sat_rect_pairs_verts gives for the pair with
 * A_i as rectangle 1 and B_j as rectangle 2 — for every input bit pattern, the non-finite rule above included.  The
 * test is symmetric in its two rectangles (the eight axes are both rectangles' edges, and every comparison is made both
 * ways), so A and B may be the same planes: with C2D_CROSS_UPPER that is the self-collision test of one set.
 *   d_a[0..7]  : set A, planes x0,y0,x1,y1,x2,y2,x3,y3, each f32[n_a]   (any alignment)
 *   d_b[0..7]  : set B, same order, f32[n_b]
 *   row_base, col_base : global indices of A_0 and B_0.  They change only the C2D_CROSS_UPPER predicate and the indices
 *                the pair list emits, so that a caller can shard A by rows (one GPU per shard) or tile B by
 *                columns and still get the right triangle; mask bit positions stay local to the call.
 *   flags      : 0, or C2D_CROSS_UPPER: only the pairs with (col_base + j) > (row_base + i) are tested; every other
 *                result is 0 and is not counted.
 *   d_count    : device uint64 *incremented* (atomically) by the number of colliding tested pairs.
 *
 * c2d_sat_rect_cross_mask: bit (j & 63) of d_mask[i * ld_words + (j >> 6)] is result (i, j) (the bit order of
 * c2d_sat_rect_pairs_verts_mask).  ld_words >= ceil(n_b / 64); d_mask 8-byte aligned.  Every bit of each row's first
 * ceil(n_b / 64) words is written (bits j >= n_b as 0); words beyond them, up to ld_words, are not touched.  d_count is
 * optional (may be NULL).  Asynchronous on `stream` and graph-capturable.
 *
 * c2d_sat_rect_cross_pairs: the colliding tested pairs as a list, d_pairs = u32[capacity][2] holding
 * (row_base + i, col_base + j) in row-major order (by i, then by j) — the order of np.argwhere on the mask.  Only the
 * first `capacity` pairs are written, nothing beyond; d_count is required and receives the TOTAL, those beyond the
 * capacity included: a caller that finds total > capacity calls again with a larger buffer (d_pairs may be NULL when
 * capacity is 0: a count-only call).  Global indices are u32: a call with row_base + n_a or col_base + n_b above 2^32 is
 * refused (C2D_ERR_INVALID_ARG).  Asynchronous on `stream`, with no host synchronisation; the order of the output is
 * deterministic.  It works through the ctx scratch (mask rows of up to 256 MiB per pass), which it grows on first use
 * and keeps: that allocation cannot happen while the stream is being captured into a graph, so a capture of this call
 * is refused (C2D_ERR_INVALID_ARG) unless an earlier call of the same or a larger size already grew the scratch. */
#define C2D_CROSS_UPPER 1   /* test only pairs with (col_base + j) > (row_base + i) */

int c2d_sat_rect_cross_mask(c2d_ctx* ctx,
                            const float* const d_a[8], size_t n_a,     /* set A: x0,y0,...,x3,y3 planes, f32[n_a] */
                            const float* const d_b[8], size_t n_b,     /* set B: same order, f32[n_b] */
                            size_t row_base, size_t col_base, int flags,
                            unsigned long long* d_mask, size_t ld_words,
                            unsigned long long* d_count, c2d_stream stream);

int c2d_sat_rect_cross_pairs(c2d_ctx* ctx,
                             const float* const d_a[8], size_t n_a,
                             const float* const d_b[8], size_t n_b,
                             size_t row_base, size_t col_base, int flags,
                             uint32_t* d_pairs, size_t capacity,        /* u32[capacity][2] */
                             unsigned long long* d_count, c2d_stream stream);

/* ---- broad-phase pair search of two rectangle sets ---------------------------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the two above.
 *
 * c2d_sat_rect_broad_pairs: the list of c2d_sat_rect_cross_pairs with row_base = col_base = 0, bit for bit and with the
 * same count, for every input (non-rectangular quads, degenerate shapes, NaN / inf and huge coordinates included), but
 * found through a broad phase: each rectangle gets a conservative box, B's boxes are sorted into a uniform grid, and the
 * exact test (rect_collide, utils.cu:159-184) runs only on the pairs whose boxes overlap.  Objects the box argument does not
 * cover ("wild": non-finite or |coordinate| >= 2^60, degenerate, or a box far wider than the scene's typical one) are tested
 * against everything.  DESIGN.md §5.8 proves that no pair is lost.  Use it for sparse scenes: its cost is about
 * O((n_a + n_b) log n_b + candidates) where the cross form's is n_a x n_b tests; dense scenes, small sets and scenes with
 * many wild objects are the cross form's.
 *   d_a, d_b, flags : as c2d_sat_rect_cross_pairs (C2D_CROSS_UPPER: only j > i).  B may be the same planes as A: then the
 *                boxes are made and sorted once.
 *   d_pairs, capacity, d_count : as c2d_sat_rect_cross_pairs: (i, j) in row-major order, only the first `capacity` written,
 *                d_count (required) incremented by the TOTAL; d_pairs may be NULL when capacity is 0 (a count-only call,
 *                which skips the emit pass).
 * A call with n_a or n_b above 2^32 is refused (C2D_ERR_INVALID_ARG).  Asynchronous on `stream`, with no host
 * synchronisation; the output is deterministic.  It works through the ctx scratch, which it grows on first use and keeps:
 * 36 bytes per object of A plus 48.5 per object of B (68.5 per object when B is A: the boxes are shared) and a 4 KiB header.
 * Graph capture follows the cross list: a capture is refused (C2D_ERR_INVALID_ARG) unless an earlier call of the same or a
 * larger size already grew the scratch. */
int c2d_sat_rect_broad_pairs(c2d_ctx* ctx,
                             const float* const d_a[8], size_t n_a,     /* set A: x0,y0,...,x3,y3 planes, f32[n_a] */
                             const float* const d_b[8], size_t n_b,     /* set B: same order; may be the same planes as d_a */
                             int flags,                                 /* 0 or C2D_CROSS_UPPER (j > i only) */
                             uint32_t* d_pairs, size_t capacity,        /* u32[capacity][2] */
                             unsigned long long* d_count, c2d_stream stream);

/* c2d_sat_poly_pairs: SAT for arbitrary convex polygons with up to
 * C2D_POLY_KMAX vertices.  Same projection / strict-< interval test as
 * utils.cu:172-180, but the axis of edge e is its true normal (-e.y, e.x):
 * the reference's edge-as-axis shortcut (utils.cu:170-171) is only valid for
 * rectangles.
 *   d_vx, d_vy : f32[2][C2D_POLY_KMAX][n]   (polygon, vertex, pair) — pair index fastest
 *   d_k        : u8[2][n]                    vertex counts, 1..C2D_POLY_KMAX
 *   d_out      : u8[n]
 * Padded vertex slots (index >= count) are never interpreted.  The call is asynchronous
 * and graph-capturable; vertex counts are checked on the device: a pair with a count
 * outside 1..C2D_POLY_KMAX gets result 0 and the error is reported by the next
 * c2d_stream_synchronize / c2d_ctx_check_async (see there). */
int c2d_sat_poly_pairs(c2d_ctx* ctx, const float* d_vx, const float* d_vy, const uint8_t* d_k,
                       size_t n, uint8_t* d_out, unsigned long long* d_count, c2d_stream stream);

/* c2d_sat_poly_pairs_rows: the same test on a layout with `rows` vertex rows per polygon instead of
 * C2D_POLY_KMAX — d_vx, d_vy : f32[2][rows][n], vertex counts 1..rows, 1 <= rows <= C2D_POLY_KMAX.
 * Batches of small polygons (triangles and quadrilaterals: rows = 4; up to octagons: rows = 8) take
 * a quarter or half of the memory and run a kernel instance sized for them (fewer registers, more
 * waves per SIMD, four or eight pairs per wave in the full evaluation); layouts of 9 .. 15 rows run as
 * one bin of the binned kernel below (its 12- and 16-row instances).  rows = C2D_POLY_KMAX is
 * c2d_sat_poly_pairs.  A batch whose pairs are ordered by vertex counts moves only the rows its waves
 * need (16-row instance: a wave skips every row above its largest count). */
int c2d_sat_poly_pairs_rows(c2d_ctx* ctx, const float* d_vx, const float* d_vy, const uint8_t* d_k,
                            size_t n, int rows, uint8_t* d_out, unsigned long long* d_count,
                            c2d_stream stream);

/* ---- all pairs of two convex polygon sets (N x M) ------------------------------
 * Additions to 0.6 (c2d_version() stays 6): a caller can detect them by symbol lookup (dlsym).
 *
 * Which of the n polygons of set A overlap which of those of set B: result (i, j) is exactly the boolean
 * c2d_sat_poly_pairs_rows gives for the pair with A_i as polygon 1 and B_j as polygon 2 — the projection and strict-<
 * interval test of utils.cu:172-180 on the true normals (-e.y, e.x) of all ka + kb edges, for every input bit pattern,
 * the non-finite rule above included; padded vertex slots are never interpreted.  Only a polygon's own edge normals are
 * axes, so degenerate polygons read as c2d_sat_poly_pairs reads them (two far-apart points "collide": a point's only axis is
 * the zero vector).  The test is symmetric in its two polygons, so a and b may describe the same memory: with
 * C2D_CROSS_UPPER that is the self-collision test of one set.  The two sets may have different `rows`.
 *
 * c2d_poly_set is one half of the padded pair layout of c2d_sat_poly_pairs_rows.  `stride` lets a caller shard A by rows or
 * tile B by columns with a pointer offset (d_vx + r0, d_vy + r0, d_k + r0, n = r1 - r0, the same stride), and makes the two
 * halves of a padded pair batch f32[2][rows][n] two sets without a copy.  A vertex count outside 1..rows gives result 0 for
 * every pair the polygon is in (those pairs are not counted), and the error is reported by the next
 * c2d_stream_synchronize / c2d_ctx_check_async, as for c2d_sat_poly_pairs.
 *
 * Everything else is c2d_sat_rect_cross_mask / c2d_sat_rect_cross_pairs word for word: row_base / col_base change only the
 * C2D_CROSS_UPPER predicate ((col_base + j) > (row_base + i)) and the indices the list emits; bit (j & 63) of
 * d_mask[i * ld_words + (j >> 6)] is result (i, j), ld_words >= ceil(n_b / 64), d_mask 8-byte aligned, every bit of each
 * row's first ceil(n_b / 64) words written (bits j >= n_b as 0), words beyond untouched; d_count is *incremented*
 * atomically (optional for the mask, required for the list).  The list is u32[capacity][2] of (row_base + i, col_base + j)
 * in row-major order (np.argwhere of the mask), only the first `capacity` pairs written, the TOTAL in d_count, d_pairs may
 * be NULL when capacity is 0; a call with row_base + n_a or col_base + n_b above 2^32 is refused.  n_a == 0 or n_b == 0 is
 * a no-op.  Both forms are asynchronous on `stream` with no host synchronisation and deterministic.  The mask form is
 * graph-capturable; the list form works through the ctx scratch like the rectangle list (a capture that would have to grow
 * the scratch is refused, C2D_ERR_INVALID_ARG). */
typedef struct c2d_poly_set {
    uint32_t rows;          /* vertex rows in memory, 1..C2D_POLY_KMAX */
    size_t n;               /* polygons */
    size_t stride;          /* elements between consecutive vertex rows, >= n; 0 = n */
    const float* d_vx;      /* f32[rows][stride], polygon index fastest; any 4-byte alignment */
    const float* d_vy;
    const uint8_t* d_k;     /* u8[n] vertex counts 1..rows, or NULL = every polygon has exactly `rows` vertices */
} c2d_poly_set;             /* a host struct, read before the call returns */

int c2d_sat_poly_cross_mask(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                            size_t row_base, size_t col_base, int flags,
                            unsigned long long* d_mask, size_t ld_words,
                            unsigned long long* d_count, c2d_stream stream);

int c2d_sat_poly_cross_pairs(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                             size_t row_base, size_t col_base, int flags,
                             uint32_t* d_pairs, size_t capacity,        /* u32[capacity][2] */
                             unsigned long long* d_count, c2d_stream stream);

/* ---- broad-phase pair search of two convex polygon sets -------------------------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the ones above.
 *
 * c2d_sat_poly_broad_pairs: the list and the total of c2d_sat_poly_cross_pairs(a, b, 0, 0, flags, ...) — the same pairs in the
 * same row-major order with the same count, for every input bit pattern: degenerate polygons (points and far-apart collinear
 * segments "collide", as above), NaN / inf and huge or subnormal coordinates, clockwise polygons and repeated vertices, sets
 * with different `rows`, any `stride`, d_k == NULL — but found through the broad phase of c2d_sat_rect_broad_pairs (the same
 * grid, sort, scan, count and emit pipeline).  A polygon's conservative box is the box of a parallelogram whose edge normals
 * are two of the polygon's own test axes, each interval widened by the test's rounding bound; polygons the argument does not
 * cover ("wild": a non-finite real vertex or a |coordinate| >= 2^60, fewer than three vertices, no two usable non-parallel
 * edges, or a box far wider than the scene's typical one) are tested against everything.  DESIGN.md §5.10 proves that no pair
 * is lost.  Use it for sparse scenes of many polygons; dense scenes, small sets and scenes with many wild polygons are the
 * cross form's.
 *   a, b       : as c2d_sat_poly_cross_pairs.  Padded vertex slots (index >= the polygon's count) are never interpreted.  A
 *                polygon with a vertex count outside 1..rows is in no pair and is not counted; the error is reported by the
 *                next c2d_stream_synchronize / c2d_ctx_check_async, exactly as for the cross form.  a and b may describe the
 *                same memory (same pointers, n, stride, rows, d_k): the boxes and the sort are then made once, and with
 *                C2D_CROSS_UPPER that is the self-collision test of one set.
 *   flags      : 0, or C2D_CROSS_UPPER: only the pairs with j > i.
 *   d_pairs, capacity, d_count : u32[capacity][2] of (i, j) in row-major order, only the first `capacity` pairs written;
 *                d_count (required) is incremented by the TOTAL; d_pairs may be NULL when capacity is 0 (a count-only call,
 *                which skips the emit pass).
 * n_a == 0 or n_b == 0 is a no-op.  A call with n_a or n_b above 2^32 is refused; an unknown flag, a NULL argument or `rows`
 * outside 1..C2D_POLY_KMAX is refused (C2D_ERR_INVALID_ARG) before a device is touched.  Asynchronous on `stream`, with no host
 * synchronisation; the output is deterministic.  It works through the ctx scratch under the workspace guard, which it grows
 * on first use and keeps; the size depends only on (n_a, n_b, same memory): 36 bytes per polygon of A plus 48.5 per polygon
 * of B (68.5 per polygon when B is A: the boxes are shared) and a 4 KiB header.  Graph capture follows the rectangle broad
 * phase: allowed after an eager call of the same or a larger size, refused (C2D_ERR_INVALID_ARG) before anything is enqueued
 * if the scratch would have to grow. */
int c2d_sat_poly_broad_pairs(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                             int flags,                                 /* 0 or C2D_CROSS_UPPER (j > i only) */
                             uint32_t* d_pairs, size_t capacity,        /* u32[capacity][2] */
                             unsigned long long* d_count, c2d_stream stream);

/* ---- contact queries: depth and normal for listed pairs -------------------------
 * Additions to 0.6 (c2d_version() stays 6), found by symbol lookup like the ones above.
 *
 * c2d_poly_pair_contacts / c2d_rect_pair_contacts: for each pair of a list — the list a cross or broad call emitted, or any
 * other — the minimum-translation contact over the pairwise test's OWN axes: a signed depth, a unit normal from A towards B,
 * the axis the contact came from, and the boolean of the pairwise test for that pair.  The list and its length stay on the
 * device, so broad phase -> pair list -> contacts runs on one stream with no host synchronisation.
 *
 * Arithmetic contract.  Everything is IEEE binary32, round to nearest, subnormals kept, nothing contracted;
 * division and square root are correctly rounded.
 *   axes     polygons: axis e is the true normal (-(y[e+1] - y[e]), x[e+1] - x[e]) of edge e, A's ka edges first (0..ka-1), then
 *            B's kb (ka..ka+kb-1), the vertex index wrapping at k; projections are nx * x + ny * y, unfused, as in
 *            c2d_sat_poly_pairs.  Rectangles: the eight edge-vector axes of convex_collide (utils.cu:170-171; 0..3 rectangle A,
 *            4..7 rectangle B), projected exactly as c2d_sat_rect_pairs_verts of the same build projects them.
 *   per axis with [minA, maxA], [minB, maxB] the two projection intervals (running fmin / fmax from +inf / -inf):
 *            o1 = maxA - minB,  o2 = maxB - minA,  o = o1 <= o2 ? o1 : o2,  len2 = nx * nx + ny * ny (unfused).
 *            The axis is unusable when len2 == 0 or when o / sqrt(len2) is NaN; otherwise d = o / sqrt(len2).
 *   result   the axis with the smallest d wins under strict <, taken in axis order (the first of equal axes wins; the first usable
 *            axis wins over nothing, whatever its d): depth = d, (nx, ny) = (+-nx / len, +-ny / len) with len = sqrt(len2) and
 *            + when o1 <= o2 — B then lies on the axis's positive side, and moving B by depth along the normal separates the
 *            pair.  With no usable axis: depth = +inf, normal (0, 0), axis = 0xFFFF, flags = C2D_CONTACT_NO_AXIS.
 *   hit      is not derived from depth: it is the pairwise boolean itself (c2d_sat_poly_pairs_rows / c2d_sat_rect_pairs_verts on
 *            the pair), for every input bit pattern, the non-finite rule above included.  For finite inputs with no overflow,
 *            hit == (depth >= 0) on every pair that has a usable axis.
 * The implementation evaluates axes in another order and in parallel; its results equal this sequential rule.  +0 and -0 compare
 * equal in depth, nx and ny.  A depth < 0 says "separated", and -depth is a lower bound of the distance.
 *
 *   a, b / d_a, n_a, d_b, n_b : the two sets, as for the cross forms (polygon sets may differ in `rows`; a and b may be the same
 *                memory).
 *   d_pairs    : u32[n_pairs][2], exactly what the cross and broad lists emit: entry p is (row_base + i, col_base + j).
 *   d_n_pairs  : optional device uint64 — the d_count a list call filled.  When given, only the first min(n_pairs, *d_n_pairs)
 *                entries are processed (the count is read on the device), so a caller passes n_pairs = the list's capacity and
 *                the count straight from the list call.  d_out[p] for p at or beyond that bound is not touched.
 *   row_base, col_base : the global indices of A_0 and B_0, as for the cross forms.
 *   d_out      : c2d_contact[n_pairs], 16-byte aligned; entry p is the contact of list entry p.
 * A pair whose index falls outside [base, base + n) reads no vertex memory and gets hit = 0, flags = C2D_CONTACT_BAD_PAIR,
 * depth = 0, normal (0, 0), axis = 0xFFFF; so does a pair with a polygon whose vertex count is outside 1..rows ("in no pair").
 * Either is reported by the next c2d_stream_synchronize / c2d_ctx_check_async, as a bad vertex count is elsewhere.  n_pairs == 0
 * is a no-op.  NULL arguments, `rows` out of range, a misaligned d_out and the like are refused (C2D_ERR_INVALID_ARG) before a
 * device is touched.  The calls use no ctx scratch; they are asynchronous on `stream` and graph-capturable. */
#define C2D_CONTACT_NO_AXIS 1   /* no usable axis: depth = +inf, normal (0, 0), axis = 0xFFFF */
#define C2D_CONTACT_BAD_PAIR 2  /* an index outside its set, or a polygon with a bad vertex count: nothing was computed */

typedef struct c2d_contact {      /* 16 bytes, 16-byte aligned output */
    float    depth;               /* min over usable axes of overlap / |axis|; < 0: separated, -depth is a lower bound of the distance */
    float    nx, ny;              /* unit axis, oriented from A towards B; (0, 0) when no axis is usable */
    uint16_t axis;                /* 0..ka-1: edge of A, ka..ka+kb-1: edge of B (rectangles: 0..3, 4..7); 0xFFFF: none */
    uint8_t  hit;                 /* the boolean of the pairwise test for this pair, for every input bit pattern */
    uint8_t  flags;               /* C2D_CONTACT_NO_AXIS, C2D_CONTACT_BAD_PAIR */
} c2d_contact;

int c2d_poly_pair_contacts(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                           const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                           size_t row_base, size_t col_base,
                           c2d_contact* d_out, c2d_stream stream);

int c2d_rect_pair_contacts(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b,
                           const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                           size_t row_base, size_t col_base,
                           c2d_contact* d_out, c2d_stream stream);

/* ---- contact manifolds: up to two contact points per listed pair ------------------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup.
 *
 * c2d_poly_pair_manifolds: c2d_poly_pair_contacts and, fused into the same device call, WHERE the two polygons touch: the edge of
 * the other polygon that faces the contact's own edge, clipped to that edge's extent — one or two points, each with its own signed
 * penetration.  The sets, the list, d_n_pairs, the bases, the records at or beyond the bound (untouched, in BOTH outputs), bad
 * pairs, the asynchronous error word, the refused arguments, "no ctx scratch" and graph capture are those of
 * c2d_poly_pair_contacts.  Both outputs are required, and both are 16-byte aligned.
 *   d_contacts[p]  : bit for bit what c2d_poly_pair_contacts writes for the same arguments.
 *   d_manifolds[p] : the manifold of list entry p.  A contact with C2D_CONTACT_BAD_PAIR or C2D_CONTACT_NO_AXIS has the empty
 *                    manifold: all coordinates and depths 0, feature = 0xFFFF, count = 0, flags = 0.
 * Polygons only.  c2d_rect_pair_contacts uses the edge VECTORS of convex_collide as axes, and an edge vector is not the normal of
 * any edge of a general quad, so "reference edge" has no meaning there: pass rectangles as 4-gons of a set with rows = 4.
 *
 * Arithmetic contract.  Everything is IEEE binary32, round to nearest, subnormals kept, nothing contracted;
 * division is correctly rounded.  The contact rule above supplies the winning axis e, its raw (nx, ny), pos = (o1 <= o2) and
 * len = sqrt(len2).
 *   1. R = A when e < ka, else B (the REFERENCE polygon; its edge r = e or e - ka is the reference edge); I is the other polygon
 *      (the INCIDENT one), with kI vertices.  sigma = +1 when (R is A) == pos, else -1.  F = sigma > 0 ? maxR : minR, with
 *      [minR, maxR] the contact rule's own interval of R on this axis.
 *   2. p_f = nx * x_f + ny * y_f for the vertices f < kI of I.  The deepest vertex w starts at f = 0; a later f replaces it only
 *      under strict p_f < p_w (sigma > 0) or p_f > p_w (sigma < 0): compare and select, not fmin — the first of equals wins and a
 *      NaN never replaces.
 *   3. nxt = (w + 1) mod kI, prv = (w - 1 + kI) mod kI.  The other end of the incident edge is u = nxt, unless p_prv is strictly
 *      deeper than p_nxt in the sense of step 2; then u = prv.  feature = (u == nxt) ? w : prv — the incident edge in I's own
 *      numbering.  kI == 1: count = 1, point 0 is w, feature = 0, and steps 4 and 5 do not apply (no clip bit, no OUTSIDE_SLAB).
 *   4. tau(x, y) = ny * x - nx * y (two products, one subtraction).  tau0, tau1 are tau at R's vertices r and (r + 1) mod kR;
 *      lo = tau0 <= tau1 ? tau0 : tau1, hi the other.
 *   5. Each end g of the incident edge is clipped against the ORIGINAL other end h: bound = lo if tau_g < lo, hi if tau_g > hi,
 *      otherwise the end stays.  A clipped end becomes x = x_g + (x_h - x_g) * s, y = y_g + (y_h - y_g) * s with
 *      s = (bound - tau_g) / (tau_h - tau_g), and its CLIPPED bit is set.  If both ends are below lo or both above hi:
 *      count = 1, point 0 is w unclipped, OUTSIDE_SLAB is set.  Otherwise count = 2: point 0 from w, point 1 from u.
 *   6. Each kept point: p = nx * x + ny * y from its final coordinates, d = (sigma > 0 ? F - p : p - F) / len.
 * Both points are always reported, each with its own sign: a corner contact has d1 < 0 and the caller filters (a speculative
 * solver wants exactly that).  Point 0 unclipped has d0 == depth of the contact.  Non-finite coordinates give whatever this
 * arithmetic gives; +0 and -0 compare equal. */
#define C2D_MANIFOLD_REF_IS_B      1  /* the reference edge belongs to B (axis >= ka) */
#define C2D_MANIFOLD_P0_CLIPPED    2  /* point 0 was moved onto a side plane of the reference edge */
#define C2D_MANIFOLD_P1_CLIPPED    4
#define C2D_MANIFOLD_OUTSIDE_SLAB  8  /* the incident edge misses the reference edge's slab: count = 1, the deepest vertex unclipped */

typedef struct c2d_manifold {   /* 32 bytes, 16-byte aligned output */
    float    x0, y0, d0;        /* point 0 (starts at the deepest vertex of the incident polygon) and its signed depth */
    float    x1, y1, d1;        /* point 1 (starts at the other end of the incident edge); 0, 0, 0 when count < 2 */
    uint16_t feature;           /* incident edge, in the incident polygon's own numbering 0..k-1; 0xFFFF: none */
    uint8_t  count;             /* 0, 1 or 2 */
    uint8_t  flags;
    uint32_t reserved;          /* written as 0 */
} c2d_manifold;

int c2d_poly_pair_manifolds(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                            const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                            size_t row_base, size_t col_base,
                            c2d_contact* d_contacts, c2d_manifold* d_manifolds, c2d_stream stream);

/* ---- distance queries: separation and closest points for listed pairs -------------
 * Additions to 0.6 (c2d_version() stays 6), found by symbol lookup like the contact calls.
 *
 * c2d_poly_pair_distances / c2d_rect_pair_distances: for each pair of a list the boolean of the pairwise test and, when the pair is
 * not hit, how far apart the two shapes are and which two points realise that distance.  (A contact's -depth is only a lower bound
 * of it: when the closest features are two vertices, no axis of the pairwise test gives the distance.)  The sets, d_pairs,
 * d_n_pairs, the bases, the records at or beyond min(n_pairs, *d_n_pairs) (untouched), bad pairs, the asynchronous error word,
 * n_pairs == 0 (a no-op), the refused arguments (NULL, a misaligned output, n_pairs >= 2^62, ...; refused before a device is
 * touched), "no ctx scratch", the single launch and graph capture are those of c2d_poly_pair_contacts / c2d_rect_pair_contacts.
 *   d_out : c2d_distance[n_pairs], 16-byte aligned; entry p is the distance record of list entry p.
 *
 * Arithmetic contract.  Everything is IEEE binary32, round to nearest, subnormals kept, nothing contracted in any
 * build; division and square root are correctly rounded.
 *   hit         the pairwise boolean itself (c2d_sat_poly_pairs_rows / c2d_sat_rect_pairs_verts of the same build on the pair), for
 *               every input bit pattern: exactly the `hit` of the contact calls.  When hit: dist = 0, both points (0, 0),
 *               edge = vert = 0xFFFF, flags = 0 (how deep is the contact calls' business).
 *   candidates  when not hit, the result is the minimum over candidates (edge, vertex).  Side 0: edge e of A (e = 0..ka-1, from
 *               vertex e to vertex (e + 1) mod ka) against vertex v of B (v = 0..kb-1).  Side 1: edge e of B against vertex v of A.
 *               Rectangles are the four vertices of their planes, k = 4.
 *   per candidate, the edge running (x0, y0) -> (x1, y1) and the vertex being (xp, yp):
 *               ex = x1 - x0, ey = y1 - y0, qx = xp - x0, qy = yp - y0, len2 = ex * ex + ey * ey, s = qx * ex + qy * ey.
 *               Region 0: if s <= 0 the closest point (cx, cy) is (x0, y0) itself.  Region 1: else if s >= len2 it is (x1, y1)
 *               itself.  Region 2: else t = s / len2, cx = x0 + t * ex, cy = y0 + t * ey (product, then sum).
 *               dx = xp - cx, dy = yp - cy, d2 = dx * dx + dy * dy.  A NaN s fails both compares and reaches region 2, so d2 is
 *               NaN.  A candidate is unusable when d2 is NaN; a d2 of +inf is usable.  A zero-length edge always lands in region 0
 *               or 1, so nothing divides by zero.
 *   the pick    candidates are taken in the order side, then e, then v.  The first usable one is the first best; a later one
 *               replaces it only under strict d2 < best (compare and select, not fmin).  Equivalently: the smallest d2 wins, and
 *               among equal d2 the smallest side * 256 + e * 16 + v.  Exact ties are the rule, not the exception: every
 *               vertex-to-vertex minimum is reached by up to four candidates with the same bits.
 *   the record  dist = sqrt(best), edge = e, vert = v.  On side 0 the closest point goes to (ax, ay) and the vertex to (bx, by); on
 *               side 1 it is the other way round and C2D_DISTANCE_EDGE_ON_B is set.  C2D_DISTANCE_INTERIOR is set in region 2.
 *               No usable candidate: dist = +inf, points (0, 0), edge = vert = 0xFFFF, C2D_DISTANCE_NO_CANDIDATE.  A bad pair (as
 *               for the contact calls): everything 0, edge = vert = 0xFFFF, C2D_DISTANCE_BAD_PAIR.
 * The implementation may evaluate candidates in another order; its results equal this sequential rule.  +0 and -0 compare equal
 * in the five floats.  For disjoint convex polygons this minimum is the Euclidean distance of the two polygons, and the two points
 * are a closest pair.  For non-convex input nothing is promised about what the numbers mean, only their bits. */
#define C2D_DISTANCE_EDGE_ON_B    1  /* the winning edge belongs to B and the vertex to A (side 1) */
#define C2D_DISTANCE_INTERIOR     2  /* the closest point lies strictly inside the edge (region 2) */
#define C2D_DISTANCE_NO_CANDIDATE 4  /* not hit, and no usable candidate: dist = +inf */
#define C2D_DISTANCE_BAD_PAIR     8  /* as C2D_CONTACT_BAD_PAIR */

typedef struct c2d_distance {   /* 32 bytes, 16-byte aligned output */
    float    dist;              /*  0: Euclidean distance; 0 when hit */
    float    ax, ay;            /*  4: the closest point on A */
    float    bx, by;            /* 12: the closest point on B */
    uint16_t edge;              /* 20: index of the winning edge in its own polygon (0..k-1); 0xFFFF: none */
    uint16_t vert;              /* 22: index of the winning vertex in the other polygon; 0xFFFF: none */
    uint8_t  hit;               /* 24: the pairwise boolean, for every input bit pattern */
    uint8_t  flags;             /* 25 */
    uint16_t reserved0;         /* 26: written as 0 */
    uint32_t reserved1;         /* 28: written as 0 */
} c2d_distance;

int c2d_poly_pair_distances(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                            const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                            size_t row_base, size_t col_base,
                            c2d_distance* d_out, c2d_stream stream);

int c2d_rect_pair_distances(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b,
                            const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                            size_t row_base, size_t col_base,
                            c2d_distance* d_out, c2d_stream stream);

/* ---- overlap queries: area, centroid and IoU of the intersection for listed pairs ----
 * Additions to 0.6 (c2d_version() stays 6), found by symbol lookup like the contact calls.
 *
 * c2d_poly_pair_overlaps / c2d_rect_pair_overlaps: for each pair of a list the boolean of the pairwise test and, when the pair is
 * hit, HOW MUCH of the two shapes overlaps: the area of A ∩ B, its centroid, the two shapes' own areas and the intersection over
 * union (rotated-box and convex-polygon IoU; area-weighted penalty forces and buoyancy; "inside" told from "crossing" by the piece
 * counts).  The sets, d_pairs, d_n_pairs, the bases, the records at or beyond min(n_pairs, *d_n_pairs) (untouched), bad pairs, the
 * asynchronous error word, n_pairs == 0 (a no-op), the refused arguments (refused before a device is touched), "no ctx scratch", the
 * single launch and graph capture are those of c2d_poly_pair_contacts / c2d_rect_pair_contacts.
 *   d_out : c2d_overlap[n_pairs], 16-byte aligned; entry p is the overlap record of list entry p.
 *
 * Arithmetic contract.  Everything is IEEE binary32, round to nearest, subnormals kept, nothing contracted in any
 * build; division is correctly rounded; cross(u, v) = u.x * v.y - u.y * v.x (two products, one difference); max and min below are
 * compare and select (t0 = q > t0 ? q : t0), so a NaN operand moves nothing.  Vertex order may be clockwise or counter-clockwise,
 * 1 <= k <= 16; rectangles are the four vertices of their planes, ka = kb = 4.
 *   hit         the pairwise boolean itself, for every input bit pattern: exactly the `hit` of the contact calls.
 *   setup       r = A's vertex 0.  Every vertex v of both shapes is replaced by v - r (one rounding per coordinate); everything below
 *               uses the shifted vertices.  sum_A = the shoelace sum  cross(v_0, v_1) + cross(v_1, v_2) + ... + cross(v_ka-1, v_0),
 *               accumulated from 0 in that order; sA = +1 if sum_A > 0, else -1; area_a = 0.5 * |sum_A|; likewise sum_B, sB, area_b.
 *               hit == 0: the record is {area 0, iou 0, centroid (0, 0), area_a, area_b, hit 0, C2D_OVERLAP_NO_CENTROID, pieces 0, 0}.
 *               Else, if sum_A or sum_B is 0 or NaN (a point, a segment, collinear vertices): area = iou = 0, centroid (0, 0),
 *               flags = C2D_OVERLAP_DEGENERATE | C2D_OVERLAP_NO_CENTROID, pieces 0, 0.
 *   setup (2)   D = the largest |coordinate| of the shifted real vertices of both shapes (compare and select from 0, so a NaN moves
 *               nothing), kD = 2^-21 * D (8 u D, u = 2^-24).
 *   the sides   side 0 walks A's edges e = 0..ka-1 as P (from vertex e to vertex (e + 1) mod ka) and clips each against all edges
 *               of B as Q; side 1 walks B's edges against A.  For P's edge p0 -> p1: ex = p1 - p0, t0 = 0, t1 = 1, and the piece's
 *               ends start as a = p0, b = p1.  For Q's edges f = 0..kq-1 in order, q0 -> q1 with g = q1 - q0: a zero-length g
 *               imposes nothing.  Otherwise four cross products,
 *                   c_p0 = cross(g, p0 - q0), c_p1 = cross(g, p1 - q0), c_q0 = cross(ex, q0 - p0), c_q1 = cross(ex, q1 - p0),
 *               and the pair of edges lies ON ONE LINE when |c_p0| <= T_g, |c_p1| <= T_g, |c_q0| <= T_e and |c_q1| <= T_e with
 *               T_x = kD * (|x.x| + |x.y|).  The two sides evaluate the same four expressions on the same operands for a pair of
 *               edges (c_p of one side is c_q of the other), so this decision, and every one below that is taken from da and db,
 *               has the same bits on both sides.  same_way = sP * sQ * (ex.x * g.x + ex.y * g.y) > 0.
 *               Not on one line:  num = sQ * c_p0, den = sQ * cross(g, ex), q = (-num) / den, and
 *                   den > 0 and q > t0:   t0 = q, a = X
 *                   den < 0 and q < t1:   t1 = q, b = X
 *                   den == 0:  (parallel) the edge survives this half-plane if num > 0, and, on side 0 only, if num == 0 and
 *                              same_way; otherwise it is dropped.
 *                   (a NaN den does none of the three.)
 *               X is the crossing of the two edges, ONE point for both sides: the point on A's edge.  On side 0
 *               X = p0 + q * ex (product, then sum).  On side 1, where A's edge is Q's, X = q0 + tq * g with
 *               tq = (-(sP * c_q0)) / (sP * cross(ex, g)): the operations of side 0 for this pair of edges, on the same operands.
 *               The pieces of the two sides then meet in the same bits, and the boundary closes, however badly the two quotients
 *               are conditioned.
 *               On one line and not same_way: the edge is dropped (the shapes only touch along it).
 *               On one line and same_way: with da, db the ends of A's edge against B's half-plane (side 0: da = sQ * c_p0,
 *               db = sQ * c_p1; side 1: da = sP * c_q0, db = sP * c_q1), A's edge is the boundary of A ∩ B where it is inside,
 *               B's edge elsewhere, so that a boundary that the two shapes share is counted once:
 *                   da >= 0 and db >= 0:              side 0: nothing is imposed; side 1: the edge is dropped
 *                   else da <= 0 and db <= 0:         side 0: the edge is dropped; side 1: nothing is imposed
 *                   da < 0 < db ("enters") or db < 0 < da ("leaves"): the edges split at ts = da / (da - db),
 *                       Xs = (A's edge).p0 + ts * (A's edge) — side 0: p0 + ts * ex, s = ts; side 1: q0 + ts * g,
 *                       s = ((Xs.x - p0.x) * ex.x + (Xs.y - p0.y) * ex.y) / (ex.x * ex.x + ex.y * ex.y).
 *                       Side 0 keeps the inside part: enters and s > t0: t0 = s, a = Xs; leaves and s < t1: t1 = s, b = Xs.
 *                       Side 1 keeps the other part; with sP * sQ > 0 (the edges run the same way as listed): leaves and s > t0:
 *                       t0 = s, a = Xs; enters and s < t1: t1 = s, b = Xs; with sP * sQ < 0 enters and leaves change places.
 *   a piece     a surviving edge with t0 < t1, from a to b as left by the clips (an end that no clip moved is the vertex itself):
 *               c = sP * cross(a, b);
 *               S += c, Mx += (a.x + b.x) * c, My += (a.y + b.y) * c, and the side's piece count goes up by one.  (A zero-length
 *               edge of P that survives is a piece like any other: it adds 0 to the sums and 1 to the count.)  Each side
 *               accumulates from 0 in edge order; then S = S0 + S1, Mx = Mx0 + Mx1, My = My0 + My1.
 *   the record  raw = 0.5 * S; area = min(max(raw, 0), min(area_a, area_b)), C2D_OVERLAP_CLAMPED where area != raw.
 *               iou = area / ((area_a + area_b) - area) where that denominator is > 0, else 0.
 *               S > 0: cx = r.x + Mx / (3 * S), cy = r.y + My / (3 * S); else (0, 0) with C2D_OVERLAP_NO_CENTROID.
 *               pieces_a, pieces_b: the pieces of side 0 and of side 1.  pieces_b == 0 && pieces_a == ka reads "A inside B".
 *               A float of the record that is NaN is stored as 0x7FC00000, whatever its sign and payload.
 *               A bad pair (as for the contact calls): everything 0, C2D_OVERLAP_BAD_PAIR.
 * The implementation may skip work whose result cannot reach the record; the stored bytes equal this sequential rule
 * (tests/overlap_ref.py restates it in numpy, every compare included).  For convex shapes with finite coordinates, with D the largest
 * |coordinate - r| and u = 2^-24, |area - exact| stays within a small multiple of u * D^2 (DESIGN.md §5.27 has the measured
 * constant), also where edges of the two shapes lie on one line or nearly so (aligned boxes, equal shapes listed from another
 * vertex): a pair of edges within 8 u D of one line is treated as on one line, and where both edges would do as the boundary A's
 * is the one counted.  For non-convex or non-finite input nothing is promised about what the numbers mean, only their bits.  overlaps(A, B)
 * and overlaps(B, A) may differ in the last bits: r and the shared-boundary clause are A's. */
#define C2D_OVERLAP_DEGENERATE  1  /* hit, but a shape has no area (its shoelace sum is 0 or NaN): area = iou = 0 */
#define C2D_OVERLAP_CLAMPED     2  /* 0.5 * S fell outside [0, min(area_a, area_b)] and was clamped */
#define C2D_OVERLAP_NO_CENTROID 4  /* no centroid: not hit, degenerate, or S <= 0 (shapes that only touch); cx = cy = 0 */
#define C2D_OVERLAP_BAD_PAIR    8  /* as C2D_CONTACT_BAD_PAIR */

typedef struct c2d_overlap {    /* 32 bytes, 16-byte aligned output */
    float    area;              /*  0: area of A ∩ B; 0 when not hit */
    float    iou;               /*  4: area / (area_a + area_b - area); 0 where that denominator is not > 0 */
    float    cx, cy;            /*  8: centroid of A ∩ B; (0, 0) with C2D_OVERLAP_NO_CENTROID */
    float    area_a, area_b;    /* 16: the two shapes' own areas (absolute) */
    uint8_t  hit;               /* 24: the pairwise boolean, for every input bit pattern */
    uint8_t  flags;             /* 25 */
    uint8_t  pieces_a;          /* 26: boundary pieces of A ∩ B that lie on A's edges */
    uint8_t  pieces_b;          /* 27: ... and on B's edges */
    uint32_t reserved;          /* 28: written as 0 */
} c2d_overlap;

int c2d_poly_pair_overlaps(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                           const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                           size_t row_base, size_t col_base,
                           c2d_overlap* d_out, c2d_stream stream);

int c2d_rect_pair_overlaps(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b,
                           const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                           size_t row_base, size_t col_base,
                           c2d_overlap* d_out, c2d_stream stream);

/* ---- ray queries: the nearest hit of every segment against a polygon set ---------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_ray_casts: for each of n_rays segments from o to o + d — a roadmap edge, the sweep of a reference point, a range-finder
 * beam — WHICH polygon of the set b it touches first and WHERE: the polygon, the parameter t of the hit point o + t * d, the edge
 * that was hit and the position u on it.  An R x M reduction: nothing of size n_rays x n_b is written, and no row is left for the
 * caller to reduce.  d = (0, 0) is the point query "which polygon contains o".
 *   d_rays     : four planes ox, oy, dx, dy, f32[n_rays] each; any 4-byte alignment.
 *   b          : the polygon set, as for the cross forms: rows, stride, d_k == NULL (every polygon has `rows` vertices), shards by
 *                pointer offset.  Padded vertex slots (index >= the polygon's count) are never interpreted.  A polygon with a vertex
 *                count outside 1..rows is in no hit; the error is reported by the next c2d_stream_synchronize /
 *                c2d_ctx_check_async, exactly as for the cross forms.
 *   col_base   : the global index of B_0: a hit reports col_base + j.
 *   d_out      : c2d_ray_hit[n_rays], 16-byte aligned; entry r is the record of ray r.  Records at or beyond n_rays are never touched.
 *
 * Arithmetic contract.  Everything is IEEE binary32, round to nearest, subnormals kept, nothing contracted in any
 * build; division is correctly rounded.
 *   per ray, polygon j and live edge e < k, the edge running from vertex e at (x0, y0) to vertex (e + 1) mod k at (x1, y1), each
 *   product first, then the difference:
 *               ex = x1 - x0, ey = y1 - y0, wx = x0 - ox, wy = y0 - oy,
 *               den = dx * ey - dy * ex,  tn = wx * ey - wy * ex,  un = wx * dy - wy * dx.
 *   usable edge decided without a division: den > 0 && tn >= 0 && tn <= den && un >= 0 && un <= den, or
 *               den < 0 && tn <= 0 && tn >= den && un <= 0 && un >= den.  A NaN fails every compare; den == 0 (a parallel or a
 *               zero-length edge) is unusable.  A usable edge has t = tn / den and u = un / den.
 *   origin inside  polygon j when no live tn is NaN and exactly one sign occurs among the live tn: some tn > 0 or some tn < 0, but
 *               not both.  So a zero-length edge (tn = +-0) is neutral, a polygon with k = 1 contains nothing, a clockwise polygon
 *               works, and an origin on the boundary of a proper polygon counts as inside.  An inside polygon is the candidate t = 0.
 *   the pick    polygons are visited in order of j, per polygon the inside candidate first and then the edges in order of e.  The
 *               best starts at +inf with nothing chosen; a candidate replaces it only under strict t < best (compare and select), so
 *               a NaN t never wins.  Equivalently: the smallest t wins, among equal t the smallest j, then inside before edges,
 *               then the smallest e.  Ties are real: a ray through a vertex reaches the same t on two edges, duplicated obstacles
 *               reach it on two polygons.
 *   the record  an edge winner: hit = 1, poly = col_base + j, its t and u, edge = e, flags = 0.  An inside winner: hit = 1,
 *               poly = col_base + j, t = 0, u = 0, edge = 0xFFFF, flags = C2D_RAY_START_INSIDE.  Nothing chosen: hit = 0,
 *               poly = 0xFFFFFFFF, t = +inf, u = 0, edge = 0xFFFF, flags = 0.
 * The implementation evaluates polygons in parallel; its results equal this sequential rule.  +0 and -0 compare equal in t and u.
 * t is never NaN; u can be (inf / inf, with an infinite coordinate), and then any NaN stands for it.
 * For non-convex input nothing is promised about what "inside" means, only the bits.
 *
 * n_rays == 0 is a no-op; n_b == 0 writes the no-hit record for every ray.  A NULL argument, `rows` out of range, a misaligned d_out,
 * col_base + n_b > 2^32 and n_rays > 2^32 are refused (C2D_ERR_INVALID_ARG) before a device is touched.  The call is asynchronous
 * on `stream` with no host synchronisation, and deterministic: two runs give the same bytes.  It uses no ctx scratch and is
 * graph-capturable (three kernel nodes in a chain). */
#define C2D_RAY_START_INSIDE 1   /* the origin lies in (or on) the winning polygon: t = 0, u = 0, edge = 0xFFFF */

typedef struct c2d_ray_hit {     /* 16 bytes, 16-byte aligned output */
    uint32_t poly;               /*  0: col_base + j of the winning polygon; 0xFFFFFFFF: none */
    float    t;                  /*  4: hit point = o + t * d, 0 <= t <= 1; +inf: none */
    float    u;                  /*  8: position on the winning edge, v[e] + u * (v[e+1] - v[e]); 0 when none / START_INSIDE */
    uint16_t edge;               /* 12: 0..k-1; 0xFFFF: none or START_INSIDE */
    uint8_t  hit;                /* 14 */
    uint8_t  flags;              /* 15 */
} c2d_ray_hit;

int c2d_poly_ray_casts(c2d_ctx* ctx, const float* const d_rays[4] /* ox, oy, dx, dy: f32[n_rays] each */, size_t n_rays,
                       const c2d_poly_set* b, size_t col_base, c2d_ray_hit* d_out, c2d_stream stream);

/* ---- ray queries through a grid ----------------------------------------------------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_ray_casts_grid: the ray query for many polygons and short segments.  It walks a uniform grid over B along each segment
 * instead of visiting every edge of every polygon.  The arguments, the record, the refused arguments, the vertex count outside
 * 1..rows (in no hit, C2D_ASYNC_ERR_POLY_K), n_rays == 0 (a no-op), n_b == 0 (the no-hit record for every ray) and the untouched
 * records at or beyond n_rays are those of c2d_poly_ray_casts.  It has a contract of its own:
 *
 *   the box of polygon j (count in 1..rows): xl, xh, yl, yh are the binary32 minimum / maximum of its live vertices' x and y.  A
 *               polygon with a NaN live coordinate is UNBOXED and is a candidate of every ray.
 *   meets(r, j) in binary64, unfused, in the written order, from the float inputs:
 *               bx = ox + dx, by = oy + dy;
 *               C  = the largest magnitude among ox, oy, bx, by, xl, xh, yl, yh (NaN when one of them is);
 *               m  = 2^-20 * C;
 *               sx = min(ox, bx) > xh + m || max(ox, bx) < xl - m,  and sy likewise with oy, by, yl, yh;
 *               cx = 0.5 * xl + 0.5 * xh,  hx = (0.5 * xh - 0.5 * xl) + m,  and cy, hy likewise;
 *               sn = |dx * (cy - oy) - dy * (cx - ox)| > hx * |dy| + hy * |dx|;
 *               meets = !(sx || sy || sn).
 *               A NaN fails every compare, so a non-finite ray or an infinite box meets.
 *   the result  for ray r: the pick of c2d_poly_ray_casts restricted to { j : unboxed(j) || meets(r, j) }: the per-polygon rule,
 *               the order, the ties and the record are unchanged.  It is deterministic (two runs give the same bytes) and does not
 *               depend on how the grid is traversed.
 *
 * Relation to c2d_poly_ray_casts.  Wherever the segment really touches a polygon, meets holds, and the two calls agree byte for
 * byte: on the project's ray scenes, their copies scaled by 1e-30 .. 1e30 and every hand case, no touched pair fails meets
 * (tests/test_ray_grid_ref_cpu.py).  They are NOT equal for every bit pattern, and cannot be: the brute-force rule's booleans are not
 * bounded by any box.  With a ray nearly collinear with an edge, den, tn and un are rounding noise, and c2d_poly_ray_casts then reports
 * hits on polygons hundreds of units away from the segment (about 0.75 % of such rays against a square or a triangle, 13 % against a
 * 2-gon).  The grid call reports no hit there.
 *
 * Unlike c2d_poly_ray_casts it uses the ctx scratch, as c2d_sat_poly_broad_pairs does: the workspace guard applies (one stream at a time
 * per ctx), the scratch grows on demand (about 48 bytes per polygon and 36 per ray), and graph capture works after an eager call of
 * the same or a larger n_rays and n_b; a capture that would have to grow the scratch is refused (C2D_ERR_INVALID_ARG) before anything
 * is enqueued.  Use it from a few thousand polygons on; below that c2d_poly_ray_casts is the faster call. */
int c2d_poly_ray_casts_grid(c2d_ctx* ctx, const float* const d_rays[4] /* ox, oy, dx, dy: f32[n_rays] each */, size_t n_rays,
                            const c2d_poly_set* b, size_t col_base, c2d_ray_hit* d_out, c2d_stream stream);

/* Diagnostics of the last c2d_poly_ray_casts_grid call with n_b > 0 on this ctx, read back with a blocking copy; call it after that
 * call's stream has been synchronised and before any other call that uses the ctx scratch (otherwise C2D_ERR_INVALID_ARG, or the
 * counters of a call in flight).  out[0] = rays that left the walk for the one-ray-per-wave route (non-finite, C >= 2^60, or more than
 * 1024 sorted entries to visit), out[1] = sorted entries the walks visited, out[2] = of those, the ones that passed meets,
 * out[3] = regular polygons tested against every ray because their box may lie outside the grid's bounds. */
int c2d_poly_ray_casts_grid_stats(c2d_ctx* ctx, unsigned long long out[4]);

/* ---- clearance queries: the nearest polygon of a set for every query polygon ------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_set_clearances: for each polygon A_i of the set a — a robot link, a footprint along a path — WHICH polygon of the set b is
 * nearest to it, HOW far it is and WHERE the two closest points lie.  An N x M reduction over the distance contract above: nothing of
 * size n_a x n_b is written, and no row is left for the caller to reduce.  (The broad-phase lists hold only pairs whose boxes
 * overlap: they cannot answer this.)
 *   a, b       : the polygon sets, as for the cross forms: rows, stride, d_k == NULL (every polygon has `rows` vertices), shards by
 *                pointer offset; a and b may be the same memory.  Rectangles go in as 4-gons with rows = 4.  Padded vertex slots are
 *                never interpreted.
 *   row_base   : the global index of A_0;  col_base: the global index of B_0: a record reports col_base + j.
 *   flags      : 0 or C2D_CLEARANCE_SKIP_SELF (self-clearance of one set: a == b, row_base == col_base).
 *   d_out      : c2d_clearance[n_a], 16-byte aligned; entry i is the record of A_i.  Records at or beyond n_a are never touched.
 *
 * The contract, stated through the distance contract.
 *   per-pair records   for query i, D(i, j) is the c2d_distance record that c2d_poly_pair_distances defines for the pair (A_i, B_j).
 *   considered         polygon j is considered when its vertex count is within 1..rows and it is not the self pair; with
 *                      C2D_CLEARANCE_SKIP_SELF the self pair is the one with row_base + i == col_base + j, without the flag there is none.
 *   the pick           the winner j* is the considered polygon with the smallest key (bits of D(i, j).dist, col_base + j).  dist is
 *                      never NaN and never -0 and a hit pair has dist = +0, so the order of the bits is the order of the values;
 *                      equal distances fall to the smaller index.  Ties are real: duplicated obstacles, two obstacles equally far, a
 *                      hit and a separated pair whose d2 underflowed to 0.  A C2D_DISTANCE_NO_CANDIDATE pair has dist = +inf: it
 *                      wins only when nothing nearer is considered.
 *   the record         a winner exists: poly = col_base + j*, and dist, ax, ay, bx, by, edge, vert, hit and flags are the same-named
 *                      fields of D(i, j*), bit for bit (+0 and -0 compare equal in the five floats); reserved0 = 0.
 *                      Nothing considered (n_b == 0, only bad polygons, only the self pair): poly = 0xFFFFFFFF, dist = +inf, both
 *                      points (0, 0), edge = vert = 0xFFFF, hit = 0, flags = C2D_CLEARANCE_NONE.
 *                      A query with a vertex count outside 1..rows: poly = 0xFFFFFFFF, everything else 0, edge = vert = 0xFFFF,
 *                      flags = C2D_DISTANCE_BAD_PAIR.
 * A vertex count outside 1..rows in a or b is reported by the next c2d_stream_synchronize / c2d_ctx_check_async
 * (C2D_ASYNC_ERR_POLY_K), as for the ray call.  The implementation evaluates polygons in parallel and may skip the candidates of a
 * pair that a certified bound proves no nearer than the best so far; its results equal the rule above.
 *
 * n_a == 0 is a no-op.  NULL arguments, `rows` out of range, misaligned planes or a misaligned d_out, stride < n, unknown flag bits and
 * row_base + n_a or col_base + n_b above 2^32 are refused (C2D_ERR_INVALID_ARG) before a device is touched.  The call is asynchronous
 * on `stream` with no host synchronisation, and deterministic: two runs give the same bytes.  It uses no ctx scratch (the workspace
 * guard is not involved) and is graph-capturable (a chain of kernel nodes). */
#define C2D_CLEARANCE_SKIP_SELF 1   /* call flag: the pair with row_base + i == col_base + j is not considered */
#define C2D_CLEARANCE_NONE 16       /* record flag: no polygon of B was considered */

typedef struct c2d_clearance {  /* 32 bytes, 16-byte aligned output */
    uint32_t poly;              /*  0: col_base + j of the winner; 0xFFFFFFFF: none */
    float    dist;              /*  4 */
    float    ax, ay;            /*  8: closest point on A_i */
    float    bx, by;            /* 16: closest point on the winner */
    uint16_t edge, vert;        /* 24, 26 */
    uint8_t  hit, flags;        /* 28, 29: flags = the C2D_DISTANCE_* bits of the winning pair, or C2D_CLEARANCE_NONE */
    uint16_t reserved0;         /* 30: written as 0 */
} c2d_clearance;

int c2d_poly_set_clearances(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                            size_t row_base, size_t col_base, int flags,
                            c2d_clearance* d_out, c2d_stream stream);

/* ---- swept queries: time of impact for listed pairs in linear motion ------------
 * Additions to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_pair_sweeps / c2d_rect_pair_sweeps: for each pair of a list, with BOTH shapes translating over the step t = 0 .. 1,
 * whether they touch during the step, the first time at which they do, and the unit normal from A towards B at that touch with the
 * axis it came from.  (Testing sampled instants tunnels: a grazing pass falls between two samples.)  The sets, d_pairs, d_n_pairs,
 * the bases, the records at or beyond min(n_pairs, *d_n_pairs) (untouched), bad pairs, the asynchronous error word, n_pairs == 0
 * (a no-op), the refused arguments, "no ctx scratch", the single launch, `stream` and graph capture are those of
 * c2d_poly_pair_distances / c2d_rect_pair_distances, that is, of the contact queries above.
 *   d_a_dx, d_a_dy : f32[n_a] each, 4-byte aligned: the displacement of object i of A over the step.  The index is LOCAL, like the
 *                    vertex planes': a shard passes the motion planes offset by the same amount as its vertices.
 *   d_b_dx, d_b_dy : the same for B.
 *                    A set whose two planes are both NULL stands still.  Exactly one NULL plane of a set is refused
 *                    (C2D_ERR_INVALID_ARG), before the other checks.
 *   d_out          : c2d_sweep[n_pairs], 16-byte aligned; entry p is the record of list entry p.
 *
 * Arithmetic contract.  Everything is IEEE binary32, round to nearest, subnormals kept, nothing contracted in any
 * build; division and square root are correctly rounded.
 *   hit0        the pairwise boolean itself (c2d_sat_poly_pairs_rows / c2d_sat_rect_pairs_verts of the same build on the pair as it
 *               stands at t = 0): exactly the `hit` of the contact calls.  When hit0: toi = 0, normal (0, 0), axis = 0xFFFF, hit = 1,
 *               flags = C2D_SWEEP_START_OVERLAP (how deep and along which normal is the contact calls' business).
 *   motion      rx = b_dx[j] - a_dx[i], ry = b_dy[j] - a_dy[i]: the displacement of B relative to A.  A set that stands still
 *               contributes +0.
 *   axes        the axes, their order and the intervals [minA, maxA], [minB, maxB] are those of the contact contract: for polygons
 *               the true normals (-ey, ex) of A's live edges (axis e), then B's (axis ka + e); for rectangles the eight edge
 *               vectors; min / max the running fmin / fmax of nx * x + ny * y over the live vertices.
 *               o1 = maxA - minB,  o2 = maxB - minA,  v = nx * rx + ny * ry (each product first, then the sum).
 *   per live axis, in axis order:
 *               v > 0:  lo = (-o2) / v,  hi = o1 / v.       v < 0:  lo = o1 / v,  hi = (-o2) / v.
 *               v == 0: the axis bounds nothing, unless o1 < 0 || o2 < 0: then `never` is set (it separates for the whole step).
 *               v NaN:  the axis is ignored.
 *   the pick    t_in starts at +0 with no axis, t_out at 1.  lo > t_in replaces t_in and records the axis and the sign of v;
 *               hi < t_out replaces t_out (compare and select, not fmax: a NaN bound fails the compare and is ignored, and among
 *               equal lo the first axis wins).
 *   the record  hit = !never && t_in <= t_out.  On a hit: toi = t_in, axis = the recorded one, (nx, ny) = s * (nx / len, ny / len)
 *               of that axis with len = sqrt(nx * nx + ny * ny), s = +1 when v < 0 and -1 when v > 0 (the unit normal from A
 *               towards B at the touch), flags = 0.  A hit whose t_in kept its start (every lo underflowed to 0 or below) has
 *               normal (0, 0) and axis = 0xFFFF, and C2D_SWEEP_START_OVERLAP stays clear: that flag means hit0 and nothing else.
 *               On a miss: toi = +inf, normal (0, 0), axis = 0xFFFF, hit = 0, flags = 0.  A bad pair (as for the contact calls):
 *               everything 0, axis = 0xFFFF, flags = C2D_SWEEP_BAD_PAIR.
 * A zero-length live edge has v = o1 = o2 = 0 and bounds nothing, so len is never 0 for a winner.  +0 and -0 compare equal in the
 * three floats.  For convex polygons in translation the rule is exact: the closed shapes first touch at the largest lo, and they
 * have parted again once a hi is passed.  For non-convex input only the bits are promised.  t_out, the time of separation, is not
 * returned, and rotation during the step is out of scope. */
#define C2D_SWEEP_START_OVERLAP 1u  /* the pair is hit at t = 0 (hit0): toi = 0, normal (0, 0), axis = 0xFFFF */
#define C2D_SWEEP_BAD_PAIR      2u  /* as C2D_CONTACT_BAD_PAIR */

typedef struct c2d_sweep {      /* 16 bytes, 16-byte aligned output */
    float    toi;               /*  0: first time of touch in 0 .. 1; +inf: none during the step */
    float    nx, ny;            /*  4: unit normal from A towards B at the touch; (0, 0) when there is no axis */
    uint16_t axis;              /* 12: 0..ka-1: edge of A, ka..ka+kb-1: edge of B (rectangles: 0..3, 4..7); 0xFFFF: none */
    uint8_t  hit;               /* 14: the shapes touch at some t in 0 .. 1 */
    uint8_t  flags;             /* 15: C2D_SWEEP_START_OVERLAP, C2D_SWEEP_BAD_PAIR */
} c2d_sweep;

int c2d_poly_pair_sweeps(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                         const float* d_a_dx, const float* d_a_dy, const float* d_b_dx, const float* d_b_dy,
                         const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                         size_t row_base, size_t col_base,
                         c2d_sweep* d_out, c2d_stream stream);

int c2d_rect_pair_sweeps(c2d_ctx* ctx, const float* const d_a[8], size_t n_a, const float* const d_b[8], size_t n_b,
                         const float* d_a_dx, const float* d_a_dy, const float* d_b_dx, const float* d_b_dy,
                         const uint32_t* d_pairs, size_t n_pairs, const unsigned long long* d_n_pairs,
                         size_t row_base, size_t col_base,
                         c2d_sweep* d_out, c2d_stream stream);

/* ---- shape casts: the first touch of each moving polygon against a set -----------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_set_casts: for each polygon A_i of the set a — a footprint moving over one time step — WHICH polygon of the set b it
 * touches first, WHEN, and with which normal.  An N x M reduction over the sweep contract above, as the clearance call is one over the
 * distance contract: nothing of size n_a x n_b is written, and no row is left for the caller to reduce.  (The broad-phase lists hold
 * only pairs whose boxes overlap at t = 0: they miss exactly the pairs a sweep is for.)
 *   a, b       : the polygon sets, as for the clearance call: rows, stride, d_k == NULL, shards by pointer offset; a and b may be the
 *                same memory.  Polygons only: rectangles go in as 4-gons with rows = 4.
 *   d_a_dx, d_a_dy, d_b_dx, d_b_dy : the motion planes of the swept queries: f32[n] each, 4-byte aligned, LOCAL indices (a shard
 *                passes them offset like its vertices).  A set whose two planes are both NULL stands still.  Exactly one NULL
 *                plane of a set is refused (C2D_ERR_INVALID_ARG), before the other checks.
 *   row_base   : the global index of A_0;  col_base: the global index of B_0: a record reports col_base + j.
 *   flags      : 0 or C2D_CAST_SKIP_SELF (one set against itself: a == b, row_base == col_base, the same motion planes).
 *   d_out      : c2d_cast[n_a], 8-byte aligned; entry i is the record of A_i.  Records at or beyond n_a are never touched.
 *
 * The contract, stated through the sweep contract.
 *   per-pair records   for query i, S(i, j) is the c2d_sweep record that c2d_poly_pair_sweeps defines for the pair (A_i, B_j) with
 *                      these motion planes.
 *   considered         polygon j is considered when its vertex count is within 1..rows and it is not the self pair; with
 *                      C2D_CAST_SKIP_SELF the self pair is the one with row_base + i == col_base + j, without the flag there is none.
 *   the pick           among the considered j with S(i, j).hit == 1, the winner j* has the smallest key (bits of S(i, j).toi, col_base + j).
 *                      A hit's toi is t_in: it starts at +0 and is replaced only by a larger value, so it is never NaN and never -0
 *                      and at most 1, and the order of the bits is the order of the values; equal times fall to the smaller index.
 *                      Ties are real: duplicated obstacles, a start overlap against a hit at +0 with no axis, symmetric scenes.
 *   the record         a winner exists: poly = col_base + j*, and toi, nx, ny, axis, hit and flags are the same-named fields of
 *                      S(i, j*), bit for bit (+0 and -0 compare equal in the three floats); reserved0 = 0.
 *                      No considered polygon is hit (n_b == 0, only bad polygons, only the self pair, all misses): poly = 0xFFFFFFFF,
 *                      toi = +inf, normal (0, 0), axis = 0xFFFF, hit = 0, flags = 0.
 *                      A query with a vertex count outside 1..rows: poly = 0xFFFFFFFF, everything else 0, axis = 0xFFFF,
 *                      flags = C2D_SWEEP_BAD_PAIR.
 * A vertex count outside 1..rows in a or b is reported by the next c2d_stream_synchronize / c2d_ctx_check_async
 * (C2D_ASYNC_ERR_POLY_K).  The implementation evaluates polygons in parallel and leaves the axes of a pair as soon as the pair can no
 * longer win; its results equal the rule above.
 *
 * n_a == 0 is a no-op.  NULL arguments, `rows` out of range, misaligned planes or motion planes, a d_out that is not 8-byte aligned,
 * stride < n, unknown flag bits, half a motion and row_base + n_a or col_base + n_b above 2^32 are refused (C2D_ERR_INVALID_ARG)
 * before a device is touched.  The call is asynchronous on `stream` with no host synchronisation, and deterministic: two runs give
 * the same bytes.  It uses no ctx scratch (the workspace guard is not involved) and is graph-capturable (a chain of kernel nodes). */
#define C2D_CAST_SKIP_SELF 1   /* call flag: the pair with row_base + i == col_base + j is not considered */

typedef struct c2d_cast {   /* 24 bytes, 8-byte aligned output */
    uint32_t poly;          /*  0: col_base + j of the winner; 0xFFFFFFFF: none */
    float    toi;           /*  4 */
    float    nx, ny;        /*  8 */
    uint16_t axis;          /* 16 */
    uint8_t  hit, flags;    /* 18, 19: flags = the C2D_SWEEP_* bits of the winning pair */
    uint32_t reserved0;     /* 20: written as 0 */
} c2d_cast;

int c2d_poly_set_casts(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                       const float* d_a_dx, const float* d_a_dy, const float* d_b_dx, const float* d_b_dy,
                       size_t row_base, size_t col_base, int flags, c2d_cast* d_out, c2d_stream stream);

/* ---- swept broad-phase pair search of two convex polygon sets ---------------------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_sweep_broad_pairs: every pair of two polygon sets that touches during one step — the front end of the swept queries, as
 * c2d_sat_poly_broad_pairs is the front end of the static ones (whose lists hold only pairs that overlap at t = 0).
 *
 * The contract, stated through the sweep contract.  S(i, j) is the c2d_sweep record that c2d_poly_pair_sweeps defines for the pair
 * (A_i, B_j) with these motion planes and row_base = col_base = 0.  The call returns the list of all (i, j), in row-major order,
 * with S(i, j).hit == 1 — for every input bit pattern: NaN, inf, huge and subnormal coordinates and motions, degenerate and
 * clockwise polygons, repeated vertices, sets with different `rows`, any `stride`, d_k == NULL.  A polygon with a vertex count
 * outside 1..rows is in no pair (its S is the BAD_PAIR record, hit = 0) and is not counted; the error is reported by the next
 * c2d_stream_synchronize / c2d_ctx_check_async (C2D_ASYNC_ERR_POLY_K).  With C2D_CROSS_UPPER only the pairs with j > i are listed.
 * Every pair of c2d_sat_poly_broad_pairs' list is in this one (a pair that overlaps at t = 0 is a hit with
 * C2D_SWEEP_START_OVERLAP).
 *
 * The pairs are found through the broad phase of c2d_sat_poly_broad_pairs (the same grid, sort, scan, count and emit pipeline) on
 * SWEPT conservative boxes: the hull of the polygon's box of that call, its slabs widened for the sweep rule's own roundings, at
 * t = 0 and displaced by the polygon's motion.  DESIGN.md §5.19 proves that no pair is lost.  Polygons the argument does not cover
 * ("wild") are tested against everything: what is wild for c2d_sat_poly_broad_pairs, a non-finite motion component, a |motion
 * component| >= 2^60, a displaced |coordinate| >= 2^60.  A box far wider than the scene's typical one is wild too, so ONE fast
 * outlier costs n_b exact tests (n_a + n_b when it is in both sets); a scene in which many polygons move many polygon sizes per
 * step belongs to c2d_poly_set_casts or to shorter steps.
 *   a, b       : as c2d_sat_poly_broad_pairs.  Polygons only: rectangles go in as 4-gons with rows = 4.  a and b may describe the
 *                same memory (same pointers, n, stride, rows, d_k AND the same motion planes): the boxes and the sort are then
 *                made once, and with C2D_CROSS_UPPER that is the continuous self-collision test of one set.  One set against
 *                itself with different motion planes is two sets.
 *   d_a_dx, d_a_dy, d_b_dx, d_b_dy : the motion planes of the swept queries: f32[n] each, 4-byte aligned.  A set whose two planes
 *                are both NULL stands still.  Exactly one NULL plane of a set is refused (C2D_ERR_INVALID_ARG), before the other
 *                checks.
 *   flags      : 0, or C2D_CROSS_UPPER: only the pairs with j > i.
 *   d_pairs, capacity, d_count : u32[capacity][2] of (i, j) in row-major order, only the first `capacity` pairs written;
 *                d_count (required) is incremented by the TOTAL; d_pairs may be NULL when capacity is 0 (a count-only call,
 *                which skips the emit pass).
 * The chain.  The list and its device-side count feed the narrow phase with no host synchronisation, on one stream:
 *     c2d_poly_sweep_broad_pairs(ctx, a, b, adx, ady, bdx, bdy, flags, d_pairs, capacity, d_count, s);     (d_count zeroed before)
 *     c2d_poly_pair_sweeps(ctx, a, b, adx, ady, bdx, bdy, d_pairs, capacity, d_count, 0, 0, d_out, s);     (d_n_pairs = d_count)
 * The second call processes min(capacity, *d_count) entries; every record it writes has hit == 1.
 *
 * n_a == 0 or n_b == 0 is a no-op.  A call with n_a or n_b above 2^32 is refused; an unknown flag, a NULL argument, `rows`
 * outside 1..C2D_POLY_KMAX, half a motion or a misaligned motion plane is refused (C2D_ERR_INVALID_ARG) before a device is
 * touched.  Asynchronous on `stream`, with no host synchronisation; the output is deterministic.  It works through the ctx scratch
 * under the workspace guard, which it grows on first use and keeps; the size depends only on (n_a, n_b, same memory): 36 bytes
 * per polygon of A plus 48.5 per polygon of B (68.5 per polygon when B is A: the boxes are shared) and a 4 KiB header.  Graph
 * capture follows c2d_sat_poly_broad_pairs: allowed after an eager call of the same or a larger size, refused
 * (C2D_ERR_INVALID_ARG) before anything is enqueued if the scratch would have to grow. */
int c2d_poly_sweep_broad_pairs(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                               const float* d_a_dx, const float* d_a_dy, const float* d_b_dx, const float* d_b_dy,
                               int flags,                               /* 0 or C2D_CROSS_UPPER (j > i only) */
                               uint32_t* d_pairs, size_t capacity,      /* u32[capacity][2] */
                               unsigned long long* d_count, c2d_stream stream);

/* ---- proximity pair search of two convex polygon sets: every pair within a distance -
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_near_broad_pairs: every pair of two polygon sets that is hit or no farther apart than max_dist — the front end of the
 * distance queries (a safety margin, speculative contacts, the neighbours of a potential field), as c2d_sat_poly_broad_pairs is the
 * front end of the static ones (whose lists hold only pairs that overlap: c2d_poly_pair_distances answers those with dist = 0).
 *
 * The contract, stated through the distance contract.  D(i, j) is the c2d_distance record that c2d_poly_pair_distances defines for
 * the pair (A_i, B_j) with row_base = col_base = 0.  The call returns the list of all (i, j), in row-major order, with
 *     D(i, j).hit == 1 || D(i, j).dist <= max_dist
 * — a binary32 compare on the record's own dist, for every input bit pattern: NaN, inf, huge and subnormal coordinates, degenerate
 * and clockwise polygons, repeated vertices, sets with different `rows`, any `stride`, d_k == NULL.  A pair without a usable
 * candidate (C2D_DISTANCE_NO_CANDIDATE, dist = +inf) is listed only when it is hit.  A polygon with a vertex count outside 1..rows is
 * in no pair (its D is the BAD_PAIR record) and is not counted; the error is reported by the next c2d_stream_synchronize /
 * c2d_ctx_check_async (C2D_ASYNC_ERR_POLY_K).  With C2D_CROSS_UPPER only the pairs with j > i are listed.  Three consequences:
 *   superset     for any admissible max_dist the list contains the list of c2d_sat_poly_broad_pairs on the same sets (its pairs are
 *                the hit ones);
 *   monotone     the list of a larger max_dist contains the list of a smaller one;
 *   the chain    the list and its device-side count feed c2d_poly_pair_distances with no host synchronisation, on one stream:
 *                    c2d_poly_near_broad_pairs(ctx, a, b, max_dist, flags, d_pairs, capacity, d_count, s);     (d_count zeroed before)
 *                    c2d_poly_pair_distances(ctx, a, b, d_pairs, capacity, d_count, 0, 0, d_out, s);           (d_n_pairs = d_count)
 *                The second call processes min(capacity, *d_count) entries; every record it writes has hit == 1 || dist <= max_dist.
 *                The contact, manifold and sweep calls take the list the same way.
 *
 * The pairs are found through the broad phase of c2d_sat_poly_broad_pairs (the same grid, sort, scan, count and emit pipeline) on
 * conservative boxes that hold the margin: the hull of the polygon's box of that call and of the box of its live vertices widened
 * on every side by half of max_dist and by what the distance rule's roundings need.  DESIGN.md §5.20 proves that no pair is lost.
 * Polygons the argument does not cover ("wild") are tested against everything: what is wild for c2d_sat_poly_broad_pairs (1- and
 * 2-gons among them) and a polygon whose largest |coordinate| is below 2^-100.  A box far wider than the scene's typical one is wild
 * too.  The cost grows with the candidates: a max_dist of many polygon sizes makes every polygon a neighbour of many.
 *   a, b       : as c2d_sat_poly_broad_pairs.  Polygons only: rectangles go in as 4-gons with rows = 4.  a and b may describe the
 *                same memory (same pointers, n, stride, rows and d_k): the boxes and the sort are then made once, and with
 *                C2D_CROSS_UPPER that is the neighbour search of one set.
 *   max_dist   : finite, 0 <= max_dist < 2^60; -0 counts as 0.  Anything else, NaN included, is refused (C2D_ERR_INVALID_ARG) before
 *                a device is touched and before the sets are looked at.  max_dist = 0 lists the hit pairs and the separated pairs
 *                whose d2 underflowed to 0.
 *   flags      : 0, or C2D_CROSS_UPPER: only the pairs with j > i.
 *   d_pairs, capacity, d_count : u32[capacity][2] of (i, j) in row-major order, only the first `capacity` pairs written;
 *                d_count (required) is incremented by the TOTAL; d_pairs may be NULL when capacity is 0 (a count-only call,
 *                which skips the emit pass).
 *
 * n_a == 0 or n_b == 0 is a no-op.  A call with n_a or n_b above 2^32 is refused; an unknown flag, a NULL argument or `rows`
 * outside 1..C2D_POLY_KMAX is refused (C2D_ERR_INVALID_ARG) before a device is touched, in the order of c2d_sat_poly_broad_pairs.
 * Asynchronous on `stream`, with no host synchronisation; the output is deterministic.  It works through the ctx scratch under the
 * workspace guard, which it grows on first use and keeps; the size is that of c2d_sat_poly_broad_pairs and depends only on
 * (n_a, n_b, same memory).  Graph capture follows c2d_sat_poly_broad_pairs: allowed after an eager call of the same or a larger
 * size, refused (C2D_ERR_INVALID_ARG) before anything is enqueued if the scratch would have to grow. */
int c2d_poly_near_broad_pairs(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                              float max_dist,                          /* finite, 0 <= max_dist < 2^60 */
                              int flags,                               /* 0 or C2D_CROSS_UPPER (j > i only) */
                              uint32_t* d_pairs, size_t capacity,      /* u32[capacity][2] */
                              unsigned long long* d_count, c2d_stream stream);

/* ---- clearance queries through a grid: the nearest polygon within a distance ---------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_set_clearances_grid: c2d_poly_set_clearances restricted to the obstacles that are hit or no farther than max_dist, found
 * through the grid of the pair searches instead of a visit to all n_a x n_b pairs: "which obstacle is nearest to each of my 10^5
 * footprints, among 10^6 obstacles, if any is within the margin".  It is the reduction of the list of c2d_poly_near_broad_pairs, made
 * on the device with nothing of that list written.
 *
 * The contract is the contract of c2d_poly_set_clearances (above), word for word, with one more clause in "considered":
 *   considered         polygon j is considered for query i when its vertex count is within 1..rows, it is not the self pair (with
 *                      C2D_CLEARANCE_SKIP_SELF the pair with row_base + i == col_base + j, without the flag there is none) and
 *                          D(i, j).hit == 1 || D(i, j).dist <= max_dist
 *                      — the binary32 compare of c2d_poly_near_broad_pairs on the record's own dist, for every input bit pattern.
 *                      A C2D_DISTANCE_NO_CANDIDATE pair (dist = +inf) is considered only when it is hit.
 *   the pick           unchanged: the considered polygon with the smallest key (bits of D(i, j).dist, col_base + j); equal distances
 *                      fall to the smaller index.
 *   the record         unchanged: the winner's fields copied from D(i, j*) bit for bit; the C2D_CLEARANCE_NONE record for a query with
 *                      nothing considered, which now includes "nothing within max_dist"; the C2D_DISTANCE_BAD_PAIR record for a query
 *                      with a vertex count outside 1..rows.
 * Three consequences:
 *   the cut      a record whose poly is not 0xFFFFFFFF has hit == 1 || dist <= max_dist;
 *   NONE         a query gets the NONE record exactly when row i of the list of c2d_poly_near_broad_pairs is empty for the same
 *                sets and max_dist (with the self pair removed under C2D_CLEARANCE_SKIP_SELF);
 *   all winners  where every query of a call has a winner, the output is byte for byte that of c2d_poly_set_clearances.
 * Raising max_dist only turns NONE records into winners: it never changes a winner.
 *
 *   a, b       : as c2d_poly_near_broad_pairs: rows, stride, d_k == NULL; a and b may describe the same memory (same pointers, n,
 *                stride, rows and d_k): the boxes and the sort are then made once.
 *   max_dist   : finite, 0 <= max_dist < 2^60; -0 counts as 0.  Anything else, NaN included, is refused (C2D_ERR_INVALID_ARG) before a
 *                device is touched and before the sets are looked at.
 *   row_base, col_base, flags, d_out : as c2d_poly_set_clearances (flags: 0 or C2D_CLEARANCE_SKIP_SELF; d_out: c2d_clearance[n_a],
 *                16-byte aligned).  Records at or beyond n_a are never touched.
 *
 * n_a == 0 is a no-op; n_b == 0 writes the NONE record (BAD_PAIR for a bad query) for every query.  NULL arguments, `rows` out of
 * range, misaligned planes or a misaligned d_out, stride < n, unknown flag bits, n_a or n_b above 2^32 and row_base + n_a or
 * col_base + n_b above 2^32 are refused (C2D_ERR_INVALID_ARG) before a device is touched.  A vertex count outside 1..rows in a or b is
 * reported by the next c2d_stream_synchronize / c2d_ctx_check_async (C2D_ASYNC_ERR_POLY_K).
 *
 * The candidates are found as c2d_poly_near_broad_pairs finds them (the same margin boxes, grid and sort; polygons it calls wild are
 * compared with everything), and a certified bound skips the candidate walk of a pair that cannot be considered or cannot win; the
 * results equal the rule above.  The cost grows with the candidates: a max_dist of many polygon sizes makes every
 * polygon a neighbour of many.  Asynchronous on `stream`, with no host synchronisation; deterministic: two runs give the same bytes.
 * It works through the ctx scratch under the workspace guard, which it grows on first use and keeps; the size is that of
 * c2d_sat_poly_broad_pairs and depends only on (n_a, n_b, same memory).  Graph capture follows c2d_sat_poly_broad_pairs: allowed after
 * an eager call of the same or a larger size, refused (C2D_ERR_INVALID_ARG) before anything is enqueued if the scratch would have to
 * grow. */
int c2d_poly_set_clearances_grid(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                                 float max_dist,            /* finite, 0 <= max_dist < 2^60; -0 counts as 0 */
                                 size_t row_base, size_t col_base, int flags,   /* 0 or C2D_CLEARANCE_SKIP_SELF */
                                 c2d_clearance* d_out, c2d_stream stream);

/* The counters of the last c2d_poly_set_clearances_grid call with n_b > 0 on this ctx, for measurements (csrc/tools/clearance_grid_bench.py):
 * synchronise the call's stream first; the read blocks.  Refused when no such call has run, or when another call has used the ctx
 * scratch since.  out[0] = queries answered by the list kernel (wild ones, and walks past the candidate cap), out[1] = sorted grid
 * entries the walks looked at, out[2] = candidates (entries whose box meets the query's, wild polygons, and what the list kernel's
 * box filter let through), out[3] = of those, the pairs that ran the pairwise test, out[4] = of those, the pairs that ran the
 * candidate walk of the distance rule (the certified bound skipped the others). */
int c2d_poly_set_clearances_grid_stats(c2d_ctx* ctx, unsigned long long out[5]);

/* ---- shape casts through a grid: each moving polygon's first touch via the grid -------
 * An addition to 0.6 (c2d_version() stays 6), found by symbol lookup like the calls above.
 *
 * c2d_poly_set_casts_grid: c2d_poly_set_casts (above) found through the grid of the pair searches instead of a visit to all
 * n_a x n_b pairs: "which obstacle does each of my 10^5 footprints touch first in this step, among 10^5 or 10^6 obstacles, when, and
 * with which face".  It is the per-row reduction of the chain c2d_poly_sweep_broad_pairs + c2d_poly_pair_sweeps, made on the device
 * with nothing of that list written.
 *
 * The contract is the contract of c2d_poly_set_casts, word for word: the per-pair records S(i, j), which polygons are considered, the
 * pick by the key (bits of S(i, j).toi, col_base + j), the three records (a winner's, the miss record, the C2D_SWEEP_BAD_PAIR record of
 * a query with a vertex count outside 1..rows), C2D_CAST_SKIP_SELF, and C2D_ASYNC_ERR_POLY_K reported by the next
 * c2d_stream_synchronize / c2d_ctx_check_async for a vertex count outside 1..rows in a or b.  The consequence: on the same arguments
 * the two calls write the same bytes, for every input bit pattern — NaN, inf, huge and subnormal coordinates and motions, degenerate
 * and clockwise polygons, ties, any order of the obstacles.  No margin and no tolerance enters: two regular polygons whose swept boxes
 * (those of c2d_poly_sweep_broad_pairs) are disjoint have a computed sweep record with hit == 0, and every other
 * pair is evaluated by the sweep rule itself.
 *
 *   a, b, d_a_dx, d_a_dy, d_b_dx, d_b_dy, row_base, col_base, flags, d_out : as c2d_poly_set_casts (flags: 0 or C2D_CAST_SKIP_SELF;
 *                d_out: c2d_cast[n_a], 8-byte aligned).  Records at or beyond n_a are never touched.  a and b may describe the same
 *                memory (same pointers, n, stride, rows, d_k AND the same motion planes): the boxes and the sort are then made once.
 *                One set against itself with different motion planes is two sets.
 *
 * The arguments are checked in the order of c2d_poly_set_casts, half a motion first.  n_a == 0 is a no-op; n_b == 0 writes the miss
 * record (BAD_PAIR for a bad query) for every query without touching the ctx scratch.  NULL arguments, `rows` out of range, misaligned
 * planes or motion planes, a d_out that is not 8-byte aligned, stride < n, unknown flag bits, half a motion, n_a or n_b above 2^32 and
 * row_base + n_a or col_base + n_b above 2^32 are refused (C2D_ERR_INVALID_ARG) before a device is touched.
 *
 * The candidates are found as c2d_poly_sweep_broad_pairs finds them (the same swept boxes, grid and sort; polygons it calls wild —
 * among them a mover whose swept box is far wider than the scene's typical one — are compared with everything).  The cost follows
 * the candidates, not n_b: a scene in which many polygons move many polygon sizes per step has many candidates per query and belongs
 * to c2d_poly_set_casts or to shorter steps.  Asynchronous on `stream`, with no host synchronisation;
 * deterministic: two runs give the same bytes.  It works through the ctx scratch under the workspace guard, which it grows on first
 * use and keeps; the size is that of c2d_poly_sweep_broad_pairs and depends only on (n_a, n_b, same memory).  Graph capture follows
 * c2d_sat_poly_broad_pairs: allowed after an eager call of the same or a larger size, refused (C2D_ERR_INVALID_ARG) before anything
 * is enqueued if the scratch would have to grow. */
int c2d_poly_set_casts_grid(c2d_ctx* ctx, const c2d_poly_set* a, const c2d_poly_set* b,
                            const float* d_a_dx, const float* d_a_dy, const float* d_b_dx, const float* d_b_dy,
                            size_t row_base, size_t col_base, int flags,   /* 0 or C2D_CAST_SKIP_SELF */
                            c2d_cast* d_out, c2d_stream stream);

/* The counters of the last c2d_poly_set_casts_grid call with n_b > 0 on this ctx, for measurements (csrc/tools/cast_grid_bench.py):
 * synchronise the call's stream first; the read blocks.  Refused when no such call has run, or when another call has used the ctx
 * scratch since (the last grid call on the ctx was not a grid cast).  out[0] = queries answered by the list kernel (wild ones, and
 * walks past the candidate cap), out[1] = sorted grid entries the walks looked at, out[2] = candidates (entries whose box meets the
 * query's, wild polygons, and what the list kernel's box filter let through), out[3] = of those, the pairs that ran the axis walk (the
 * others could not beat a best at time 0 with a smaller index), out[4] = 0 (reserved). */
int c2d_poly_set_casts_grid_stats(c2d_ctx* ctx, unsigned long long out[5]);

/* ---- binned polygon batches ---------------------------------------------------
 * The padded layout above moves 16 vertex rows per polygon whatever the polygons are: with
 * K ~ U{3..16} that is 259 bytes per pair for 155 bytes of real vertices, and no kernel can
 * avoid it — the pairs of a wave have unrelated counts, so every 64-byte segment of every row
 * holds a vertex somebody needs.  A caller that keeps its pairs in BINS — pairs grouped by the
 * size of their polygons, each bin a tight plane layout of its own — hands over the exact
 * bytes instead, and the bin's row counts are known before any count byte has been read:
 *
 *   bin:  rows_a, rows_b        vertex rows of polygon A / B in this bin, 1..C2D_POLY_KMAX
 *         n                     pairs in the bin (any number, < 2^32; every vertex plane — rows x stride
 *                               floats — must stay below 4 GiB: split larger bins)
 *         stride                elements between the vertex rows of a plane (0 = n; a multiple of 64
 *                               with 256-byte aligned planes keeps every row segment aligned)
 *         d_ax, d_ay            f32[rows_a][stride]  polygon A's vertices, pair index fastest
 *         d_bx, d_by            f32[rows_b][stride]  polygon B's
 *         d_ka, d_kb            u8[n] vertex counts 1..rows_a / 1..rows_b, or NULL = every
 *                               polygon of the bin has exactly rows_a / rows_b vertices
 *         d_out                 u8[n] results
 *
 * Same arithmetic and the same results as c2d_sat_poly_pairs for the same polygons (true normals,
 * unfused projections, strict <; SAT is symmetric in A and B, so a producer may swap the two
 * polygons of a pair to halve the number of bins).  Any number of bins (up to 65535), any
 * mix of row counts; ONE launch covers all of them.
 *
 *   c2d_poly_bins_create   validates the descriptors and uploads the launch table (synchronous;
 *                          the buffers stay the caller's and may be refilled between tests: the
 *                          table holds pointers and sizes, not data);
 *   c2d_sat_poly_pairs_binned   tests every pair of every bin: asynchronous on `stream`,
 *                          graph-capturable; vertex counts are checked on the device as for
 *                          c2d_sat_poly_pairs (pair reads 0, error at the next synchronise);
 *   c2d_poly_bins_from_padded   bins a padded batch (the layout of c2d_sat_poly_pairs_rows) on the
 *                          device: polygon sizes are rounded up to a multiple of `granularity`
 *                          rows (1 = one bin per (ka, kb), no padding at all; 4 = at most 16 bins),
 *                          the bins live in ONE device block owned by the handle.  This moves
 *                          every vertex once (about 1.3 ms per 1e7 pairs, what eight tests save against the padded layout;
 *                          profiles/notes_r04_bin_move.md): it pays when the
 *                          batch is tested more than once or as a converter for stored datasets;
 *                          a producer that can write bins directly should.  Synchronous; a vertex
 *                          count outside 1..rows is refused (C2D_ERR_INVALID_ARG, no handle).
 *                          Every n up to 2^32 - 65 is accepted: a size class whose vertex plane would
 *                          reach 4 GiB becomes several bins of 2^k pairs (the last one the rest), so
 *                          c2d_poly_bins_size / _get show it as consecutive bins with planes below
 *                          4 GiB.  (The 4 GiB rule of c2d_poly_bins_create is the caller's.)
 *   c2d_poly_bins_results  for a handle made by c2d_poly_bins_from_padded: the results in the
 *                          ORDER OF THE PADDED INPUT, u8[n] (asynchronous on `stream`);
 *   c2d_poly_bins_get      descriptor i of the handle (device pointers), for inspection: bin i of
 *                          c2d_poly_bins_create is the caller's bin i (a bin with n = 0 stays in the list and
 *                          takes no work). */
typedef struct c2d_poly_bin {
    uint32_t rows_a, rows_b;
    size_t n;
    size_t stride;   /* elements between consecutive vertex rows of a plane, >= n; 0 = n */
    const float* d_ax;
    const float* d_ay;
    const float* d_bx;
    const float* d_by;
    const uint8_t* d_ka;
    const uint8_t* d_kb;
    uint8_t* d_out;
} c2d_poly_bin;
typedef struct c2d_poly_bins c2d_poly_bins;
int c2d_poly_bins_create(c2d_ctx* ctx, const c2d_poly_bin* bins, size_t n_bins, c2d_poly_bins** out);
int c2d_poly_bins_from_padded(c2d_ctx* ctx, const float* d_vx, const float* d_vy, const uint8_t* d_k, size_t n,
                              int rows, int granularity, c2d_poly_bins** out, c2d_stream stream);
int c2d_poly_bins_destroy(c2d_ctx* ctx, c2d_poly_bins* bins);
size_t c2d_poly_bins_size(const c2d_poly_bins* bins);   /* number of bins  */
size_t c2d_poly_bins_pairs(const c2d_poly_bins* bins);  /* pairs in total  */
size_t c2d_poly_bins_bytes(const c2d_poly_bins* bins);  /* bytes one test moves: vertices, counts, results */
int c2d_poly_bins_get(const c2d_poly_bins* bins, size_t i, c2d_poly_bin* out);
int c2d_sat_poly_pairs_binned(c2d_ctx* ctx, const c2d_poly_bins* bins, unsigned long long* d_count,
                              c2d_stream stream);
int c2d_poly_bins_results(c2d_ctx* ctx, const c2d_poly_bins* bins, uint8_t* d_out, c2d_stream stream);

/* ---- random stream -----------------------------------------------------------
 * Replaces setup_kernel + curand_normal (utils.cu:111-117, :146-150).  The
 * generator is counter based: Philox4x32-10 with key = seed and subsequence =
 * scene_id — rocRAND's rocrand_state_philox4x32_10 engine.  No state array, no
 * set-up kernel, results independent of launch geometry and of how samples are
 * sharded over GPUs.
 *
 * Draw layout.  The samples of a stream are drawn in groups of four: sample s is
 * member j = s & 3 of group g = s >> 2, which owns blocks 8g .. 8g+5 of the
 * subsequence (rocRAND: rocrand_init(seed, scene_id, offset = 4 * (8g + b))):
 *   block 8g+0, word j                  radius word of the first Box-Muller pair (dx, dy)
 *   block 8g+1, word j                  angle word of that pair
 *   block 8g+2+(j>>1), words 2(j&1)..   radius, angle word of the second pair (dtheta, dw)
 *   block 8g+4+(j>>1), words 2(j&1)..   third pair (dh; its second normal is unused)
 * The draw ORDER per sample is the reference's (dx, dy, dtheta, dw, dh).  Grouping
 * the four radius words of four samples in one block is what lets the kernels
 * prove "certain miss" for most samples of a far scene at a quarter of a Philox
 * block per sample.
 *
 * c2d_philox_normals (parity/debug): for samples sample_begin .. +n writes the
 * five N(0,1) draws in the reference's order dx,dy,dtheta,dw,dh
 * (utils.cu:146-150) to d_normals[n][5] and, if d_raw != NULL, the six raw
 * 32-bit words in draw order to d_raw[n][6]. */
int c2d_philox_normals(c2d_ctx* ctx, uint64_t seed, uint64_t scene_id, uint64_t sample_begin,
                       size_t n, float* d_normals, uint32_t* d_raw, c2d_stream stream);

/* c2d_math_eval (parity/debug): evaluates one canonical math function of the
 * arithmetic contract on n inputs given as raw 32-bit patterns, so that tests
 * can compare the device implementation with the oracle bit for bit.
 *   C2D_MATH_LOG        out0 = log(x)                 x = float(bits) > 0, normal
 *   C2D_MATH_SINCOS     out0, out1 = sin(x), cos(x)   stands in for utils.cu:133-134
 *   C2D_MATH_SINCOS_U32 out0, out1 = sin, cos of 2*pi*bits/2^32
 *   C2D_MATH_SQRT       out0 = correctly rounded sqrt(x), x in {+-0} U [2^-96, 2^96]
 *   C2D_MATH_BOX_MULLER out0, out1 = the two normals of words (bits, ~bits * 2654435761) */
#define C2D_MATH_LOG 0
#define C2D_MATH_SINCOS 1
#define C2D_MATH_SINCOS_U32 2
#define C2D_MATH_SQRT 3
#define C2D_MATH_BOX_MULLER 4
int c2d_math_eval(c2d_ctx* ctx, int fn, const uint32_t* d_in_bits, size_t n, float* d_out0,
                  float* d_out1, c2d_stream stream);

/* ---- Monte-Carlo collision probability ---------------------------------------
 *
 * c2d_mc_pair: one scene, sample-parallel.  Replaces the body of
 * monte_carlo_sample_collision_dataset_uniform for a single data point
 * (compute_collision_probability.cu:119-139): robot = create_rect(robot_w,
 * robot_h) rotated by pose->theta and moved to pos (:132-133); obstacle =
 * create_rect(pose->width, pose->height) (:128); each sample perturbs the
 * obstacle with sample_rectangle (utils.cu:144-157) and tests it with
 * convex_collide (utils.cu:159-184).  Samples sample_begin .. sample_begin +
 * n_samples - 1 of stream (seed, scene_id) are evaluated; *d_hits (device
 * uint64) is incremented by the number of colliding samples.  Disjoint sample
 * ranges may run on different GPUs and be summed. */
int c2d_mc_pair(c2d_ctx* ctx, float robot_w, float robot_h, const Position* pos, const Pose* pose,
                const StdDev* std_dev, uint64_t seed, uint64_t scene_id, uint64_t sample_begin,
                uint64_t n_samples, unsigned long long* d_hits, c2d_stream stream);

/* c2d_mc_scenes: many scenes with the reference's adaptive stopping rule.
 * Replaces the host loop + kernel + thrust compaction of
 * compute_collision_probability.cu:276-332 (= generate_dataset.cu:420-479):
 * every scene is sampled in batches (C2D_MC_* schedule above); after each
 * batch the 95 % half-width calcSlack (utils.cu:186-196, with the int
 * overflow D1 fixed) is compared with bin_accuracy[getBin(p)]
 * (utils.cu:198-207, with the out-of-bounds read D2 fixed); a scene stops at
 * the first check that passes, or when n_samples >= max_samples.
 * Scene i uses random stream (seed, scene_id_base + i), so results do not
 * depend on batching, completion order or the number of GPUs.
 * The whole loop is enqueued on `stream` without any read-back (the schedule
 * state lives on the device); the call only synchronises when a host output
 * (total_samples, iterations) is requested.  Every step of the schedule — until
 * n_samples >= max_samples — is enqueued, 2 launches per step; steps after the last
 * scene finished retire at once (~5 us).  Schedules of more than 100 000 steps are
 * refused (C2D_ERR_INVALID_ARG): use larger batches.  With a host output requested the
 * call looks at the device state every 64 steps and stops enqueuing once no scene is left. */
typedef struct c2d_mc_scenes_args {
    const Pose* d_poses;          /* device Pose[num_poses]          (utils.cu:91-94)  */
    uint32_t num_poses;
    const StdDev* d_std_devs;     /* device StdDev[num_std_devs] — standard deviations,
                                     i.e. sqrt of variances.npy (ccp.cu:188-194)       */
    uint32_t num_std_devs;
    const PositionWithVarAndPoseIdx* d_scenes; /* device rows (x,y,var_idx,pose_idx)  */
    size_t n_scenes;
    float robot_w, robot_h;       /* ccp.cu:39-40 defaults 4.07 x 1.74                 */
    const float* accuracy_bins;   /* host f32[n_accuracy_bins], e.g. {0,.01,.1,1}      */
    const float* bin_accuracy;    /* host f32[n_accuracy_bins-1], e.g. {1e-4,1e-3,1e-2} */
    uint32_t n_accuracy_bins;     /* <= 16                                             */
    uint32_t max_samples;         /* ccp.cu:38 default 4000000                         */
    uint64_t seed;
    uint64_t scene_id_base;
    /* Sampling schedule; all three 0 = the reference default (C2D_MC_* above).  ztest.cu
     * uses a constant batch of 10000 (ztest.cu:332-339): small = large = 10000. */
    uint32_t schedule_small_batch;  /* batch size while n_samples < schedule_switch_at   */
    uint32_t schedule_large_batch;  /* batch size afterwards                             */
    uint32_t schedule_switch_at;
    uint32_t* d_hits;             /* device u32[n_scenes]  out: colliding samples      */
    uint32_t* d_n_used;           /* device u32[n_scenes]  out: samples drawn          */
    PoseCPVarAndPoseIdx* d_rows;  /* optional device rows (x,y,cp,var_idx,pose_idx) =
                                     one output .npy row each (ccp.cu:337-344), cp =
                                     hits / n_used (utils.cu:210-215)                  */
    uint64_t* total_samples;      /* optional host out: sum of n_used                  */
    uint32_t* iterations;         /* optional host out: schedule steps executed        */
} c2d_mc_scenes_args;

int c2d_mc_scenes(c2d_ctx* ctx, const c2d_mc_scenes_args* args, c2d_stream stream);

/* c2d_sample_scenes: draws the scenes themselves, replacing the iteration==0
 * branch of the generate_dataset kernel (generate_dataset.cu:207-219):
 * pose_idx and var_idx uniform over the tables, robot placed on a ring around
 * the obstacle (formula SURVEY.md §5.6).  Scene i uses stream
 * (seed, scene_id_base + i) in a key domain disjoint from the MC samples. */
int c2d_sample_scenes(c2d_ctx* ctx, const Pose* d_poses, uint32_t num_poses,
                      const StdDev* d_std_devs, uint32_t num_std_devs, float robot_w,
                      float robot_h, float spread, uint64_t seed, uint64_t scene_id_base,
                      size_t n_scenes, PositionWithVarAndPoseIdx* d_scenes, c2d_stream stream);

/* ---- Monte-Carlo collision probability for convex polygons -----------------------
 * The reference's README (README.md:3) says its code "can easily be extended to handle arbitrary
 * convex 2D shapes"; its own functions stop at rectangles (sample_rectangle utils.cu:144-157,
 * convex_collide utils.cu:159-184).  These two entry points are that extension of c2d_mc_pair /
 * c2d_mc_scenes, with the same random stream, draw order, sample sharding and stopping rule.
 * STATUS: c2d_mc_poly_* goes beyond the reference — the semantics below (notably "dw, dh scale the
 * obstacle frame") are this build's own generalisation, pinned only by this build's own oracle and by
 * the rectangle case; no reference code or fixture stands behind them.  They are an extension OUTSIDE
 * BASELINE.json's configs (none of the five names a polygon Monte-Carlo), frozen as of round 5: kept
 * working and tested, not developed further.
 *
 *   robot     a polygon in its own frame, rotated by theta and moved to pos with the arithmetic of
 *             rot_trans_rectangle (utils.cu:132-142; ccp.cu:132-133);
 *   obstacle  a polygon about the origin (ccp.cu:128).  A sample draws the five normals of
 *             utils.cu:146-150 in that order and applies them as sample_rectangle does: dw, dh change
 *             the SHAPE first — the obstacle frame's x / y coordinates are scaled by (1 + dw), (1 + dh),
 *             so StdDev.width / .height are RELATIVE standard deviations here (a w x h rectangle given
 *             as a 4-gon with sigma_w / w, sigma_h / h has the distribution of the reference's sample,
 *             utils.cu:152-155) — then the shape is rotated by dtheta about the origin and moved by
 *             (dx, dy) (utils.cu:156);
 *   test      the projection / strict-< interval test of utils.cu:172-180 on the true normals of all
 *             ka + kb edges, exactly as c2d_sat_poly_pairs.
 *
 * With sigma_w = sigma_h = 0 a rectangle given as a 4-gon gets, sample for sample, the very vertices
 * c2d_mc_pair gives it; the two tests then differ only in the scale of their axes (edge vector there,
 * normal here), which can move a boolean only for a sample within an ulp of touching.
 * Vertex order may be clockwise or counter-clockwise; 1 <= k <= C2D_POLY_KMAX (k = 1, 2: a point, a
 * segment).  The certain-miss shortcuts and the fast evaluation require finite parameters small enough
 * for no intermediate to overflow or to turn denormal: vertices, position, sigma_x, sigma_y zero or
 * between 1e-15 and 1e8 in magnitude, the
 * relative deviations sigma_w, sigma_h below 1e4 (a scale factor multiplies every coordinate), angles
 * below 1e15; outside that domain every sample is evaluated in full with the all-bit-patterns test and
 * the hit counts still equal the oracle's. */
typedef struct c2d_polygon {
    uint32_t k;                   /* vertices used */
    float x[C2D_POLY_KMAX];
    float y[C2D_POLY_KMAX];
} c2d_polygon;

/* c2d_mc_poly_pair: one polygon scene, sample-parallel (c2d_mc_pair's contract: samples sample_begin ..
 * sample_begin + n_samples - 1 of stream (seed, scene_id); *d_hits is incremented).  robot, obstacle,
 * pos and std_dev are host pointers read before the call returns. */
int c2d_mc_poly_pair(c2d_ctx* ctx, const c2d_polygon* robot, const Position* pos, float robot_theta,
                     const c2d_polygon* obstacle, const StdDev* std_dev, uint64_t seed, uint64_t scene_id,
                     uint64_t sample_begin, uint64_t n_samples, unsigned long long* d_hits, c2d_stream stream);

/* One entry of the polygon scene table: what Pose {width, height, theta} (utils.cu:91-94) is to the
 * rectangle dataset — the robot's rotation in the scene and the obstacle's shape. */
typedef struct c2d_poly_pose {
    float theta;
    c2d_polygon obstacle;
} c2d_poly_pose;

/* c2d_mc_poly_scenes: c2d_mc_scenes for polygon scenes.  `base` carries the scenes, tables of standard
 * deviations, schedule, stop rule, seeds and outputs exactly as for c2d_mc_scenes; its d_poses, num_poses,
 * robot_w and robot_h are ignored and replaced by d_poly_poses / num_poly_poses (device table indexed by
 * the rows' pose_idx) and the robot polygon (host pointer).  A vertex count outside 1..C2D_POLY_KMAX in the
 * device table is clamped and reported by the next c2d_stream_synchronize / c2d_ctx_check_async. */
typedef struct c2d_mc_poly_scenes_args {
    c2d_mc_scenes_args base;
    const c2d_polygon* robot;            /* host */
    const c2d_poly_pose* d_poly_poses;   /* device c2d_poly_pose[num_poly_poses] */
    uint32_t num_poly_poses;
} c2d_mc_poly_scenes_args;
int c2d_mc_poly_scenes(c2d_ctx* ctx, const c2d_mc_poly_scenes_args* args, c2d_stream stream);

/* ---- the dataset's tables -------------------------------------------------------
 * c2d_uniform_table_minstd: the table fill of generate_dataset.cu:279-332 on the device.  The reference
 * draws its variance and pose tables on the host from ONE std::default_random_engine (minstd_rand0,
 * default seed), row by row, dimension d uniform in [lo[d], hi[d]) through
 * std::uniform_real_distribution<float>, and uploads them; this writes d_out[rows][dims] with exactly those
 * floats (libstdc++'s: one engine call per float, value = float(x - 1) * 2^-31 * (hi - lo) + lo), engine
 * calls first_draw .. first_draw + rows * dims - 1 of that engine — the variances first (first_draw = 0),
 * then the poses (first_draw = 5 * num_variances), as the reference.  lo, hi: host float[dims], dims <= 8.
 * c2d_sqrt_f32: element-wise correctly rounded square root, d_out[i] = sqrt(d_in[i]) — the standard
 * deviations of the variance table (generate_dataset.cu:309-317, compute_collision_probability.cu:188-194). */
int c2d_uniform_table_minstd(c2d_ctx* ctx, float* d_out, size_t rows, int dims, const float* lo, const float* hi,
                             uint64_t first_draw, c2d_stream stream);
int c2d_sqrt_f32(c2d_ctx* ctx, const float* d_in, float* d_out, size_t n, c2d_stream stream);

/* ---- multi-GPU aggregation ----------------------------------------------------
 * New work (the reference is single-GPU, compute_collision_probability.cu:212-251): pairs,
 * scenes and Monte-Carlo sample ranges shard over the GPUs of a node with no exchange on
 * the data path (random streams are keyed by scene id and sample index, so the union of
 * the shards is bit-identical to a one-GPU run), and ONE sum-reduction of the 64-bit hit /
 * sample / histogram counters closes a run.  One process per GPU; the reduction is
 * ncclAllReduce(uint64, sum) of RCCL over xGMI, loaded (dlopen librccl.so.1) at the first
 * c2d_dist_* call only.
 *
 *   c2d_dist_unique_id : rank 0 creates the 128-byte communicator id (ncclGetUniqueId) and
 *                        hands it to the other ranks by any channel it has;
 *   c2d_dist_init      : collective over all ranks (ncclCommInitRank) on the ctx's device;
 *   c2d_dist_init_file : the same with the id exchanged through `path`: rank 0 writes the
 *                        file atomically, the others wait up to timeout_s seconds for it;
 *                        `path` must not exist beforehand (use a fresh name per run) and is
 *                        removed again once every rank has joined;
 *   c2d_dist_all_reduce_sum_u64 / c2d_dist_broadcast_u64 : in place on device words,
 *                        asynchronous on `stream` like every other entry point;
 *   c2d_dist_barrier   : a one-word all-reduce followed by a stream synchronise.
 *
 * c2d_dist_init, c2d_dist_barrier (hence c2d_dist_init_file) and c2d_dist_stream_synchronize run
 * under a watchdog: if the peers do not arrive within the time limit (timeout_s of
 * c2d_dist_init_file, 0 = the default; $C2D_DIST_TIMEOUT_S or 300 s otherwise) they return
 * C2D_ERR_DIST instead of blocking for ever.  A helper thread is then left inside RCCL / HIP:
 * c2d_dist_timed_out() says so, the communicator refuses further use, c2d_dist_destroy leaves it
 * alone, and the process should report the error and end with _exit() — the runtime's teardown in
 * a normal exit() would race that thread (the drivers do exactly this).
 * c2d_dist_all_reduce_sum_u64 / c2d_dist_broadcast_u64 only ENQUEUE; a caller that waits for them
 * with c2d_stream_synchronize blocks for ever if a peer died after the communicator was built —
 * c2d_dist_stream_synchronize is the same wait under the watchdog.
 *
 * c2d_dist_transport() names the transport: "rccl" — the only one this library contains.  A
 * separate test build (lib-rehearsal/libc2d.so, `make lib-rehearsal`) replaces it by a sum
 * through small files, which lets several ranks share one device (RCCL refuses that) so that
 * the N > 1 host logic can be rehearsed on a one-GPU box; it reports "file (rehearsal)". */
#define C2D_DIST_ID_BYTES 128
typedef struct c2d_dist c2d_dist;
int c2d_dist_unique_id(void* id_out /* [C2D_DIST_ID_BYTES] */);
int c2d_dist_init(c2d_ctx* ctx, int rank, int world_size, const void* id, c2d_dist** out);
int c2d_dist_init_file(c2d_ctx* ctx, int rank, int world_size, const char* path, double timeout_s,
                       c2d_dist** out);
int c2d_dist_rank(const c2d_dist* dist);
int c2d_dist_world_size(const c2d_dist* dist); /* as counted by RCCL (ncclCommCount) */
const char* c2d_dist_transport(const c2d_dist* dist);
/* Which RCCL sums the counters: ncclGetVersion's code (22203 = 2.22.3) and the file the library was loaded from (dladdr;
 * "" if unknown), so that a scaling record can be read without the logs.  Loads librccl if no c2d_dist_* call has yet.
 * Inside a process that already holds a librccl.so.1 — PyTorch ships its own — the loader hands back THAT one (same
 * soname), otherwise /opt/rocm's; both are plain RCCL and nothing else is ever used.  The rehearsal build reports
 * version 0 and "file (rehearsal)". */
int c2d_dist_rccl_version(int* version, char* path_out, size_t path_bytes);
int c2d_dist_all_reduce_sum_u64(c2d_dist* dist, unsigned long long* d_buf, size_t count,
                                c2d_stream stream);
int c2d_dist_broadcast_u64(c2d_dist* dist, unsigned long long* d_buf, size_t count, int root,
                           c2d_stream stream);
int c2d_dist_barrier(c2d_dist* dist, c2d_stream stream);
int c2d_dist_stream_synchronize(c2d_dist* dist, c2d_stream stream);
int c2d_dist_timed_out(const c2d_dist* dist); /* 1 after a watchdog time-out on this communicator */
int c2d_dist_destroy(c2d_dist* dist);

/* Host-side helpers with the reference's semantics, exported so that callers
 * and tests see exactly what the device evaluates (utils.cu:186-207). */
float c2d_calc_slack(uint32_t n_samples, uint32_t n_true);
int c2d_get_bin(float p, const float* accuracy_bins, uint32_t n_accuracy_bins);

#ifdef __cplusplus
}
#endif

#endif /* C2D_H_ */
