// c2d_grid_best.hpp — the best-key queries through the grid of the pair searches, as one frame over a query policy.
//
// For every object A_i of a set, the smallest key over the objects B_j of a set that the query considers: the reduction of an N x M
// call, found through the boxes, the grid and the sorted keys of c2d_broad.hpp instead of a visit to every B_j.  The frame holds the
// walk, the list pass, the counters and the launch sequence; a query policy P supplies what differs between the queries:
//   P::Shape                            the box policy of the pipeline (broad_box_kernel<P::Shape>; its Set holds P::Set as `set`)
//   P::Set, P::Obj, P::load(set, i, o)  the device-side description of one set, one object in registers, object i of the set
//   P::size(set)                        the objects of the set (host and device)
//   P::Aux, P::aux(obj)                 what the per-pair step wants of a query object beyond the object, made once per query
//   P::Params                           what it wants of the call (may be empty)
//   P::Out                              the output record; a row's key goes to its first eight bytes
//   P::kCounters, P::kMagic, P::kNoKey  counters per call (0: walked, 1: met, from 2: the policy's own), the word that marks them in
//                                       the scene header, and the key of "nothing"
//   P::pair(a, aux, b, params, gj, best, count)
//                                       the per-pair step for the candidate with global index gj: best = min(best, the pair's key)
//                                       when the pair is considered, in ANY order of the candidates (the walk visits B in cell-key
//                                       order, the tail and the list in index order); it counts itself in count.n[kGridBestMet]
// The pipeline of one call, on the caller's stream, through the ctx scratch of the pair searches:
//   1. boxes      broad_box_kernel<P::Shape> on both sets (once when they are the same)      } broad_prepare
//   2. grid, sort broad_grid_and_sort, unchanged: a box over more than two cells becomes wild }
//   3. counters   grid_best_begin_kernel: the counters of this call, in the scene header's extent histogram (dead by now)
//   4. rows       grid_best_row_kernel, one query per lane: the cell walk of broad_row_query (the same cell range, boxes_meet on the
//                 sorted boxes, then the wild tail) with a running best key instead of a count.  A wild query, and one whose walk
//                 would pass kCandidateCap sorted entries, goes to a list; an absent one keeps "nothing" (the caller's last pass
//                 writes its BAD_PAIR record).  Every other query's key goes to the first eight bytes of its record.
//   5. list       grid_best_list_kernel, one listed query per wave over all of B in index order: the box filter where both are
//                 regular, the same per-pair step, a wave minimum of the key, one store.
// A row has one owner in every pass: there are no atomics on the records.  The caller initialises nothing (every row is written in 4
// or 5) and turns the keys into records behind 5.
//
// The kernel argument keeps the members and the order that each query's own struct had before the frame, with the set sizes read
// through P::size and an empty P::Params taking no room: the instances' machine code is that of the kernels they replace
// (profiles/grid_best_refactor_isa.txt).
#pragma once

#include <cstring>

#include "c2d_broad.hpp"

namespace c2d {

enum { kGridBestWalked = 0, kGridBestMet = 1 };   // the frame's own counters; a policy's follow

// The counters of one call live in the scene header's extent histogram, which is dead once the cell size has been picked (as
// c2d_ray_grid.hip's do).  n[0]: sorted entries the row kernel's walks looked at (the aborted walks of listed queries included);
// n[1]: candidates: entries whose box meets the query's, the wild tail, and what the list kernel's filter let through.
template <int N>
struct GridBestStats {
    unsigned long long n[N];
    unsigned int magic;
    unsigned int pad_;
};

template <int N>
struct GridBestCount {
    uint32_t n[N] = {};   // per lane and launch: a lane sees far fewer than 2^32 pairs (n_b <= 2^32 in all)
};

template <int N>
C2D_DEV GridBestStats<N>* grid_best_stats(BroadGrid* g)
{
    static_assert(sizeof(GridBestStats<N>) <= sizeof(unsigned int) * kHistBins && offsetof(BroadGrid, hist) == 0, "the counters sit at the start of the scene header");
    return reinterpret_cast<GridBestStats<N>*>(g->hist);
}

// a wave's counts into the header: one atomic per counter and wave
template <int N>
C2D_DEV void grid_best_count(BroadGrid* g, const GridBestCount<N>& c)
{
    unsigned long long v[N];
#pragma unroll
    for (int q = 0; q < N; q++) v[q] = c.n[q];
#pragma unroll
    for (int q = 0; q < N; q++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        GridBestStats<N>* st = grid_best_stats<N>(g);
#pragma unroll
        for (int q = 0; q < N; q++)
            if (v[q]) atomicAdd(&st->n[q], v[q]);
    }
}

// 3. the counters of this call
template <class P>
__global__ void grid_best_begin_kernel(BroadGrid* __restrict__ g)
{
    if (threadIdx.x != 0) return;
    GridBestStats<P::kCounters>* st = grid_best_stats<P::kCounters>(g);
#pragma unroll
    for (int q = P::kCounters - 1; q >= 0; q--) st->n[q] = 0ull;
    st->magic = P::kMagic;
    st->pad_ = 0u;
}

template <class P>
struct GridBestQuery {
    typename P::Set A, B;
    const float4* box_a;        // [n_a] the policy's boxes (NaN: wild or absent)
    const float4* box_b;        // [n_b], index order
    const uint32_t* keys;       // [n_b] sorted keys: regular ones first, then kWildKey, then kAbsentKey
    const uint32_t* idx;        // [n_b] index of each sorted key
    const float4* sbox;         // [n_b] boxes in key order
    BroadGrid* g;
    uint32_t* listed;           // [n_a] the queries left to the list kernel (g->n_long of them)
    size_t row_base, col_base;
    [[no_unique_address]] typename P::Params params;
    int skip_self;
};

// 4. one query per lane
template <class P>
__global__ __launch_bounds__(kBroadBlock) void grid_best_row_kernel(GridBestQuery<P> q, typename P::Out* __restrict__ out)
{
    constexpr size_t kStride = sizeof(typename P::Out) / 8;   // a record in 64-bit words
    BroadGrid* g = q.g;
    const size_t n_a = P::size(q.A), n_b = P::size(q.B);
    const uint32_t n_reg = g->n_reg_b;
    const uint32_t gx = g->gx, gy = g->gy;
    GridBestCount<P::kCounters> count;
    for (size_t i = (size_t)blockIdx.x * kBroadBlock + threadIdx.x; i < n_a; i += (size_t)gridDim.x * kBroadBlock) {
        const float4 ba = q.box_a[i];
        unsigned long long best = P::kNoKey;
        bool listed = box_wild(ba) && !box_absent(ba);
        if (!box_wild(ba)) {
            typename P::Obj a;
            P::load(q.A, i, a);
            const typename P::Aux aux = P::aux(a);
            const size_t gi = q.row_base + i;
            const BroadCells c = broad_cell_range(g, gx, gy, ba);
            uint32_t walked = 0;
#pragma unroll 1
            for (uint32_t cy = c.cy0; cy <= c.cy1 && !listed; cy++) {
                const uint32_t k_lo = cy * gx + c.cx0, k_hi = cy * gx + c.cx1;
#pragma unroll 1
                for (uint32_t k = lower_bound_u32(q.keys, n_reg, k_lo); k < n_reg && q.keys[k] <= k_hi; k++) {
                    if (++walked > kCandidateCap) {
                        listed = true;
                        break;
                    }
                    if (!boxes_meet(ba, q.sbox[k])) continue;
                    const uint32_t j = q.idx[k];
                    if ((size_t)j >= n_b) continue;   // (never: a sorted entry is an object of B)
                    if (q.skip_self && gi == q.col_base + j) continue;
                    typename P::Obj b;
                    P::load(q.B, j, b);
                    P::pair(a, aux, b, q.params, (uint32_t)(q.col_base + j), best, count);
                }
            }
            count.n[kGridBestWalked] += walked < kCandidateCap ? walked : kCandidateCap;
            if (!listed) {
#pragma unroll 1
                for (size_t k = n_reg; k < n_b && q.keys[k] != kAbsentKey; k++) {   // the wild tail ends where the absent objects begin
                    const uint32_t j = q.idx[k];
                    if ((size_t)j >= n_b) continue;
                    if (q.skip_self && gi == q.col_base + j) continue;
                    typename P::Obj b;
                    P::load(q.B, j, b);
                    P::pair(a, aux, b, q.params, (uint32_t)(q.col_base + j), best, count);
                }
            }
        }
        if (listed) {
            const unsigned int slot = atomicAdd(&g->n_long, 1u);   // each query at most once: slot < n_a
            if ((size_t)slot < n_a) q.listed[slot] = (uint32_t)i;
        } else {
            reinterpret_cast<unsigned long long*>(out)[kStride * i] = best;   // (an absent query: "nothing"; the last pass knows it is bad)
        }
    }
    grid_best_count(g, count);   // (every lane of the block arrives: the loop above has no early return)
}

// 5. the listed queries: one per wave over all of B's columns
template <class P>
__global__ __launch_bounds__(kBroadBlock) void grid_best_list_kernel(GridBestQuery<P> q, typename P::Out* __restrict__ out)
{
    constexpr size_t kStride = sizeof(typename P::Out) / 8;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_long = q.g->n_long;
    const size_t n_a = P::size(q.A), n_b = P::size(q.B);
    const size_t waves = (size_t)gridDim.x * (kBroadBlock / 64);
    GridBestCount<P::kCounters> count;
    for (size_t w = (size_t)blockIdx.x * (kBroadBlock / 64) + (threadIdx.x >> 6); w < n_long && w < n_a; w += waves) {
        const size_t i = q.listed[w];
        if (i >= n_a) continue;
        const float4 ba = q.box_a[i];
        typename P::Obj a;
        P::load(q.A, i, a);
        const typename P::Aux aux = P::aux(a);
        const size_t gi = q.row_base + i;
        unsigned long long best = P::kNoKey;
#pragma unroll 1
        for (size_t j = lane; j < n_b; j += 64) {
            const float4 bb = q.box_b[j];
            if (box_absent(bb)) continue;
            if (!box_wild(ba) && !box_wild(bb) && !boxes_meet(ba, bb)) continue;
            if (q.skip_self && gi == q.col_base + j) continue;
            typename P::Obj b;
            P::load(q.B, j, b);
            P::pair(a, aux, b, q.params, (uint32_t)(q.col_base + j), best, count);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {   // wave_min_u64, spelt out: through the helper the clearance instance's tail is scheduled anew
            const unsigned long long o = __shfl_down(best, off, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) reinterpret_cast<unsigned long long*>(out)[kStride * i] = best;
    }
    grid_best_count(q.g, count);
}

// Stages 1 to 5 of one call with n_b > 0.  The caller has checked its arguments, holds the DeviceGuard and owns `use` (armed here,
// broad_prepare): it queues its own last pass behind this and then calls use.done().
template <class P>
int grid_best_run(c2d_ctx* ctx, hipStream_t s, const char* what, const typename P::Shape::Set& A, const typename P::Shape::Set& B, bool same,
                  size_t row_base, size_t col_base, bool skip_self, const typename P::Params& params, typename P::Out* d_out, WorkspaceUse& use)
{
    const size_t n_a = P::size(A.set), n_b = P::size(B.set);
    BroadScratch W;
    if (int rc = broad_prepare<typename P::Shape>(ctx, s, what, A, n_a, B, n_b, same, W, use)) return rc;
    hipLaunchKernelGGL(grid_best_begin_kernel<P>, dim3(1), dim3(64), 0, s, W.g);
    C2D_LAUNCH_CHECK(ctx);
    const GridBestQuery<P> q{A.set, B.set, W.box_a, W.box_b, W.keys, W.idx, W.sbox, W.g, W.long_rows, row_base, col_base, params, skip_self ? 1 : 0};
    hipLaunchKernelGGL(grid_best_row_kernel<P>, dim3(grid_for(n_a, kBroadBlock, 8192)), dim3(kBroadBlock), 0, s, q, d_out);
    C2D_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(grid_best_list_kernel<P>, dim3(kLongGrid), dim3(kBroadBlock), 0, s, q, d_out);
    C2D_LAUNCH_CHECK(ctx);
    return C2D_OK;
}

// The reader of a grid query's _stats entry point.  Such a query keeps its counters (Stats, with a `magic` word that names the query)
// at the start of the scene header, in the extent histogram, which is dead once the cell size has been picked.  A blocking copy of the
// header of the ctx scratch; `none_msg`: no scratch yet, `other_msg`: the header's counters are another query's.
template <class Stats>
int grid_stats_read(c2d_ctx* ctx, const char* what, const void* out, const char* none_msg, const char* other_msg, unsigned int magic, Stats& st,
                    unsigned int& n_long)
{
    if (!ctx) return C2D_ERR_INVALID_ARG;
    if (!out) return cross_fail(ctx, what, "NULL argument");
    if (!ctx->d_scratch || ctx->scratch_bytes < sizeof(BroadGrid)) return cross_fail(ctx, what, none_msg);
    DeviceGuard dg(ctx->device);
    static_assert(sizeof(BroadGrid) % 8 == 0, "copied as 64-bit words");
    unsigned long long raw[sizeof(BroadGrid) / 8];
    C2D_HIP(ctx, hipMemcpy(raw, ctx->d_scratch, sizeof(BroadGrid), hipMemcpyDeviceToHost));
    BroadGrid h;
    std::memcpy(&h, raw, sizeof h);
    std::memcpy(&st, h.hist, sizeof st);
    if (st.magic != magic) return cross_fail(ctx, what, other_msg);
    n_long = h.n_long;
    return C2D_OK;
}

}  // namespace c2d
