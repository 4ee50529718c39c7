// c2d_cross.hpp — the host front end shared by the N x M queries: the rectangle and polygon cross forms (c2d_cross.hip,
// c2d_poly_cross.hip: bit mask and pair list) and the two broad phases (c2d_broad.hip, c2d_poly_broad.hip: pair list).  The
// argument checks that every form states, once; the cut of a mask into launches; and the pair list behind any mask producer.
// Every check returns C2D_OK or the status to return, with the message "<entry point>: <why>" left in the ctx.
#pragma once

#include <cstdio>
#include <functional>

#include "c2d_cross_tiles.hpp"
#include "c2d_internal.hpp"

namespace c2d {

constexpr size_t kBaseLimit = (size_t)1 << 62;    // row_base + n_a, col_base + n_b stay far from signed overflow
constexpr size_t kIndexLimit = (size_t)1 << 32;   // the pair list's indices are u32

inline int cross_fail(c2d_ctx* ctx, const char* what, const char* why)
{
    char msg[256];
    std::snprintf(msg, sizeof msg, "%s: %s", what, why);
    return fail_arg(ctx, msg);
}

inline int cross_check_flags(c2d_ctx* ctx, const char* what, int flags)
{
    return (flags & ~C2D_CROSS_UPPER) ? cross_fail(ctx, what, "unknown flag") : C2D_OK;
}

// the flags, then the bases of the cross forms
inline int cross_check_flags_bases(c2d_ctx* ctx, const char* what, size_t n_a, size_t n_b, size_t row_base, size_t col_base, int flags)
{
    if (int rc = cross_check_flags(ctx, what, flags)) return rc;
    if (n_a > kBaseLimit || n_b > kBaseLimit || row_base > kBaseLimit - n_a || col_base > kBaseLimit - n_b)
        return cross_fail(ctx, what, "row_base + n_a and col_base + n_b must stay below 2^62");
    return C2D_OK;
}

// the bases of a per-row reduction, whose keys carry base + index as u32; refused with the entry point's own `beyond`
inline int cross_check_index_bases(c2d_ctx* ctx, const char* what, size_t n_a, size_t n_b, size_t row_base, size_t col_base, const char* beyond)
{
    if (n_a > kIndexLimit || row_base > kIndexLimit - n_a || n_b > kIndexLimit || col_base > kIndexLimit - n_b) return cross_fail(ctx, what, beyond);
    return C2D_OK;
}

// the output of a mask form: rows of ld_words 64-bit words, n_b columns
inline int cross_check_mask(c2d_ctx* ctx, const char* what, const unsigned long long* d_mask, size_t ld_words, size_t n_b)
{
    if (!d_mask) return cross_fail(ctx, what, "NULL mask");
    if (reinterpret_cast<uintptr_t>(d_mask) & 7u) return cross_fail(ctx, what, "the mask must be 8-byte aligned");
    if (ld_words < (n_b + 63) / 64) return cross_fail(ctx, what, "ld_words < ceil(n_b / 64)");
    return C2D_OK;
}

// The output of a list form.  end_a, end_b are one past the largest row and column index the list can hold (the cross forms:
// base + n; the broad forms: n), refused with `beyond` when either exceeds `limit`.
inline int cross_check_list(c2d_ctx* ctx, const char* what, const uint32_t* d_pairs, size_t capacity, const unsigned long long* d_count,
                            size_t end_a, size_t end_b, size_t limit, const char* beyond)
{
    if (!d_count) return cross_fail(ctx, what, "d_count is required");
    if (!d_pairs && capacity) return cross_fail(ctx, what, "NULL pair buffer");
    if (end_a > limit || end_b > limit) return cross_fail(ctx, what, beyond);
    return C2D_OK;
}

// The pair list behind an N x M bit mask (c2d_cross.hip): row passes of A through the ctx scratch, per pass the mask rows
// (`pass` queues the counting mask kernel of rows [r0, r0 + rows) into d_mask, row stride `words`), the row counts, the chunk scan
// with the running base on the device, and the emit.  Checks d_count / d_pairs / the u32 index limit (cross_check_list), grows the
// scratch (refused during graph capture).  The caller holds the DeviceGuard.  Shared by the rectangle and the polygon forms.
using CrossMaskPass = std::function<int(size_t r0, size_t rows, unsigned long long* d_mask, size_t words)>;
int cross_list_run(c2d_ctx* ctx, hipStream_t s, const char* what, size_t n_a, size_t n_b, size_t row_base, size_t col_base, uint32_t* d_pairs,
                   size_t capacity, unsigned long long* d_count, const CrossMaskPass& pass);

}  // namespace c2d
