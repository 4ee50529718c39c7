"""A Python mirror of the layout c2d_poly_bins_from_padded gives its device block (csrc/c2d_poly_binned.hip, "2. layout of the
block"): which bins a padded batch becomes, where each bin's planes lie in the block, and how large the block is.  The tests
compare it with the handle's descriptors (c2d_poly_bins_get) and use it to place a batch on a chosen side of a size limit.
TEST INFRASTRUCTURE."""
import numpy as np

PLANE_MAX = 2**32 - 1          # C2D_FROM_PADDED_PLANE_MAX of the product build
SPLITCHECK_PLANE_MAX = 32768   # ... of make lib-splitcheck
BIN_DESC_BYTES = 72            # sizeof(BinDesc)


def _align(v, a):
    return (v + a - 1) // a * a


def class_histogram(k, rows, g):
    """pairs per class, {class: pairs}, of a padded batch's counts k (uint8 [2][n]); counts outside 1..rows are left out"""
    ka, kb = k[0].astype(np.int64), k[1].astype(np.int64)
    ok = (ka >= 1) & (ka <= rows) & (kb >= 1) & (kb <= rows)
    cls = ((ka[ok] + g - 1) // g - 1) * 16 + ((kb[ok] + g - 1) // g - 1)
    vals, cnts = np.unique(cls, return_counts=True)
    return {int(c): int(m) for c, m in zip(vals, cnts)}


def split_lg(rows, plane_max=PLANE_MAX):
    lg = 6
    while rows * (2 << lg) * 4 <= plane_max:
        lg += 1
    return lg


def from_padded_layout(hist, n, rows, g, plane_max=PLANE_MAX):
    """-> (bins, block_bytes).  bins: in the handle's order, dicts rows_a, rows_b, n, stride and the byte offsets ax, ay, bx, by
    of the bin's planes in the block (ka, kb too when the bins are counted); n = pairs of the input, bad ones included."""
    counted = g > 1
    bins, nbytes, pairs = [], 0, 0
    for c in sorted(hist):
        n_c = hist[c]
        if not n_c:
            continue
        ra, rb = min(rows, (c // 16 + 1) * g), min(rows, (c % 16 + 1) * g)
        cap = n_c
        if max(ra, rb) * _align(n_c, 64) * 4 > plane_max:
            cap = 1 << split_lg(max(ra, rb), plane_max)
        subs = [min(cap, n_c - j) for j in range(0, n_c, cap)]
        strides = [_align(m, 64) for m in subs]
        elems = sum(strides)
        off = {}
        for name, r in (("ax", ra), ("ay", ra), ("bx", rb), ("by", rb)):
            off[name] = nbytes
            nbytes = _align(nbytes + r * elems * 4, 256)
        if counted:
            for name in ("ka", "kb"):
                off[name] = nbytes
                nbytes = _align(nbytes + n_c, 256)
        for m, st in zip(subs, strides):
            bins.append(dict(rows_a=ra, rows_b=rb, n=m, stride=st, **off))
            for name, r in (("ax", ra), ("ay", ra), ("bx", rb), ("by", rb)):
                off[name] += r * st * 4
            if counted:
                off["ka"] += m
                off["kb"] += m
        pairs += n_c
    nbytes = _align(nbytes + pairs, 256)             # results
    nbytes += 4 * n                                  # index
    nbytes = _align(nbytes, 256) + (len(bins) + 1) * 4   # pair bases
    nbytes = _align(nbytes, 256) + 256 * 2           # class -> bin
    tiles = sum((b["n"] + 63) // 64 for b in bins)
    nbytes = _align(nbytes, 256) + _align(len(bins) * BIN_DESC_BYTES, 256) + 4 * tiles   # launch table, tile list
    return bins, nbytes


def assert_handle_matches(handle, bins):
    """the handle's descriptors are the mirror's bins: same shapes, and planes at the same offsets from bin 0's ax plane"""
    assert len(handle) == len(bins), (len(handle), len(bins))
    base = handle.get(0)["ax"] if bins else 0
    for i, want in enumerate(bins):
        got = handle.get(i)
        for key in ("rows_a", "rows_b", "n", "stride"):
            assert got[key] == want[key], (i, key, got[key], want[key])
        for key in ("ax", "ay", "bx", "by", "ka", "kb"):
            if key in want:
                assert got[key] - base == want[key], (i, key, got[key] - base, want[key])
