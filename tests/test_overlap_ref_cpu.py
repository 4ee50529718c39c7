"""CPU tests that pin tests/overlap_ref.py — the numpy restatement of the overlap contract of include/c2d.h that the GPU tests compare
c2d_poly_pair_overlaps / c2d_rect_pair_overlaps with — on hand-computed cases on a 1/16 grid, where every operation of the rule is
exact in binary32 (tests/overlap_cases.py), and, for its accuracy, against a binary64 Sutherland-Hodgman clipper written here: another
algorithm (it builds the intersection polygon; the rule never does) in another precision: over random pairs, and over the families
of tests/overlap_cases.py in which edges of the two shapes lie on one line or nearly so."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_cases as oc  # noqa: E402
import overlap_ref as ref  # noqa: E402

F = np.float32
U = 2.0 ** -24
# The accuracy constants of DESIGN.md §5.27: four times the worst ratio measured over the inputs of accuracy_inputs() and over the
# families of tests/overlap_cases.py (3.19 for the area, 0.83 for the centroid), rounded up to a power of two.
C_AREA, C_CENTROID = 16.0, 4.0


def fields(rec):
    return tuple(rec[f].item() for f in oc.FIELDS)


@pytest.mark.parametrize("name", list(oc.EXACT))
def test_exact_cases_on_the_grid(name):
    a, b, expect = oc.EXACT[name]
    got = ref.poly_overlaps(oc.poly_set([a]), oc.poly_set([b]), [0], [0])[0]
    assert got["reserved"] == 0 and fields(got) == expect
    if len(a) == 4 and len(b) == 4:          # the rectangle form of the same pair
        planes = [np.array(pts, F).reshape(8, 1) for pts in (a, b)]
        assert ref.same(ref.rect_overlaps(*planes, [0], [0]), np.array([got])).all()


def test_the_whole_table_in_one_call_and_padding_junk_changes_nothing():
    """the cases as one list, in 16 rows with NaN, 1e30 and 0 behind each polygon's own vertices: the same bytes"""
    a, b, want = oc.exact_sets()
    n = len(want)
    got = ref.poly_overlaps(a, b, np.arange(n), np.arange(n))
    assert ref.same(got, want).all(), [name for name, ok in zip(oc.EXACT, ref.same(got, want)) if not ok]
    for junk in (1e30, 0.0, -np.inf):
        a, b, _ = oc.exact_sets(junk)
        assert ref.same(ref.poly_overlaps(a, b, np.arange(n), np.arange(n)), want).all(), junk


def test_the_area_far_from_the_origin_has_the_same_bits():
    """the frame is A's vertex 0: a pair moved by (100, 100), where 100 + x is exact for every coordinate, keeps every bit of the
    area, of the IoU and of the piece counts"""
    rng = np.random.default_rng(41)
    near, far = [], []
    for _ in range(50):
        pa = [tuple(p) for p in rng.integers(-32, 33, (2,)) / 16.0 + np.array(oc.square(0, 0, rng.integers(4, 40) / 16.0))]
        pb = [tuple(p) for p in rng.integers(-32, 33, (2,)) / 16.0 + np.array(oc.square(0, 0, rng.integers(4, 40) / 16.0))]
        near.append((pa, pb))
        far.append(([(x + 100, y + 100) for x, y in pa], [(x + 100, y + 100) for x, y in pb]))
    idx = np.arange(50)
    g0 = ref.poly_overlaps(oc.poly_set([p[0] for p in near]), oc.poly_set([p[1] for p in near]), idx, idx)
    g1 = ref.poly_overlaps(oc.poly_set([p[0] for p in far]), oc.poly_set([p[1] for p in far]), idx, idx)
    assert (g0["area"] > 0).sum() > 10
    for f in ("area", "iou", "area_a", "area_b", "hit", "flags", "pieces_a", "pieces_b"):
        assert g0[f].tobytes() == g1[f].tobytes(), f


def test_a_repeated_vertex_inside_the_other_shape_counts_as_a_piece():
    """pieces_a == ka reads "A inside B" with repeated vertices too: the zero-length edge survives every half-plane, adds 0 to the
    sums and 1 to the count, so area, IoU and centroid are those of the square without it"""
    plain = ref.poly_overlaps(oc.poly_set([oc.square(0.5, 0.5)]), oc.poly_set([oc.square(0, 0, 2.0)]), [0], [0])[0]
    twice = ref.poly_overlaps(oc.poly_set([[(0.5, 0.5), (1.5, 0.5), (1.5, 0.5), (1.5, 1.5), (0.5, 1.5)]]), oc.poly_set([oc.square(0, 0, 2.0)]), [0], [0])[0]
    assert fields(plain) == (1.0, 0.25, 1.0, 1.0, 1.0, 4.0, 1, 0, 4, 0)
    assert fields(twice) == (1.0, 0.25, 1.0, 1.0, 1.0, 4.0, 1, 0, 5, 0)


def test_bad_pairs_and_non_finite_input():
    a, b, want = oc.exact_sets()
    n = len(want)
    got = ref.poly_overlaps(a, b, [0, n, 0, -1], [0, 0, n + 5, 0])
    assert ref.same(got[:1], want[:1]).all()
    assert (got["flags"][1:] == ref.BAD_PAIR).all() and all(got[f][1:].tobytes() == bytes(got[f][1:].nbytes) for f in got.dtype.names if f != "flags")
    assert ref.BAD_PAIR == 8 and ref.same(got[1:2], got[2:3]).all()
    # NaN and infinity in a real slot: whatever the rule gives, in a well-formed record, and a NaN is the one quiet NaN
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(4):
            pa = [list(p) for p in oc.square(0, 0)]
            pa[slot][slot % 2] = bad
            for x, y in ((pa, oc.square(0.5, 0)), (oc.square(0.5, 0), pa)):
                rec = ref.poly_overlaps(oc.poly_set([x]), oc.poly_set([y]), [0], [0])[0]
                assert rec["reserved"] == 0 and rec["hit"] in (0, 1) and int(rec["flags"]) < 8
                for f in ref.FLOATS:
                    assert not np.isnan(rec[f]) or rec[f].view(np.uint32) == 0x7FC00000
                assert not np.isnan(rec["area"]) and not np.isnan(rec["iou"]) and rec["area"] >= 0


# ---- accuracy against a binary64 Sutherland-Hodgman clipper ----------------------------------------------------------------------------
convex_as_exact_values, random_convex = oc.convex_as_exact_values, oc.random_convex


def test_the_convexity_filter_sees_a_dent():
    assert convex_as_exact_values(np.array([0, 1, 1, 0], F), np.array([0, 0, 1, 1], F))
    assert convex_as_exact_values(np.array([0, 0, 1, 1], F), np.array([0, 1, 1, 0], F))                  # clockwise
    assert not convex_as_exact_values(np.array([0, 1, 0.4, 0], F), np.array([0, 0, 0.4, 1], F))
    assert not convex_as_exact_values(np.array([0, 1, 2], F), np.array([0, 1, 2], F))                    # all collinear


DRAWS = {0.0: 1100, 10.0: 1100, 1e3: 1100, 1e5: 1800}       # centre offset -> pairs drawn


def accuracy_inputs():
    """-> the kept pairs as [(offset, (ax, ay), (bx, by))] and, per offset, the share of the draws left out as not convex"""
    rng = np.random.default_rng(2501)
    kept, left_out = [], {}
    for offset, draws in DRAWS.items():
        scale = 1.0
        out = 0
        for _ in range(draws):
            ox, oy = offset * rng.choice([-1.0, 1.0]), offset * rng.uniform(-1.0, 1.0)
            a = random_convex(rng, ox + rng.uniform(-1, 1), oy + rng.uniform(-1, 1), scale)
            b = random_convex(rng, ox + scale * rng.uniform(-1.5, 1.5), oy + scale * rng.uniform(-1.5, 1.5), scale)
            if convex_as_exact_values(*a) and convex_as_exact_values(*b):
                kept.append((offset, a, b))
            else:
                out += 1
        left_out[offset] = out / draws
    return kept, left_out


def signed_area2(p):
    return sum(p[i][0] * p[(i + 1) % len(p)][1] - p[i][1] * p[(i + 1) % len(p)][0] for i in range(len(p)))


def clip64(a, b):
    """Sutherland-Hodgman in binary64: polygon a cut by each edge's half-plane of the convex polygon b (both counter-clockwise)
    -> the intersection polygon's area and centroid (None where the area is 0)"""
    out = a
    for f in range(len(b)):
        (qx, qy), (q1x, q1y) = b[f], b[(f + 1) % len(b)]
        gx, gy = q1x - qx, q1y - qy
        src, out = out, []
        for i in range(len(src)):
            (cx, cy), (nx, ny) = src[i], src[(i + 1) % len(src)]
            dc, dn = gx * (cy - qy) - gy * (cx - qx), gx * (ny - qy) - gy * (nx - qx)
            if dc >= 0:
                out.append((cx, cy))
            if (dc > 0 and dn < 0) or (dc < 0 and dn > 0):
                t = dc / (dc - dn)
                out.append((cx + t * (nx - cx), cy + t * (ny - cy)))
        if len(out) < 3:
            return 0.0, None
    s = signed_area2(out)
    if not s > 0:
        return 0.0, None
    mx = sum((out[i][0] + out[(i + 1) % len(out)][0]) * (out[i][0] * out[(i + 1) % len(out)][1] - out[i][1] * out[(i + 1) % len(out)][0]) for i in range(len(out)))
    my = sum((out[i][1] + out[(i + 1) % len(out)][1]) * (out[i][0] * out[(i + 1) % len(out)][1] - out[i][1] * out[(i + 1) % len(out)][0]) for i in range(len(out)))
    return 0.5 * s, (mx / (3 * s), my / (3 * s))


def pair_ratios(a, b, rec):
    """one pair's vertices (x, y binary32 arrays each) and its record -> |area - area64| / (u D^2) and, where area64 >= D^2 / 256,
    |centroid - centroid64| / (u (D^3 / area64 + |r| + D)) (infinity if the record has no centroid there), else NaN.  The clipper works in A's frame as well (the subtraction is
    exact in binary64 up to 2^-53 of r), so that its own error stays far below u D^2 at every offset."""
    (ax, ay), (bx, by) = a, b
    rx, ry = float(ax[0]), float(ay[0])
    pa = [(float(x) - rx, float(y) - ry) for x, y in zip(ax, ay)]
    pb = [(float(x) - rx, float(y) - ry) for x, y in zip(bx, by)]
    D = max(max(abs(c) for p in pa + pb for c in p), 1e-300)
    pa = pa if signed_area2(pa) > 0 else pa[::-1]
    pb = pb if signed_area2(pb) > 0 else pb[::-1]
    area64, c64 = clip64(pa, pb)
    r_area, r_cent = abs(float(rec["area"]) - area64) / (U * D * D), np.nan
    if area64 >= D * D / 256:
        err = np.hypot(float(rec["cx"]) - (rx + c64[0]), float(rec["cy"]) - (ry + c64[1]))
        r_cent = err / (U * (D ** 3 / area64 + np.hypot(rx, ry) + D))
        if rec["hit"] != 1 or rec["flags"] & ref.NO_CENTROID:          # such a pair has a centroid: a record without one is infinitely wrong
            r_cent = np.inf
    return r_area, r_cent


def accuracy_ratios():
    """-> per kept pair: its offset and the two ratios of pair_ratios(); and the shares left out"""
    kept, left_out = accuracy_inputs()
    n = len(kept)
    a, b = oc.poly_set([list(zip(*p[1])) for p in kept]), oc.poly_set([list(zip(*p[2])) for p in kept])
    got = ref.poly_overlaps(a, b, np.arange(n), np.arange(n))
    offsets, r_area, r_cent = np.zeros(n), np.zeros(n), np.full(n, np.nan)
    for q, (offset, pa, pb) in enumerate(kept):
        offsets[q] = offset
        r_area[q], r_cent[q] = pair_ratios(pa, pb, got[q])
    return offsets, r_area, r_cent, left_out, got


def test_accuracy_against_a_binary64_clipper():
    """|area - area64| <= C_AREA u D^2 for every pair, and |centroid - centroid64| <= C_CENTROID u (D^3 / area64 + |r| + D) where
    area64 >= D^2 / 256; D the largest |coordinate - r|, u = 2^-24.  Measured over these inputs: worst ratios 1.82 and 0.73, 5 100
    pairs, 3 460 of them with a centroid to compare; the jittered angles keep every vertex far enough from its neighbours' chord
    that no draw is left out as not convex, at offset 1e5 either."""
    offsets, r_area, r_cent, left_out, got = accuracy_ratios()
    print("pairs", len(offsets), "left out", left_out, "worst area ratio", r_area.max(), "worst centroid ratio", np.nanmax(r_cent),
          "with a centroid", int(np.isfinite(r_cent).sum()), "hit", float(got["hit"].mean()))
    assert len(offsets) >= 4000
    assert left_out[1e5] <= 0.4 and left_out[0.0] == 0 and left_out[10.0] == 0
    assert all((offsets == o).sum() >= 900 for o in DRAWS)
    assert 0.3 < got["hit"].mean() < 0.9 and np.isfinite(r_cent).sum() > 1500
    assert C_AREA <= 64 and C_CENTROID <= 64
    assert r_area.max() <= C_AREA, (int(r_area.argmax()), r_area.max())
    assert np.nanmax(r_cent) <= C_CENTROID, (int(np.nanargmax(r_cent)), np.nanmax(r_cent))


# ---- the families where two edges of the two shapes lie nearly on one line (tests/overlap_cases.py) -----------------------------------
def family_ratios(f):
    """-> the two ratios of pair_ratios() for every pair of the family, and the reference's records"""
    idx = np.arange(f.n)
    got = ref.poly_overlaps(f.a, f.b, idx, idx)
    r_area, r_cent = np.zeros(f.n), np.full(f.n, np.nan)
    for q in range(f.n):
        ka, kb = int(f.a[2][q]), int(f.b[2][q])
        r_area[q], r_cent[q] = pair_ratios((f.a[0][:ka, q], f.a[1][:ka, q]), (f.b[0][:kb, q], f.b[1][:kb, q]), got[q])
    return r_area, r_cent, got


# The constants per family: (area, centroid), each four times the worst ratio measured under the rule, rounded up to a power of two
# (DESIGN.md §5.27 and profiles/notes_r26_overlap_coincident.md list the measured values).  The box families and the neighbours keep
# the constants of the random pairs; the triangle and the jittered equal shapes have their own, capped at 2^14 u D^2.
C_AREA_ON_LINE, C_CENTROID_ON_LINE = 16.0, 4.0          # measured: 3.19 (equal shapes, 1 step) and 0.73 (equal shapes, 0 steps)
AREA_CAP = 2.0 ** 14


def family_bound(name):
    own = name == "triangle on an edge" or name.startswith("equal shapes")
    return (C_AREA_ON_LINE, C_CENTROID_ON_LINE) if own else (C_AREA, C_CENTROID)


def test_the_families_are_what_they_say():
    fam = oc.families()
    assert list(fam) == ["aligned boxes", "nested aligned box", "triangle on an edge"] + [f"equal shapes, {k} steps" for k in oc.JITTER_STEPS] + list(oc.NEIGHBOURS)
    for name, f in fam.items():
        assert f.left_out <= 0.05 and f.n >= 380 and set(f.offsets) == set(oc.FAMILY_OFFSETS), name
        assert f.a[0].shape == (16, f.n) and (f.planes is not None) == (name in oc.BOX_FAMILIES)
    f = fam["aligned boxes"]
    assert f.planes[0].shape == (8, f.n) and np.array_equal(f.planes[1][3], f.b[1][1]) and (f.area > 0).all() and ((f.iou > 0) & (f.iou < 1)).all()
    a, b = fam["equal shapes, 0 steps"].a, fam["equal shapes, 0 steps"].b
    assert np.array_equal(a[0][:, 0], b[0][:, 0], equal_nan=True) and not np.array_equal(a[0][:, 1], b[0][:, 1], equal_nan=True)      # same order, then relisted
    assert np.array_equal(np.sort(a[0][:a[2][1], 1]), np.sort(b[0][:b[2][1], 1]))
    one = np.array([1.0, -1.0, 0.0, 2.0 ** -149], F)
    assert np.array_equal(oc.steps32(one, np.array([1, 1, -1, -2])), np.array([1.0 + 2.0 ** -23, -(1.0 - 2.0 ** -24), -(2.0 ** -149), -(2.0 ** -149)], F))


@pytest.mark.parametrize("name", list(oc._family_draws()))
def test_accuracy_where_edges_lie_nearly_on_one_line(name):
    """Each family of tests/overlap_cases.py against the binary64 clipper, with the bounds of
    test_accuracy_against_a_binary64_clipper: |area - area64| <= c u D^2 and, where area64 >= D^2 / 256, a centroid within
    c' u (D^3 / area64 + |r| + D) (a record without a centroid there counts as infinitely wrong); the box families also against
    their analytic area and IoU.  Measured under the rule: no family above 3.19 (area) and 0.83 (centroid).  The rule before it
    (two edges counted as parallel only where den == 0 exactly; each side cutting at its own quotient) gave up to 3.1e6 u D^2 for
    the aligned boxes and 1.2e6 for equal shapes relisted and moved by two binary32 steps, with flags == 0."""
    f = oc.families()[name]
    c_area, c_cent = family_bound(name)
    assert c_area <= AREA_CAP
    r_area, r_cent, got = family_ratios(f)
    print(name, "pairs", f.n, "left out", f.left_out, "worst area ratio", r_area.max(), "pairs over the bound", int((r_area > c_area).sum()),
          "worst centroid ratio", np.nanmax(r_cent), "with a centroid", int(np.isfinite(r_cent).sum() + np.isinf(r_cent).sum()), "hit", float(got["hit"].mean()))
    if f.planes is not None:
        assert ref.same(ref.rect_overlaps(*f.planes, np.arange(f.n), np.arange(f.n)), got).all()
        oc.check_against_the_analytic_boxes(f, got, C_AREA, name)
    assert (got["hit"] == 1).mean() > 0.9
    assert (~np.isnan(r_cent)).sum() > f.n // 4 or name == "thin rectangle"          # (whose common area is below D^2 / 256 but for a few)
    assert r_area.max() <= c_area, (int(r_area.argmax()), r_area.max())
    assert np.nanmax(r_cent) <= c_cent, (int(np.nanargmax(r_cent)), np.nanmax(r_cent))
