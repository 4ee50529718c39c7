"""rect_gap_certified (csrc/c2d_math.hpp), the first tier of the pairwise rectangle kernels, on the CPU: its float32 numpy
restatement (tests/rect_gap_ref.py) decision by decision against the oracle's vertex SAT, the share of pairs it leaves to the
second tier, the inequality its margin rests on in float64, and the inputs that must come out thin."""
import numpy as np
import pytest

from rect_gap_cases import certified_base, degenerate_quads, non_parallelogram_pairs, pose_planes, scaled_to, ulp_touching_pairs, with_non_finite
from rect_gap_ref import U, rect_gap_certified, rect_gap_terms

F, D = np.float32, np.float64

RANDOM_SCALES = ((8, 0.1, 5, 1), (8, 0.1, 5, 1e-3), (8, 0.1, 5, 1e4), (100, 0.1, 5, 1), (1, 0.5, 2, 1), (1000, 0.01, 1, 1), (3, 3, 6, 1), (2, 1e-3, 4, 1))
TOUCHING = ((1.0, 0.0), (1.0, 50.0), (1e-4, 0.0), (1e3, 0.0))


def random_poses(rng, n, pos, lo, hi, scale):
    xy = [rng.uniform(-pos, pos, n) * scale for _ in range(4)]
    wh = [rng.uniform(lo, hi, n) * scale for _ in range(4)]
    th = [rng.uniform(-7, 7, n) for _ in range(2)]
    return np.stack([xy[0], xy[1], wh[0], wh[1], th[0], xy[2], xy[3], wh[2], wh[3], th[1]]).astype(F)


@pytest.fixture(scope="module")
def random_planes(oracle):
    rng = np.random.default_rng(11)
    return [pose_planes(oracle, random_poses(rng, 60_000, *s)) for s in RANDOM_SCALES]


@pytest.fixture(scope="module")
def touching_planes(oracle, wl):
    return [pose_planes(oracle, wl.touching_pose_pairs(40_000, seed=12 + seed, scale=scale, offset=off)) for seed, (scale, off) in enumerate(TOUCHING)]


def variant(oracle, name):
    return oracle if name == "canonical" else oracle.load_variant(name)


def against_oracle(orc, planes):
    """-> thin share; every decision taken must be the oracle's"""
    with np.errstate(all="ignore"):
        ref, _ = orc.sat_rect_pairs_verts(np.ascontiguousarray(planes, F))
    col, sep, thin = rect_gap_certified(planes)
    assert not (col & sep).any() and ((col | sep) ^ thin).all()
    assert not (sep & (ref != 0)).any(), "gap form says separated, the oracle says the pair collides"
    assert not (col & (ref == 0)).any(), "gap form says colliding, the oracle finds a separating axis"
    return float(thin.mean())


@pytest.mark.parametrize("build", ["canonical", "fmad1", "fmad2"])
def test_gap_form_decides_like_the_oracle_on_random_pairs(oracle, random_planes, build):
    for s, planes in zip(RANDOM_SCALES, random_planes):
        assert against_oracle(variant(oracle, build), planes) < 1e-3, s


@pytest.mark.parametrize("build", ["canonical", "fmad1", "fmad2"])
def test_gap_form_on_razor_thin_pairs(oracle, touching_planes, build):
    """Pairs built to touch (workloads.touching_pose_pairs): 48 - 71 % of them are thin, the rest decided as the oracle decides."""
    for planes in touching_planes:
        assert against_oracle(variant(oracle, build), planes) > 0.01, "the construction is meant to land inside the margin often"


def test_thin_share_on_the_bench_workload(oracle, wl):
    """Config 2 (centres +-8, sizes 0.1 - 5): 0.7e-5 .. 1.5e-5 of the pairs are thin (three seeds of 2e6 pairs); the cap leaves a
    factor of ten, so that about one wave of 256 pairs in 400 falls back."""
    thin = against_oracle(oracle, pose_planes(oracle, wl.random_obb_pose_planes(1_000_000)))
    assert thin <= 1e-4, thin


def _projections(ax, ay, r, fmad):
    """the reference's four projections of a quad (8 planes) onto the float32 axis (ax, ay), dot2 of c2d_math.hpp"""
    out = []
    for k in range(4):
        x, y = r[2 * k], r[2 * k + 1]
        if fmad == 0:
            p = ((ax * x).astype(F) + (ay * y).astype(F)).astype(F)
        elif fmad == 1:
            p = (ax.astype(D) * x + (ay * y).astype(F)).astype(F)
        else:
            p = (ay.astype(D) * y + (ax * x).astype(F)).astype(F)
        out.append(p)
    return np.stack(out)


def test_gap_form_error_budget(oracle, wl, random_planes, touching_planes):
    """The inequalities the margin rests on (c2d_math.hpp rect_gap_certified, (1) .. (5)), in float64, on random and on touching
    pairs, for the reference's unfused projections and both fused forms.  With G_d the real gap of the real edge vectors, doubled
    centres and defects, on every one of the reference's eight axes n (computed, float32):
      * twice the smaller computed overlap differs from -G_d by at most R = 12.04u (A + e_q) C + 4 C e_q + 3 (|d.delta_1| + |d.delta_2|);
      * the gap as evaluated differs from G_d by at most 82.6 u A C;
      * the margin the code uses is at least the sum of the two.
    Worst ratios seen: 0.97 (the defect term is attained on touching pairs), 0.12 and 0.75."""
    worst = [0.0, 0.0, 0.0]
    for planes in [p[:, :20_000] for p in random_planes] + [p[:, :20_000] for p in touching_planes]:
        G32, M32, C32 = rect_gap_terms(planes)
        C = C32.astype(D)
        P = planes.astype(D)
        quads = []
        for r in (P[:8], P[8:]):
            a = (r[2] - r[0], r[3] - r[1])
            b = (r[6] - r[0], r[7] - r[1])
            s = (r[0] + r[4], r[1] + r[5])
            delta = (s[0] - (r[2] + r[6]), s[1] - (r[3] + r[7]))
            quads.append((a, b, s, delta))
        Dx, Dy = quads[1][2][0] - quads[0][2][0], quads[1][2][1] - quads[0][2][1]
        e = [np.abs(q[3][0]) + np.abs(q[3][1]) for q in quads]

        def dot(p, q):
            return p[0] * q[0] + p[1] * q[1]

        for qi, r in enumerate((planes[:8], planes[8:])):
            for i in range(4):
                d = quads[qi][i % 2]                                     # edges 0, 2 go with a, edges 1, 3 with b
                A = np.abs(d[0]) + np.abs(d[1])
                G = np.abs(dot(d, (Dx, Dy))) - sum(np.abs(dot(d, quads[q][k])) for q in range(2) for k in range(2))
                R = 12.04 * U * (A + e[qi]) * C + 4 * C * e[qi] + 3 * (np.abs(dot(d, quads[0][3])) + np.abs(dot(d, quads[1][3]))) + 1e-37
                ax, ay = (r[(2 * i + 2) & 7] - r[2 * i]).astype(F), (r[(2 * i + 3) & 7] - r[2 * i + 1]).astype(F)
                for fmad in range(3):
                    p1, p2 = _projections(ax, ay, planes[:8], fmad).astype(D), _projections(ax, ay, planes[8:], fmad).astype(D)
                    overlap = np.minimum(p1.max(0) - p2.min(0), p2.max(0) - p1.min(0))
                    ratio = np.abs(2 * overlap + G) / R
                    assert (ratio <= 1.0).all(), (qi, i, fmad, float(ratio.max()))
                    worst[0] = max(worst[0], float(ratio.max()))
                if i < 2:
                    g, m = G32[2 * qi + i].astype(D), M32[2 * qi + i].astype(D)
                    E = 82.6 * U * A * C + 1e-37
                    ratio = np.abs(g - G) / E
                    assert (ratio <= 1.0).all(), (qi, i, float(ratio.max()))
                    worst[1] = max(worst[1], float(ratio.max()))
                    ratio = (R + E) / m
                    assert (ratio <= 1.0).all(), (qi, i, float(ratio.max()))
                    worst[2] = max(worst[2], float(ratio.max()))
    assert 0.5 < worst[0] and 0.01 < worst[1] and 0.5 < worst[2], worst   # the ratios above are <= 1; these say the test can see them


@pytest.mark.parametrize("kind", ["trapezoid", "kite"])
def test_quads_that_are_no_parallelograms_are_thin_where_their_model_errs(oracle, kind):
    """A trapezoid or kite next to a small square near its vertex 2: wherever the parallelogram through v0, v1, v3 (what the gap
    form models) gets another answer from the oracle than the quad itself, the pair must be thin — through the defect term, not
    by luck.  Both orders of the pair; no decision taken anywhere differs from the oracle's."""
    rng = np.random.default_rng(21 if kind == "kite" else 22)
    for order in (0, 1):
        planes, errs = non_parallelogram_pairs(oracle, rng, 40_000, kind, order)
        assert errs.sum() > 1000, "the construction is meant to make the model err often"
        truth, _ = oracle.sat_rect_pairs_verts(planes)
        col, sep, thin = rect_gap_certified(planes)
        assert thin[errs].all()
        assert not (sep & (truth != 0)).any() and not (col & (truth == 0)).any()


def test_pairs_within_a_few_ulps_of_touching(oracle):
    """Intervals that touch on one chosen axis of the reference, the touching vertex moved by -8 .. 8 ulps: on that axis the gap is far
    inside the margin, so the pair is thin unless another direction separates it outright (a corner beside an edge: 28 % of the
    construction); none is decided against the oracle."""
    planes = ulp_touching_pairs(np.random.default_rng(31), reps=20)
    assert against_oracle(oracle, planes) > 0.5
    col, _, _ = rect_gap_certified(planes)
    assert not col.any()


def test_degenerate_quads_are_thin(oracle, wl):
    """Quads without area that touch the other rectangle: collapsed to a point, to a segment (v0 = v3, v1 = v2), with a repeated
    vertex (v0 = v1; v1 = v2), or with all four vertices on a line.  A zero edge vector has G = 0 and can certify nothing, so
    such a pair is never certified as colliding; placed on the other rectangle's centre it is not certified as separated either.
    (Far from the other rectangle a degenerate quad may be certified as separated: the reference's axes say the same.  Four
    vertices on a line are a parallelogram with parallel axes, which the form models exactly: decided or thin, never wrongly.)"""
    base = certified_base(oracle, wl, 2_000)
    for name, quad in degenerate_quads(base[8:]).items():
        for planes in (np.concatenate([quad, base[8:]]), np.concatenate([base[8:], quad])):
            col, sep, thin = rect_gap_certified(planes)
            if name != "on a line":
                assert thin.all(), name
            ref, _ = oracle.sat_rect_pairs_verts(np.ascontiguousarray(planes))
            assert not (sep & (ref != 0)).any() and not (col & (ref == 0)).any(), name
        far = np.ascontiguousarray(np.concatenate([quad + F(40.0), base[8:]]))
        col, sep, thin = rect_gap_certified(far)
        ref, _ = oracle.sat_rect_pairs_verts(far)
        assert not col.any() or name == "on a line"
        assert not (sep & (ref != 0)).any() and not (col & (ref == 0)).any(), name


def test_out_of_domain_and_non_finite_pairs_are_thin(oracle, wl):
    """Subnormal coordinates (every |G| below the absolute slack), coordinates of 2^61 and more (products may overflow), and a
    NaN, +inf or -inf in each of the sixteen positions of otherwise certified pairs."""
    base = certified_base(oracle, wl, 1_000)
    assert rect_gap_certified((base * F(2.0 ** -140)).astype(F))[2].all()
    for top in (2.0 ** 61, 2.0 ** 61 * 1.5, 2.0 ** 90, 2.0 ** 126, 3e38):
        assert rect_gap_certified(scaled_to(base, top))[2].all(), top
    assert not rect_gap_certified(scaled_to(base, 2.0 ** 60))[2].any(), "2^60 is inside the domain"
    for k in range(16):
        for bad in (np.nan, np.inf, -np.inf):
            planes = base.copy()
            planes[k] = bad
            assert rect_gap_certified(planes)[2].all(), (k, bad)
    some, touched = with_non_finite(base, np.random.default_rng(3))
    assert rect_gap_certified(some)[2][touched].all()
