"""Constructed inputs for the tests of the pairwise rectangle kernels' first tier (rect_gap_certified, csrc/c2d_math.hpp):
pairs it certifies by one chosen direction, pairs that touch to within a few ulps on one chosen axis of the reference, quads
that are no parallelograms, quads without area, coordinates outside the certificate's domain and non-finite ones.  Used by
tests/test_rect_gap_cpu.py (numpy restatement against the oracle) and tests/test_gpu_sat_gap_form.py (kernels against the oracle)."""
import numpy as np

from rect_gap_ref import rect_gap_certified, rect_gap_terms

F, D = np.float32, np.float64


def pose_planes(oracle, poses):
    poses = [np.asarray(p, F) for p in poses]
    return np.concatenate([oracle.rects_from_poses(*poses[:5]), oracle.rects_from_poses(*poses[5:])])


def certified_pools(oracle, wl, seed, n=60_000, extent=4.0):
    """-> (sep_by[4], col): planes of random pairs that exactly one direction (a1, b1, a2, b2) certifies as separated, and of
    pairs certified as colliding"""
    planes = pose_planes(oracle, wl.random_obb_pose_planes(n, seed=seed, extent=extent))
    G, M, _ = rect_gap_terms(planes)
    over = np.stack([(g - m).astype(F) > 0 for g, m in zip(G, M)])
    col, _, _ = rect_gap_certified(planes)
    return [planes[:, over[k] & (over.sum(0) == 1)] for k in range(4)], planes[:, col]


def _rect64(rng):
    """a random rectangle in the reference's vertex order, float64 [4][2]"""
    hx, hy = rng.uniform(0.25, 2.0, 2)
    th = rng.uniform(0, 2 * np.pi)
    c = rng.uniform(-6, 6, 2)
    u, v = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
    return np.stack([c - hx * u - hy * v, c + hx * u - hy * v, c + hx * u + hy * v, c - hx * u + hy * v])


def ulp_touching_pairs(rng, reps, nudges=range(-8, 9)):
    """Pairs whose projection intervals touch on ONE of the reference's eight axes (edge i of rectangle 1 for axis i < 4, edge
    i - 4 of rectangle 2 otherwise; the other rectangle sits on the side the edge vector points to), and overlap on the others;
    the touching vertex is then moved by k float32 ulps along the axis' dominant coordinate, k in `nudges`.
    -> planes f32[16][reps * 8 * len(nudges)], ordered (rep, axis, nudge)"""
    out = []
    for _ in range(reps):
        A, B = _rect64(rng), _rect64(rng)
        for axis in range(8):
            own, other = (A, B) if axis < 4 else (B, A)
            i = axis % 4
            nrm = own[(i + 1) % 4] - own[i]
            nrm = nrm / np.hypot(*nrm)
            perp = np.array([-nrm[1], nrm[0]])
            moved = other - other.mean(0) + own.mean(0) + perp * rng.uniform(-0.2, 0.2)
            moved = moved + nrm * ((own @ nrm).max() - (moved @ nrm).min())
            own32, moved32 = own.astype(F), moved.astype(F)
            k_vertex = int(np.argmin(moved @ nrm))
            k_coord = int(np.argmax(np.abs(nrm)))
            away = F(np.inf) if nrm[k_coord] > 0 else F(-np.inf)
            for k in nudges:
                m = moved32.copy()
                for _ in range(abs(k)):
                    m[k_vertex, k_coord] = np.nextafter(m[k_vertex, k_coord], away if k > 0 else -away)
                r1, r2 = (own32, m) if axis < 4 else (m, own32)
                out.append(np.concatenate([r1.ravel(), r2.ravel()]))
    return np.ascontiguousarray(np.array(out, F).T)


def _quads(rng, n, kind):
    """n convex quads (8 planes) that are no parallelograms: v0, v0 + a, v0 + a + b + delta, v0 + b"""
    th = rng.uniform(0, 2 * np.pi, n)
    w, h = rng.uniform(1, 4, n), rng.uniform(1, 4, n)
    a = np.stack([w * np.cos(th), w * np.sin(th)])
    b = np.stack([-h * np.sin(th), h * np.cos(th)])
    if kind == "kite":      # v2 on the diagonal through v0, nearer or farther than a parallelogram's
        delta = (a + b) * rng.uniform(-0.4, 0.8, n)
    else:                   # trapezoid: the edge v3 -> v2 parallel to a, shorter or longer
        delta = a * rng.uniform(-0.7, 0.7, n)
    v0 = rng.uniform(-6, 6, (2, n))
    v = [v0, v0 + a, v0 + a + b + delta, v0 + b]
    return np.stack([c for p in v for c in p]).astype(F)


def non_parallelogram_pairs(oracle, rng, n, kind, order):
    """A trapezoid or kite and a small square between its vertex 2 and the vertex 2 of the parallelogram through its v0, v1, v3
    (what the gap form models).  order 0: the quad is rectangle 1.  -> (planes, errs): errs marks the pairs for which the oracle
    answers differently for the model than for the quad itself"""
    q = _quads(rng, n, kind)
    model = q.copy()
    model[4], model[5] = (q[2] + q[6]) - q[0], (q[3] + q[7]) - q[1]
    c = np.stack([(q[4] + model[4]) / 2, (q[5] + model[5]) / 2]) + rng.normal(0, 0.7, (2, n))
    s = rng.uniform(0.05, 0.6, n)
    th = rng.uniform(0, 2 * np.pi, n)
    ux, uy = s * np.cos(th), s * np.sin(th)
    sq = np.stack([c[0] - ux + uy, c[1] - uy - ux, c[0] + ux + uy, c[1] + uy - ux, c[0] + ux - uy, c[1] + uy + ux, c[0] - ux - uy, c[1] - uy + ux]).astype(F)
    planes = np.ascontiguousarray(np.concatenate([q, sq] if order == 0 else [sq, q]))
    as_model = np.ascontiguousarray(np.concatenate([model, sq] if order == 0 else [sq, model]))
    truth, _ = oracle.sat_rect_pairs_verts(planes)
    modelled, _ = oracle.sat_rect_pairs_verts(as_model)
    return planes, truth != modelled


def certified_base(oracle, wl, n, seed=77):
    """n random pairs of the bench workload's kind, none of them thin"""
    planes = pose_planes(oracle, wl.random_obb_pose_planes(2 * n + 64, seed=seed))
    _, _, thin = rect_gap_certified(planes)
    planes = np.ascontiguousarray(planes[:, ~thin][:, :n])
    assert planes.shape[1] == n
    return planes


def degenerate_quads(rect):
    """Quads without area on the centre of `rect` (8 planes): a point, a segment (v0 = v3, v1 = v2), a repeated vertex
    (v0 = v1; v1 = v2), all four vertices on a line.  -> {name: 8 planes}"""
    cx, cy = (rect[0] + rect[4]) / 2, (rect[1] + rect[5]) / 2
    hx, hy = (rect[2] - rect[0]) / 4, (rect[3] - rect[1]) / 4            # a quarter of its edge 0
    fams = {
        "point": [cx, cy, cx, cy, cx, cy, cx, cy],
        "segment": [cx - hx, cy - hy, cx + hx, cy + hy, cx + hx, cy + hy, cx - hx, cy - hy],
        "v0 = v1": [cx - hx, cy - hy, cx - hx, cy - hy, cx + hx, cy + hy, cx + hy, cy - hx],
        "v1 = v2": [cx - hx, cy - hy, cx + hx, cy + hy, cx + hx, cy + hy, cx + hy, cy - hx],
        "on a line": [cx - hx, cy - hy, cx - hx / 2, cy - hy / 2, cx + hx, cy + hy, cx + hx / 2, cy + hy / 2],
    }
    return {k: np.stack(v).astype(F) for k, v in fams.items()}


def scaled_to(base, top):
    """the pairs of `base`, each scaled so that its largest |coordinate| is exactly `top`"""
    C = np.abs(base).max(0)
    with np.errstate(over="ignore"):
        out = (base.astype(D) / C * top).astype(F)
        out[np.abs(base) == C] = np.copysign(F(top), base[np.abs(base) == C])
    return out


def with_non_finite(base, rng, share=0.1):
    """`base` with NaN, +inf, -inf in a random `share` of its coordinates -> (planes, touched pairs)"""
    out = base.copy()
    hit = rng.random(base.shape) < share
    out[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(hit.sum()))
    return out, hit.any(0)
