"""The pairwise rectangle kernels' parallel-axis certificate (rect_collide_certified, c2d_math.hpp) outside its domain.

The certificate is a rounding bound: with a coordinate of 3e38 or inf an overlap of +inf passes a `need` of +inf, and a pair that
an axis of edge 2 or 3 separates was certified "collide".  The wave-wide fall-back hides this whenever another lane of the wave
holds a thin pair, so it shows only in a wave whose other pairs are all certified or separated: the exploring fuzz leg
sat_rect_verts met it at n = 4 (seed 465526156, configuration 6116), the four pairs recorded below.  The certificate is now kept
to |coordinate| < 2^61, as the N x M path keeps it (rect_side, c2d_cross.hip)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# float32 bit patterns, [pair][16]: x0 y0 .. x3 y3 of rectangle 1, then of rectangle 2.  Pairs 0 .. 2 are finite and not thin;
# pair 3 holds -3e38, -inf and 3e38 and is separated on an axis the fast path does not evaluate.
RECORDED = np.array([
    [3227768744, 1069591400, 1060253342, 1059451203, 1062139478, 1067085598, 3227297210, 1074008306,
     3219578760, 1060900181, 3223038025, 3197340990, 3213620780, 3213766018, 3203273866, 3182704762],
    [3208065356, 3224781945, 1063804696, 3222894413, 1021623728, 1061588120, 3217831228, 1051111376,
     3196647609, 1054940624, 1052211994, 1057455270, 1041030256, 1074044704, 3204056474, 1073596257],
    [3189539744, 1064971556, 3219437364, 3219632606, 1074940164, 3230028272, 1081793636, 3216277330,
     3213060517, 1063147454, 3221040054, 1045380800, 3211527988, 3215399053, 1022336480, 3206785292],
    [3224202464, 1070228080, 3223876834, 4284592614, 3208723852, 1038746040, 3210026372, 1071011660,
     1053267012, 4286578688, 1066636872, 3219525398, 2137108966, 1060607071, 1073019126, 1066860718],
], np.uint32).view(np.float32)


def all_entry_points(eng, planes):
    """booleans of c2d_sat_rect_pairs_verts (16-byte aligned planes: the 4-pairs-per-lane kernel), _verts_mask and _aos"""
    n = planes.shape[1]
    d = eng.to_device(planes)
    ptrs = [d.row(k) for k in range(16)]
    d_out, d_cnt = eng.zeros(n, np.uint8), eng.zeros(1, np.uint64)
    eng.sat_rect_pairs_verts(ptrs, n, d_out, d_cnt)
    verts, cnt = d_out.get(), int(d_cnt.get()[0])
    words = (n + 63) // 64
    d_mask = eng.zeros(words, np.uint64)
    eng.sat_rect_pairs_verts_mask(ptrs, n, d_mask, None)
    mask = np.unpackbits(d_mask.get().view(np.uint8), bitorder="little")[:n]
    d1, d2 = eng.to_device(np.ascontiguousarray(planes[:8].T)), eng.to_device(np.ascontiguousarray(planes[8:].T))
    d_aos = eng.zeros(n, np.uint8)
    eng.sat_rect_pairs_aos(d1, d2, n, d_aos, None)
    aos = d_aos.get()
    for a in (d, d_out, d_cnt, d_mask, d1, d2, d_aos):
        a.free()
    return {"verts": verts, "mask": mask, "aos": aos}, cnt


@pytest.mark.parametrize("reps", [1, 16, 64, 257])   # one lane; a quarter wave; one full wave; more than one block of the wide kernel
def test_recorded_pairs_outside_the_certificates_domain(eng, oracle, reps):
    planes = np.ascontiguousarray(np.tile(RECORDED.T, (1, reps)))
    with np.errstate(all="ignore"):
        ref, ref_cnt = oracle.sat_rect_pairs_verts(planes)
    assert list(ref[:4]) == [0, 1, 1, 0], "the recorded pairs no longer read as recorded"
    got, cnt = all_entry_points(eng, planes)
    for name, out in got.items():
        assert np.array_equal(out, ref), f"{name}: pairs {np.flatnonzero(out != ref)[:8]} differ from the oracle"
    assert cnt == ref_cnt


def test_recorded_pair_under_its_symmetries(eng, oracle):
    """The recorded pair with its rectangles exchanged, negated, mirrored in x = y and their vertex order rotated: 128 pairs, all
    separated.  The rotations move the separating axis between the edges the fast path evaluates (0, 1) and those it certifies
    (2, 3); no variant is thin, so no lane makes its wave fall back."""
    r1, r2 = RECORDED[3][:8].reshape(4, 2), RECORDED[3][8:].reshape(4, 2)
    pairs = []
    for a, b in ((r1, r2), (r2, r1)):
        for sign in (1, -1):
            for mirror in (False, True):
                for s1 in range(4):
                    for s2 in range(4):
                        aa, bb = np.roll(a, s1, 0) * sign, np.roll(b, s2, 0) * sign
                        if mirror:
                            aa, bb = aa[:, ::-1], bb[:, ::-1]
                        pairs.append(np.concatenate([aa.ravel(), bb.ravel()]))
    planes = np.ascontiguousarray(np.array(pairs, np.float32).T)
    with np.errstate(all="ignore"):
        ref, ref_cnt = oracle.sat_rect_pairs_verts(planes)
    assert ref_cnt == 0, "a symmetry of a separated pair reads as colliding"
    got, cnt = all_entry_points(eng, planes)
    for name, out in got.items():
        assert np.array_equal(out, ref), f"{name}: pairs {np.flatnonzero(out != ref)[:8]} differ from the oracle"
    assert cnt == ref_cnt
