"""What the tests of c2d_poly_sweep_broad_pairs share (test_gpu_sweep_broad.py, tools/sweep_broad_fuzz.py): a moving set on the
device with guard bands around its motion planes, the list call between guard entries, the judge that compares a list with the
reference (tests/sweep_broad_ref.py), and the scenes.  The judge and the scenes are numpy only, so the CPU tests can reach them."""
import numpy as np

import sweep_broad_ref as ref

F32 = np.float32
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
BAND = 8                      # guard floats on either side of a motion plane: NaN, so that a read outside the plane poisons the list


# ---- scenes (numpy only) ------------------------------------------------------------------------------------------------------
def nan_padded(s):
    """the set with NaN in every vertex slot >= the polygon's count"""
    vx, vy, k = s
    if k is None:
        return s
    pad = np.arange(vx.shape[0])[:, None] >= np.clip(k.astype(np.int64), 1, None)[None, :]
    return np.where(pad, F32(np.nan), vx), np.where(pad, F32(np.nan), vy), k


def motion(n, seed, lo=3.0, hi=9.0):
    """one displacement per polygon: a random direction, lo .. hi long (the scenes' polygons are about 3 across)"""
    rng = np.random.default_rng(seed)
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(lo, hi, n)
    return (mag * np.cos(ang)).astype(F32), (mag * np.sin(ang)).astype(F32)


def sparse_scene(wl, n, seed, rows=16, kmax=16, density=1.0):
    """(set, motion): the sparse scene of the polygon broad phase's tests, moving by one to three polygon sizes"""
    extent = 200.0 * np.sqrt(max(n, 64) / 32768) / density
    s = nan_padded(wl.random_convex_polygon_set(n, seed=seed, kmin=min(3, kmax), kmax=kmax, extent=extent, rows=rows))
    return s, motion(n, seed + 7)


# ---- the judge (numpy only) ---------------------------------------------------------------------------------------------------
def compare(got, total, want):
    """None when the list `got` (u32[m][2]) with the reported total equals the reference list `want`, else what differs"""
    want = np.asarray(want, np.uint32).reshape(-1, 2)
    got = np.asarray(got, np.uint32).reshape(-1, 2)
    if total != len(want):
        return f"the total is {total}, the reference has {len(want)} pairs"
    if len(got) != len(want):
        return f"{len(got)} pairs written, the reference has {len(want)}"
    if np.array_equal(got, want):
        return None
    gs, ws = set(map(tuple, got.tolist())), set(map(tuple, want.tolist()))
    if gs == ws:
        at = int(np.flatnonzero((got != want).any(1))[0])
        return f"the same pairs in another order: first at position {at}, got {got[at].tolist()}, want {want[at].tolist()}"
    return f"{len(ws - gs)} pairs missing, e.g. {sorted(ws - gs)[:3]}; {len(gs - ws)} extra, e.g. {sorted(gs - ws)[:3]}"


# ---- the device side ----------------------------------------------------------------------------------------------------------
class MovingSet:
    """A set on the device as test_gpu_sat_poly_cross.Uploaded lays it out (row offset, stride, gaps of NaN), with its motion: two
    planes f32[n], each between BAND guard floats of NaN.  .set is the c2d_poly_set, .motion the pair of plane pointers or None;
    .check() asserts that the planes and their bands still hold what was uploaded."""

    def __init__(self, eng, s, mot=None, offset=0, stride=None, with_k=True):
        vx, vy, k = s
        self.eng, self.rows, self.n = eng, vx.shape[0], vx.shape[1]
        self.stride = self.n if stride is None else stride
        host = np.full((2, self.rows * self.stride + 4), np.nan, F32)
        for p, v in enumerate((vx, vy)):
            for r in range(self.rows):
                host[p, offset + r * self.stride: offset + r * self.stride + self.n] = v[r]
        self.d = eng.to_device(host)
        self.px, self.py = self.d.row(0) + 4 * offset, self.d.row(1) + 4 * offset
        self.dk = eng.to_device(k) if (k is not None and with_k) else None
        self.set = eng.poly_set(self.px, self.py, self.dk, self.n, self.rows, self.stride)
        self._upload_motion(mot)

    def _upload_motion(self, mot):
        self.dm = self.motion = self.host_m = None
        if mot is not None:
            self.host_m = np.full((2, self.n + 2 * BAND), np.nan, F32)
            self.host_m[0, BAND:BAND + self.n], self.host_m[1, BAND:BAND + self.n] = mot
            self.dm = self.eng.to_device(self.host_m)
            self.motion = (self.dm.row(0) + 4 * BAND, self.dm.row(1) + 4 * BAND)

    def with_motion(self, mot):
        """the same vertex memory (the same c2d_poly_set) with other motion planes; its free() frees those planes only"""
        other = MovingSet.__new__(MovingSet)
        other.eng, other.rows, other.n, other.stride, other.set = self.eng, self.rows, self.n, self.stride, self.set
        other.d = other.dk = None
        other._upload_motion(mot)
        return other

    def check(self):
        if self.dm is not None:
            assert self.dm.get().tobytes() == self.host_m.tobytes(), "a motion plane or its guard band was written"

    def free(self):
        self.check()
        for x in (self.d, self.dk, self.dm):
            if x is not None:
                x.free()


def _synchronize(eng, absent):
    """the synchronise behind a call: with a vertex count out of range in the sets it must report the error, once"""
    if not absent:
        eng.synchronize()
        return
    try:
        eng.synchronize()
    except Exception as e:                    # (c2d_amd.binding.C2DError; the harness does not import the package)
        if type(e).__name__ != "C2DError":
            raise
    else:
        raise AssertionError("a vertex count outside 1..rows was not reported by the synchronise")
    eng.synchronize()                         # reported once, then clear


def run(eng, A, B, upper=False, capacity=None, ma="own", mb="own", stream=0, absent=False):
    """(pairs u32[capacity][2], total) of c2d_poly_sweep_broad_pairs on the MovingSets A, B (their own motions unless given);
    capacity None: count first, then exact.  The list sits between four guard entries in front and four (plus everything past
    the capacity) behind, which are checked.  absent: the sets hold a vertex count out of range, which every call must report."""
    ma = A.motion if isinstance(ma, str) else ma
    mb = B.motion if isinstance(mb, str) else mb
    d_cnt = eng.zeros(1, np.uint64)
    if capacity is None:
        eng.poly_sweep_broad_pairs(A.set, B.set, None, 0, d_cnt, ma, mb, upper=upper, stream=stream)
        _synchronize(eng, absent)
        capacity = int(d_cnt.get()[0])
        eng.memset(d_cnt, 0, 8)
    d_pairs = eng.empty((capacity + 8, 2), np.uint32)
    eng.memset(d_pairs, 0xA5, d_pairs.nbytes)
    eng.poly_sweep_broad_pairs(A.set, B.set, d_pairs.ptr + 32, capacity, d_cnt, ma, mb, upper=upper, stream=stream)
    _synchronize(eng, absent)
    p, c = d_pairs.get(), int(d_cnt.get()[0])
    d_pairs.free()
    d_cnt.free()
    assert (p[:4].view(np.uint64) == SENTINEL).all(), "written in front of the list"
    assert (p[4 + capacity:].view(np.uint64) == SENTINEL).all(), "written past the capacity"
    return p[4:4 + capacity], c


def check(eng, a, b, ma, mb, upper=False, min_pairs=1, want=None, place_a=(1, 3), place_b=(2, 0), with_k=True):
    """the list of (a, ma) against (b, mb) — b None: the set against itself, the same memory and the same planes — equals the
    reference; returns (list, reference list)"""
    A = MovingSet(eng, a, ma, offset=place_a[0], stride=a[0].shape[1] + place_a[1], with_k=with_k)
    B = A if b is None else MovingSet(eng, b, mb, offset=place_b[0], stride=b[0].shape[1] + place_b[1], with_k=with_k)
    try:
        got, total = run(eng, A, B, upper)
    finally:
        A.free()
        if B is not A:
            B.free()
    if want is None:
        want = ref.pairs(a, a if b is None else b, ma, ma if b is None else mb, upper=upper)
    why = compare(got, total, want)
    assert why is None, why
    assert total >= min_pairs, total
    return got, want
