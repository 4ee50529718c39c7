"""The one frame of the tests of the pair searches (c2d_sat_rect_cross_pairs / _broad_pairs, c2d_sat_poly_cross_pairs / _broad_pairs,
c2d_poly_sweep_broad_pairs, c2d_poly_near_broad_pairs), as csrc/c2d_broad.hpp is the one frame of their kernels: every one of them
fills a row-major u32[capacity][2] list and increments a device count by the total.  Here: the polygon set on the device (with or
without motion planes), run() with its guard entries around the list, the judge compare(), the scenes the searches share, and one
adaptor per entry point that turns its arguments into run()'s call.  A plain module (pytest does not collect it) on numpy only: it
never loads libc2d.so, so the CPU tests reach the judge, the guard check and the scenes.  tests/test_pair_search_harness_cpu.py plants faults for guard_fault() and compare()."""
import numpy as np

F32 = np.float32
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)      # a guard entry: both indices 0xA5A5A5A5
GUARD = 4                                     # guard entries in front of and behind every list
BAND = 8                                      # guard floats on either side of a motion plane: NaN, so that a read outside the plane poisons the list


# ---- scenes (numpy only) ------------------------------------------------------------------------------------------------------
def nan_padded(s):
    """the set with NaN in every vertex slot >= the polygon's count (counts outside 1..rows: every slot of a count of 0 stays)"""
    vx, vy, k = s
    if k is None:
        return s
    pad = np.arange(vx.shape[0])[:, None] >= np.clip(k.astype(np.int64), 1, None)[None, :]
    return np.where(pad, F32(np.nan), vx), np.where(pad, F32(np.nan), vy), k


def sparse_set(wl, n, seed, rows=16, kmax=16, density=1.0):
    """the sparse scene of the polygon cross bench, its extent scaled so that the hits per polygon stay constant; polygons about 2.5 across"""
    extent = 200.0 * np.sqrt(max(n, 64) / 32768) / density
    return nan_padded(wl.random_convex_polygon_set(n, seed=seed, kmin=min(3, kmax), kmax=kmax, extent=extent, rows=rows))


# ---- the judges (numpy only) --------------------------------------------------------------------------------------------------
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


def guard_fault(buf, capacity):
    """None when the downloaded buffer u32[GUARD + capacity + GUARD][2] still holds its guard entries, else which of them was written"""
    assert buf.shape == (capacity + 2 * GUARD, 2) and buf.dtype == np.uint32, (buf.shape, buf.dtype, capacity)
    flat = np.ascontiguousarray(buf).view(np.uint64).reshape(-1)
    front, rear = np.flatnonzero(flat[:GUARD] != SENTINEL), np.flatnonzero(flat[GUARD + capacity:] != SENTINEL)
    if len(front):
        return f"written in front of the list: {GUARD - int(front[-1])} entries before it, {buf[front[-1]].tolist()}"
    if len(rear):
        return f"written past the capacity: entry {capacity + int(rear[0])} of a list of {capacity}, {buf[GUARD + capacity + rear[0]].tolist()}"
    return None


# ---- the device side ----------------------------------------------------------------------------------------------------------
class DeviceSet:
    """A polygon set on the device: every plane row shifted by `offset` floats, `stride` >= n elements between vertex rows; the gaps
    hold NaN.  .set is the c2d_poly_set; .sub(r0, r1) the shard of polygons [r0, r1) (pointer offset, the same stride).  With `mot`
    it carries its motion: two planes f32[n], each between BAND guard floats of NaN; .motion is the pair of plane pointers or None,
    and .check() asserts that the planes and their bands still hold what was uploaded.  A set at rest is one without motion."""

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
        self.set = self.sub(0, self.n)
        self._upload_motion(mot)

    def sub(self, r0, r1):
        return self.eng.poly_set(self.px + 4 * r0, self.py + 4 * r0, None if self.dk is None else self.dk.ptr + r0, r1 - r0, self.rows, self.stride)

    def _upload_motion(self, mot):
        self.dm = self.motion = self.host_m = None
        if mot is not None:
            self.host_m = np.full((2, self.n + 2 * BAND), np.nan, F32)
            self.host_m[0, BAND:BAND + self.n], self.host_m[1, BAND:BAND + self.n] = mot
            self.dm = self.eng.to_device(self.host_m)
            self.motion = (self.dm.row(0) + 4 * BAND, self.dm.row(1) + 4 * BAND)

    def with_motion(self, mot):
        """the same vertex memory (the same c2d_poly_set) with other motion planes; its free() frees those planes only"""
        other = DeviceSet.__new__(DeviceSet)
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


def synchronize(eng, absent=False):
    """the synchronise behind a call: with a vertex count out of range in the sets (absent) it must report the error, once"""
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


def run(eng, call, capacity=None, absent=False):
    """(pairs u32[capacity][2], total) of call(pairs_ptr, capacity, count), one of the adaptors below; capacity None: count first
    (no list), then exact.  The count starts at 0.  The list sits between GUARD guard entries in front and GUARD (plus everything
    past the capacity) behind, which are checked (guard_fault).  absent: the sets hold a vertex count out of range, which every call
    must report through its synchronise."""
    d_cnt = eng.zeros(1, np.uint64)
    if capacity is None:
        call(None, 0, d_cnt)
        synchronize(eng, absent)
        capacity = int(d_cnt.get()[0])
        eng.memset(d_cnt, 0, 8)
    d_buf = eng.empty((capacity + 2 * GUARD, 2), np.uint32)
    eng.memset(d_buf, 0xA5, d_buf.nbytes)
    call(d_buf.ptr + 8 * GUARD, capacity, d_cnt)
    synchronize(eng, absent)
    buf, total = d_buf.get(), int(d_cnt.get()[0])
    d_buf.free()
    d_cnt.free()
    why = guard_fault(buf, capacity)
    assert why is None, why
    return buf[GUARD:GUARD + capacity], total


# ---- one adaptor per entry point: its arguments -> run()'s call(pairs_ptr, capacity, count) --------------------------------------
# Rectangle sets are (the eight plane pointers, n); polygon sets are DeviceSets A, B (the swept search takes their motion planes too).
def rect_cross(eng, pa, n_a, pb, n_b, upper=False, row_base=0, col_base=0):
    return lambda pairs, cap, cnt: eng.sat_rect_cross_pairs(pa, n_a, pb, n_b, pairs, cap, cnt, row_base=row_base, col_base=col_base, upper=upper)


def rect_broad(eng, pa, n_a, pb, n_b, upper=False):
    return lambda pairs, cap, cnt: eng.sat_rect_broad_pairs(pa, n_a, pb, n_b, pairs, cap, cnt, upper=upper)


def poly_cross(eng, A, B, upper=False, row_base=0, col_base=0):
    return lambda pairs, cap, cnt: eng.sat_poly_cross_pairs(A.set, B.set, pairs, cap, cnt, row_base=row_base, col_base=col_base, upper=upper)


def poly_broad(eng, A, B, upper=False):
    return lambda pairs, cap, cnt: eng.sat_poly_broad_pairs(A.set, B.set, pairs, cap, cnt, upper=upper)


def sweep_broad(eng, A, B, upper=False):
    return lambda pairs, cap, cnt: eng.poly_sweep_broad_pairs(A.set, B.set, pairs, cap, cnt, A.motion, B.motion, upper=upper)


def near_broad(eng, A, B, max_dist, upper=False):
    return lambda pairs, cap, cnt: eng.poly_near_broad_pairs(A.set, B.set, max_dist, pairs, cap, cnt, upper=upper)


def same_as(eng, call, ref_call):
    """the list and total of `call` equal those of `ref_call` (a broad-phase search against its cross form), each counted first and
    then listed between guard entries; returns (list, total)"""
    want, wc = run(eng, ref_call)
    got, gc = run(eng, call)
    why = compare(got, gc, want)
    assert why is None and wc == len(want), (why, wc)
    return got, gc


def static_broad(eng, A, B, upper=False):
    """the list of c2d_sat_poly_broad_pairs on the DeviceSets A, B: what the swept and the proximity lists must contain"""
    return run(eng, poly_broad(eng, A, B, upper))[0]
