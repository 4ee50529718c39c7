"""GPU tests of the contact queries where the kernel's first pass decides (c2d_contact.hip FastPick): pairs whose
two best axes are not parallel and 2^-26 .. 2^-15 apart, batches scaled across the edges of the first pass's window, eleven
scales side by side in every wave, and a list long enough for a second trip of the grid-stride loop.  As in test_gpu_contacts.py
every field of every contact is compared with tests/contact_ref.py (floats bit for bit) behind guard bands, and `hit` also with the
oracle and the pairwise GPU path.  tests/test_contact_near_ties_cpu.py holds the conditions on these inputs."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases as cases  # noqa: E402
import contact_ref as ref  # noqa: E402
import contact_bands as ties  # noqa: E402
import pair_list_harness as h  # noqa: E402   (the upload, run() with its guard bands, the comparisons)

pytestmark = pytest.mark.gpu
FUZZ_SEED = 20262
Q = h.CONTACTS


def assert_same_by_band(got, want, terms, what):
    ok = ref.same(got, want)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        gap = ties.relative_gap({f: terms[f][q:q + 1] for f in terms})
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(want)} contacts differ; first at {q}, relative gap of its two best axes "
                             f"{gap[0]:.3e} (band {ties.BAND_NAMES[int(ties.band_of(gap)[0])]}): got {got[q]}, want {want[q]}; "
                             f"o {terms['o'][q][terms['usable'][q]]}, len2 {terms['len2'][q][terms['usable'][q]]}, d {terms['d'][q][terms['usable'][q]]}")


def test_near_ties(eng, oracle):
    """The three near-tie batches: polygons and boxes (as 4-gons) through the polygon call, boxes and quads through the rectangle
    call; each as the diagonal list and as the same list in a fixed shuffled order (a wave then mixes all bands and its rows change)."""
    pa, pb = cases.near_tie_poly_sets()
    (ba, bb), (bra, brb) = cases.near_tie_box_sets()
    qa, qb = cases.near_tie_quad_sets()
    for name, a, b in (("polygons", pa, pb), ("boxes as 4-gons", ba, bb)):
        n = a[0].shape[1]
        pairs = h.diag(n)
        idx = np.arange(n)
        want, terms = ref.poly_contacts(a, b, idx, idx), ref.poly_axis_terms(a, b, idx, idx)
        assert np.array_equal(want["hit"], h.oracle_hits(oracle, a, b, pairs))
        ua, ub = h.Uploaded(eng, a), h.Uploaded(eng, b)
        got = Q.run(eng, Q.poly_call(eng, ua.set, ub.set), pairs)
        assert_same_by_band(got, want, terms, name)
        assert np.array_equal(got["hit"], h.pairwise_gpu(eng, a, b, pairs)), name
        order = np.random.default_rng(8301).permutation(n)
        got = Q.run(eng, Q.poly_call(eng, ua.set, ub.set), pairs[order])
        assert_same_by_band(got, want[order], {f: terms[f][order] for f in terms}, name + ", shuffled")
        ua.free()
        ub.free()
    for name, a, b in (("boxes", bra, brb), ("quads", qa, qb)):
        n = a.shape[1]
        pairs = h.diag(n)
        idx = np.arange(n)
        want, terms = ref.rect_contacts(a, b, idx, idx), ref.rect_axis_terms(a, b, idx, idx)
        assert np.array_equal(want["hit"], oracle.sat_rect_pairs_verts(np.concatenate([a, b]))[0])
        da, db = h.RectsOnDevice(eng, a), h.RectsOnDevice(eng, b)
        got = Q.run(eng, Q.rect_call(eng, da, db), pairs)
        assert_same_by_band(got, want, terms, name)
        assert np.array_equal(got["hit"], h.rect_pairwise_gpu(eng, a, b, pairs)), name
        order = np.random.default_rng(8302).permutation(n)
        got = Q.run(eng, Q.rect_call(eng, da, db), pairs[order])
        assert_same_by_band(got, want[order], {f: terms[f][order] for f in terms}, name + ", shuffled")
        da.free()
        db.free()
    eng.check_async()


def assert_same_by_scale(got, want, k, what):
    ok = ref.same(got, want)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(want)} contacts differ, at scales 2^k for k in {sorted(set(k[~ok].tolist()))}; "
                             f"first at {q} (k = {int(k[q])}): got {got[q]}, want {want[q]}")


def test_window_edges(eng, oracle, wl):
    """The 48 x 48 polygon batch of the hard inputs and 200 rectangles per set, multiplied exactly by 2^k for k in -54 .. -46,
    26 .. 32 and 46 .. 54: len2 crosses 2^-100 and 2^100 and |o| crosses 2^60 pair by pair (the CPU file asserts the shares)."""
    a, b, pairs, k = cases.window_edge_poly_batch(wl)
    want = ref.poly_contacts(a, b, *h.local(pairs))
    ua, ub = h.Uploaded(eng, a), h.Uploaded(eng, b)
    got = Q.run(eng, Q.poly_call(eng, ua.set, ub.set), pairs)
    ua.free()
    ub.free()
    assert_same_by_scale(got, want, k, "polygons")
    assert np.array_equal(got["hit"], h.oracle_hits(oracle, a, b, pairs))
    assert np.array_equal(got["hit"], h.pairwise_gpu(eng, a, b, pairs))
    ra, rb, pairs, k = cases.window_edge_rect_batch(oracle, wl)
    i, j = h.local(pairs)
    want = ref.rect_contacts(ra, rb, i, j)
    da, db = h.RectsOnDevice(eng, ra), h.RectsOnDevice(eng, rb)
    got = Q.run(eng, Q.rect_call(eng, da, db), pairs)
    da.free()
    db.free()
    assert_same_by_scale(got, want, k, "rectangles")
    assert np.array_equal(got["hit"], oracle.sat_rect_pairs_verts(np.concatenate([ra[:, i], rb[:, j]]))[0])
    assert np.array_equal(got["hit"], h.rect_pairwise_gpu(eng, ra, rb, pairs))
    eng.check_async()


def test_mixed_scales_in_one_wave(eng, oracle, wl):
    """Polygon i of both sets carries the scale 2^k_i, k_i cycling through 0, 29, 30, 49, 50, 51, -49, -50, -51, 60, -60: lanes
    decided by the first pass, lanes at the window's edges and hard lanes sit side by side in every wave.  The whole list, then
    the list cut by the device count five entries into a wave, for eleven waves: the lanes beyond the count compute the pair of the
    wave's first lane, which is of each of the eleven kinds in turn."""
    a, b, pairs, k = cases.mixed_scale_poly_batch(wl)
    want = ref.poly_contacts(a, b, *h.local(pairs))
    ua, ub = h.Uploaded(eng, a), h.Uploaded(eng, b)
    got = Q.run(eng, Q.poly_call(eng, ua.set, ub.set), pairs)
    assert_same_by_scale(got, want, k, "mixed scales")
    assert np.array_equal(got["hit"], h.oracle_hits(oracle, a, b, pairs))
    assert np.array_equal(got["hit"], h.pairwise_gpu(eng, a, b, pairs))
    waves = 64 * np.arange(1, (len(pairs) - 5) // 64)
    assert set(k[waves].tolist()) == set(cases.MIXED_SCALE_K), "a scale begins no wave of the list: the cut lists below would miss it"
    starts = [int(waves[k[waves] == kk][0]) for kk in cases.MIXED_SCALE_K]      # per kind, the first wave that begins with it
    for s in starts:
        got = Q.run(eng, Q.poly_call(eng, ua.set, ub.set), pairs, n_dev=int(s) + 5)
        assert_same_by_scale(got[:s + 5], want[:s + 5], k[:s + 5], f"mixed scales, device count {s + 5}")
    ua.free()
    ub.free()
    eng.check_async()


def test_list_longer_than_one_grid(eng, oracle, wl):
    """2^24 + 197 entries (a 4099-entry mixed list of the rectangle batch, tiled): the launch is capped at 65 536 blocks of 256, so
    the last 197 entries are the second trip of the grid-stride loop.  Once without a device count, once with 2^24 + 70: the
    127 records beyond it keep the band bytes (run() checks them).  The whole output is compared."""
    ra, rb = cases.rect_sets(oracle, wl)
    mixed = cases.all_pairs(500, 500)[::41][:4099]
    want = ref.rect_contacts(ra, rb, *h.local(mixed))
    assert len(mixed) == 4099 and 0.02 < want["hit"].mean() < 0.5
    total = (1 << 24) + 197
    tile = np.arange(total) % 4099
    listed = mixed[tile]
    want32 = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
    da, db = h.RectsOnDevice(eng, ra), h.RectsOnDevice(eng, rb)
    for n_dev in (None, (1 << 24) + 70):
        bound = total if n_dev is None else n_dev
        got = Q.run(eng, Q.rect_call(eng, da, db), listed, n_dev=n_dev)[:bound]
        got32 = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
        whole = bound // 4099 * 4099
        differs = np.concatenate([(got32[:whole].reshape(-1, 4099, 4) != want32[None]).any(axis=2).ravel(),
                                  (got32[whole:] != want32[:bound - whole]).any(axis=1)])
        at = np.flatnonzero(differs)        # not the same bytes: +0 against -0 is still the same contact
        if len(at):
            ok = ref.same(got[at], want[tile[at]])
            assert ok.all(), (f"device count {n_dev}: {int((~ok).sum())} of {bound} contacts differ; first at entry {int(at[~ok][0])}: "
                              f"got {got[at[~ok][0]]}, want {want[tile[at[~ok][0]]]}")
    da.free()
    db.free()
    eng.check_async()


def test_fuzzer_configurations_at_a_fixed_seed(eng):
    """tests/tools/contact_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations, among
    them near-tied polygons and near-tied quads at power-of-two scales (the fuzzer draws those one time in five)."""
    spec = importlib.util.spec_from_file_location("contact_fuzz", os.path.join(HERE, "tools", "contact_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    seen, compared = [], 0
    for i in range(16):
        ok, (desc, bound) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i)
        assert ok, desc
        seen.append(desc)
        compared += bound
    assert any("near-ties, polygons" in d for d in seen) and any("near-ties, quads" in d for d in seen), seen
    assert compared > 1000
    eng.check_async()
