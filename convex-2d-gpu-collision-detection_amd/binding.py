"""ctypes mirror of include/c2d.h.

Every method maps one-to-one onto a C-ABI entry point; argument names and
meaning follow the header (which cites the reference lines each call replaces).
Device pointers are plain integers, so buffers may come from ``Engine.malloc``
or from any other allocator on the same device (e.g. ``torch.Tensor.data_ptr()``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
KMAX = 16
CROSS_UPPER = 1   # C2D_CROSS_UPPER: N x M calls test only pairs with (col_base + j) > (row_base + i)

POSE_DT = np.dtype([("width", "<f4"), ("height", "<f4"), ("theta", "<f4")])
STD_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("theta", "<f4"), ("width", "<f4"), ("height", "<f4")])
SCENE_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("var_idx", "<f4"), ("pose_idx", "<f4")])
ROW_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("cp", "<f4"), ("var_idx", "<f4"), ("pose_idx", "<f4")])


# polygon Monte-Carlo (include/c2d.h, "Monte-Carlo collision probability for convex polygons")
POLY_DT = np.dtype([("k", "<u4"), ("x", "<f4", (KMAX,)), ("y", "<f4", (KMAX,))])       # c2d_polygon
POLY_POSE_DT = np.dtype([("theta", "<f4"), ("obstacle", POLY_DT)])                       # c2d_poly_pose

# contact queries (include/c2d.h, "contact queries: depth and normal for listed pairs")
CONTACT_DT = np.dtype([("depth", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("axis", "<u2"), ("hit", "u1"), ("flags", "u1")])   # c2d_contact
CONTACT_NO_AXIS, CONTACT_BAD_PAIR = 1, 2

# contact manifolds (include/c2d.h, "contact manifolds: up to two contact points per listed pair")
MANIFOLD_DT = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("d0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("d1", "<f4"), ("feature", "<u2"), ("count", "u1"),
                        ("flags", "u1"), ("reserved", "<u4")])   # c2d_manifold
MANIFOLD_REF_IS_B, MANIFOLD_P0_CLIPPED, MANIFOLD_P1_CLIPPED, MANIFOLD_OUTSIDE_SLAB = 1, 2, 4, 8

# distance queries (include/c2d.h, "distance queries: separation and closest points for listed pairs")
DISTANCE_DT = np.dtype([("dist", "<f4"), ("ax", "<f4"), ("ay", "<f4"), ("bx", "<f4"), ("by", "<f4"), ("edge", "<u2"), ("vert", "<u2"), ("hit", "u1"),
                        ("flags", "u1"), ("reserved0", "<u2"), ("reserved1", "<u4")])   # c2d_distance
DISTANCE_EDGE_ON_B, DISTANCE_INTERIOR, DISTANCE_NO_CANDIDATE, DISTANCE_BAD_PAIR = 1, 2, 4, 8

# overlap queries (include/c2d.h, "overlap queries: area, centroid and IoU of the intersection for listed pairs")
OVERLAP_DT = np.dtype([("area", "<f4"), ("iou", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("area_a", "<f4"), ("area_b", "<f4"), ("hit", "u1"), ("flags", "u1"),
                       ("pieces_a", "u1"), ("pieces_b", "u1"), ("reserved", "<u4")])   # c2d_overlap
OVERLAP_DEGENERATE, OVERLAP_CLAMPED, OVERLAP_NO_CENTROID, OVERLAP_BAD_PAIR = 1, 2, 4, 8

# ray queries (include/c2d.h, "ray queries: the nearest hit of every segment against a polygon set")
RAY_HIT_DT = np.dtype([("poly", "<u4"), ("t", "<f4"), ("u", "<f4"), ("edge", "<u2"), ("hit", "u1"), ("flags", "u1")])   # c2d_ray_hit
RAY_START_INSIDE = 1

# clearance queries (include/c2d.h, "clearance queries: the nearest polygon of a set for every query polygon")
CLEARANCE_DT = np.dtype([("poly", "<u4"), ("dist", "<f4"), ("ax", "<f4"), ("ay", "<f4"), ("bx", "<f4"), ("by", "<f4"), ("edge", "<u2"), ("vert", "<u2"),
                         ("hit", "u1"), ("flags", "u1"), ("reserved0", "<u2")])   # c2d_clearance
CLEARANCE_SKIP_SELF, CLEARANCE_NONE = 1, 16

# swept queries (include/c2d.h, "swept queries: time of impact for listed pairs in linear motion")
SWEEP_DT = np.dtype([("toi", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("axis", "<u2"), ("hit", "u1"), ("flags", "u1")])   # c2d_sweep
SWEEP_START_OVERLAP, SWEEP_BAD_PAIR = 1, 2
# shape casts (include/c2d.h, "shape casts: the first touch of each moving polygon against a set")
CAST_DT = np.dtype([("poly", "<u4"), ("toi", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("axis", "<u2"), ("hit", "u1"), ("flags", "u1"), ("reserved0", "<u4")])   # c2d_cast
CAST_SKIP_SELF = 1


class C2DError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = ""):
        self.status = status
        super().__init__(f"{what}: status {status}" + (f" ({detail})" if detail else ""))


class _Position(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class _Pose(C.Structure):
    _fields_ = [("width", C.c_float), ("height", C.c_float), ("theta", C.c_float)]


class _StdDev(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("theta", C.c_float), ("width", C.c_float), ("height", C.c_float)]


class _DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 64), ("device", C.c_int), ("compute_units", C.c_int),
                ("wavefront_size", C.c_int), ("lds_bytes_per_cu", C.c_int), ("hbm_bytes", C.c_size_t), ("pci_bus_id", C.c_char * 32)]


class _PolyBin(C.Structure):
    _fields_ = [("rows_a", C.c_uint32), ("rows_b", C.c_uint32), ("n", C.c_size_t), ("stride", C.c_size_t),
                ("d_ax", C.c_void_p), ("d_ay", C.c_void_p), ("d_bx", C.c_void_p), ("d_by", C.c_void_p),
                ("d_ka", C.c_void_p), ("d_kb", C.c_void_p), ("d_out", C.c_void_p)]


class _PolySet(C.Structure):
    """c2d_poly_set: one set of convex polygons (one half of the padded pair layout)"""
    _fields_ = [("rows", C.c_uint32), ("n", C.c_size_t), ("stride", C.c_size_t), ("d_vx", C.c_void_p), ("d_vy", C.c_void_p), ("d_k", C.c_void_p)]


class _McScenesArgs(C.Structure):
    _fields_ = [
        ("d_poses", C.c_void_p), ("num_poses", C.c_uint32),
        ("d_std_devs", C.c_void_p), ("num_std_devs", C.c_uint32),
        ("d_scenes", C.c_void_p), ("n_scenes", C.c_size_t),
        ("robot_w", C.c_float), ("robot_h", C.c_float),
        ("accuracy_bins", C.POINTER(C.c_float)), ("bin_accuracy", C.POINTER(C.c_float)),
        ("n_accuracy_bins", C.c_uint32), ("max_samples", C.c_uint32),
        ("seed", C.c_uint64), ("scene_id_base", C.c_uint64),
        ("schedule_small_batch", C.c_uint32), ("schedule_large_batch", C.c_uint32), ("schedule_switch_at", C.c_uint32),
        ("d_hits", C.c_void_p), ("d_n_used", C.c_void_p), ("d_rows", C.c_void_p),
        ("total_samples", C.POINTER(C.c_uint64)), ("iterations", C.POINTER(C.c_uint32)),
    ]


class _Polygon(C.Structure):
    _fields_ = [("k", C.c_uint32), ("x", C.c_float * KMAX), ("y", C.c_float * KMAX)]


class _McPolyScenesArgs(C.Structure):
    _fields_ = [("base", _McScenesArgs), ("robot", C.POINTER(_Polygon)), ("d_poly_poses", C.c_void_p), ("num_poly_poses", C.c_uint32)]


def make_polygon(xs, ys=None) -> _Polygon:
    """A c2d_polygon from vertex coordinates (xs, ys), or from one POLY_DT record."""
    if isinstance(xs, _Polygon):
        return xs
    if ys is None:
        rec = xs
        k = int(rec["k"])
        p = _Polygon()
        p.k = k  # (as given: the library validates it)
        for i in range(KMAX):
            p.x[i], p.y[i] = float(rec["x"][i]), float(rec["y"][i])
        return p
    xs, ys = np.asarray(xs, np.float32), np.asarray(ys, np.float32)
    if not (len(xs) == len(ys) <= KMAX):
        raise ValueError("a polygon has at most %d vertices" % KMAX)
    p = _Polygon()
    p.k = len(xs)
    for i in range(len(xs)):
        p.x[i], p.y[i] = float(xs[i]), float(ys[i])
    return p


def library_path() -> str:
    """lib/libc2d.so next to this file; C2D_LIBRARY overrides it (to try another build of the same C-ABI)."""
    return os.environ.get("C2D_LIBRARY") or os.path.join(_HERE, "lib", "libc2d.so")


_lib: Optional[C.CDLL] = None

# name -> (restype, argtypes); also the list of symbols the header declares
_SIGNATURES = {
    "c2d_version": (C.c_int, []),
    "c2d_status_string": (C.c_char_p, [C.c_int]),
    "c2d_last_error": (C.c_char_p, [C.c_void_p]),
    "c2d_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "c2d_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "c2d_ctx_destroy": (C.c_int, [C.c_void_p]),
    "c2d_ctx_info": (C.c_int, [C.c_void_p, C.POINTER(_DeviceInfo)]),   # (the 0.4 layout: kept for old binaries, not called here)
    "c2d_ctx_info_sized": (C.c_int, [C.c_void_p, C.POINTER(_DeviceInfo), C.c_size_t]),
    "c2d_ctx_check_async": (C.c_int, [C.c_void_p]),
    "c2d_malloc": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "c2d_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c2d_malloc_host": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "c2d_free_host": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c2d_memset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "c2d_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "c2d_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "c2d_stream_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "c2d_stream_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c2d_stream_synchronize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c2d_rects_from_poses": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5 + [C.c_size_t, C.POINTER(C.c_void_p), C.c_void_p]),
    "c2d_sat_rect_pairs_verts": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_sat_rect_pairs_verts_mask": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_sat_rect_pairs_aos": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_sat_rect_pairs_pose": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_sat_rect_pairs_verts_host": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "c2d_sat_rect_pairs_pose_host": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "c2d_sat_rect_cross_mask": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t, C.c_size_t,
                                          C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_sat_rect_cross_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t, C.c_size_t,
                                           C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_sat_rect_broad_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_int,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_sat_poly_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_sat_poly_pairs_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_sat_poly_cross_mask": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_void_p]),
    "c2d_sat_poly_cross_pairs": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p]),
    "c2d_sat_poly_broad_pairs": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_void_p]),
    "c2d_poly_pair_contacts": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                         C.c_void_p, C.c_void_p]),
    "c2d_poly_pair_manifolds": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_rect_pair_contacts": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_poly_pair_distances": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                          C.c_void_p, C.c_void_p]),
    "c2d_rect_pair_distances": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_poly_pair_overlaps": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                         C.c_void_p, C.c_void_p]),
    "c2d_rect_pair_overlaps": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_poly_ray_casts": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(_PolySet), C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_poly_ray_casts_grid": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(_PolySet), C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_poly_ray_casts_grid_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "c2d_poly_set_clearances": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "c2d_poly_pair_sweeps": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_rect_pair_sweeps": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_poly_set_casts": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                     C.c_int, C.c_void_p, C.c_void_p]),
    "c2d_poly_sweep_broad_pairs": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_poly_near_broad_pairs": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_void_p]),
    "c2d_poly_set_clearances_grid": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_float, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p,
                                               C.c_void_p]),
    "c2d_poly_set_clearances_grid_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "c2d_poly_set_casts_grid": (C.c_int, [C.c_void_p, C.POINTER(_PolySet), C.POINTER(_PolySet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "c2d_poly_set_casts_grid_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "c2d_poly_bins_create": (C.c_int, [C.c_void_p, C.POINTER(_PolyBin), C.c_size_t, C.POINTER(C.c_void_p)]),
    "c2d_poly_bins_from_padded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "c2d_poly_bins_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c2d_poly_bins_size": (C.c_size_t, [C.c_void_p]),
    "c2d_poly_bins_pairs": (C.c_size_t, [C.c_void_p]),
    "c2d_poly_bins_bytes": (C.c_size_t, [C.c_void_p]),
    "c2d_poly_bins_get": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_PolyBin)]),
    "c2d_sat_poly_pairs_binned": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_poly_bins_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_philox_normals": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_math_eval": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c2d_mc_pair": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.POINTER(_Position), C.POINTER(_Pose), C.POINTER(_StdDev),
                              C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "c2d_mc_scenes": (C.c_int, [C.c_void_p, C.POINTER(_McScenesArgs), C.c_void_p]),
    "c2d_mc_poly_pair": (C.c_int, [C.c_void_p, C.POINTER(_Polygon), C.POINTER(_Position), C.c_float, C.POINTER(_Polygon), C.POINTER(_StdDev),
                                   C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "c2d_mc_poly_scenes": (C.c_int, [C.c_void_p, C.POINTER(_McPolyScenesArgs), C.c_void_p]),
    "c2d_sample_scenes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                    C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p, C.c_void_p]),
    "c2d_uniform_table_minstd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint64, C.c_void_p]),
    "c2d_sqrt_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "c2d_dist_unique_id": (C.c_int, [C.c_void_p]),
    "c2d_dist_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "c2d_dist_init_file": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_double, C.POINTER(C.c_void_p)]),
    "c2d_dist_rank": (C.c_int, [C.c_void_p]),
    "c2d_dist_world_size": (C.c_int, [C.c_void_p]),
    "c2d_dist_transport": (C.c_char_p, [C.c_void_p]),
    "c2d_dist_rccl_version": (C.c_int, [C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "c2d_dist_all_reduce_sum_u64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "c2d_dist_broadcast_u64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "c2d_dist_barrier": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c2d_dist_stream_synchronize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c2d_dist_timed_out": (C.c_int, [C.c_void_p]),
    "c2d_dist_destroy": (C.c_int, [C.c_void_p]),
    "c2d_calc_slack": (C.c_float, [C.c_uint32, C.c_uint32]),
    "c2d_get_bin": (C.c_int, [C.c_float, C.POINTER(C.c_float), C.c_uint32]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _open_library(path: str) -> C.CDLL:
    if not os.path.exists(path):
        raise C2DError(-3, "libc2d.so not built", f"run `make lib` or __graft_entry__.build(); expected {path}")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library() -> C.CDLL:
    """dlopen lib/libc2d.so and type every entry point.  Raises if the HIP
    library has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        _lib = _open_library(library_path())
    return _lib


class DeviceArray:
    """A device allocation owned by an Engine, with numpy-like metadata."""

    def __init__(self, eng: "Engine", ptr: int, shape, dtype):
        self.eng, self.ptr, self.shape, self.dtype = eng, ptr, tuple(shape), np.dtype(dtype)

    @property
    def nbytes(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    def row(self, i: int) -> int:
        """device pointer of sub-array [i] of a C-contiguous array"""
        inner = int(np.prod(self.shape[1:], dtype=np.int64)) * self.dtype.itemsize
        return self.ptr + i * inner

    def get(self, stream: int = 0) -> np.ndarray:
        return self.eng.to_host(self, stream)

    def free(self):
        if self.ptr:
            self.eng.free(self.ptr)
            self.ptr = 0


DIST_ID_BYTES = 128


class Dist:
    """One c2d_dist: this rank's end of the RCCL communicator that sums the hit counters
    (include/c2d.h, multi-GPU block).  Collective calls: every rank must make them."""

    def __init__(self, eng: "Engine", handle):
        self.eng, self.h = eng, handle

    @property
    def rank(self) -> int:
        return int(self.eng.lib.c2d_dist_rank(self.h))

    @property
    def world_size(self) -> int:
        return int(self.eng.lib.c2d_dist_world_size(self.h))

    @property
    def transport(self) -> str:
        return self.eng.lib.c2d_dist_transport(self.h).decode()

    def all_reduce_sum_u64(self, buf, count: int, stream: int = 0):
        self.eng._check(self.eng.lib.c2d_dist_all_reduce_sum_u64(self.h, C.c_void_p(_ptr_of(buf)), count, C.c_void_p(stream)),
                        "c2d_dist_all_reduce_sum_u64")

    def broadcast_u64(self, buf, count: int, root: int = 0, stream: int = 0):
        self.eng._check(self.eng.lib.c2d_dist_broadcast_u64(self.h, C.c_void_p(_ptr_of(buf)), count, root, C.c_void_p(stream)),
                        "c2d_dist_broadcast_u64")

    def barrier(self, stream: int = 0):
        self.eng._check(self.eng.lib.c2d_dist_barrier(self.h, C.c_void_p(stream)), "c2d_dist_barrier")

    def synchronize(self, stream: int = 0):
        """wait for the collectives queued on `stream` under the watchdog (c2d_dist_stream_synchronize)"""
        self.eng._check(self.eng.lib.c2d_dist_stream_synchronize(self.h, C.c_void_p(stream)), "c2d_dist_stream_synchronize")

    @property
    def timed_out(self) -> bool:
        return bool(self.eng.lib.c2d_dist_timed_out(self.h))

    def close(self):
        if self.h:
            self.eng.lib.c2d_dist_destroy(self.h)
            self.h = None


class PolyBins:
    """One c2d_poly_bins handle: the launch table of a binned polygon batch."""

    def __init__(self, eng: "Engine", handle):
        self.eng, self.h = eng, handle

    def __len__(self) -> int:
        return int(self.eng.lib.c2d_poly_bins_size(self.h))

    @property
    def pairs(self) -> int:
        return int(self.eng.lib.c2d_poly_bins_pairs(self.h))

    @property
    def bytes(self) -> int:
        return int(self.eng.lib.c2d_poly_bins_bytes(self.h))

    def get(self, i: int) -> dict:
        b = _PolyBin()
        self.eng._check(self.eng.lib.c2d_poly_bins_get(self.h, i, C.byref(b)), "c2d_poly_bins_get")
        return {"rows_a": b.rows_a, "rows_b": b.rows_b, "n": b.n, "stride": b.stride, "ax": b.d_ax or 0, "ay": b.d_ay or 0, "bx": b.d_bx or 0,
                "by": b.d_by or 0, "ka": b.d_ka or 0, "kb": b.d_kb or 0, "out": b.d_out or 0}

    def results(self, out, stream: int = 0):
        """results in the order of the padded input (handles made by poly_bins_from_padded)"""
        self.eng._check(self.eng.lib.c2d_poly_bins_results(self.eng.h, self.h, _ptr_of(out), C.c_void_p(stream)), "c2d_poly_bins_results")

    def close(self):
        if self.h:
            self.eng.lib.c2d_poly_bins_destroy(self.eng.h, self.h)
            self.h = None


def _ptr_of(x) -> int:
    if isinstance(x, DeviceArray):
        return x.ptr
    if x is None:
        return 0
    return int(x)


class Engine:
    """One c2d_ctx (one device)."""

    def __init__(self, device: int = 0, lib_path: Optional[str] = None):
        # lib_path: another build of the same C-ABI (validation builds such as lib/libc2d_fmad1.so)
        self.lib = _open_library(lib_path) if lib_path else load_library()
        h = C.c_void_p()
        st = self.lib.c2d_ctx_create(device, C.byref(h))
        if st != 0:
            raise C2DError(st, "c2d_ctx_create", self.lib.c2d_status_string(st).decode())
        self.h = h
        self.device = device

    # -- plumbing -----------------------------------------------------------
    def _check(self, st: int, what: str):
        if st != 0:
            raise C2DError(st, what, self.lib.c2d_last_error(self.h).decode() or self.lib.c2d_status_string(st).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.c2d_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        di = _DeviceInfo()
        self._check(self.lib.c2d_ctx_info_sized(self.h, C.byref(di), C.sizeof(di)), "c2d_ctx_info_sized")   # told how large THIS mirror of the struct is
        return {"name": di.name.decode(), "arch": di.arch.decode(), "device": di.device, "compute_units": di.compute_units,
                "wavefront_size": di.wavefront_size, "lds_bytes_per_cu": di.lds_bytes_per_cu, "hbm_bytes": di.hbm_bytes,
                "pci_bus_id": di.pci_bus_id.decode()}

    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self.lib.c2d_malloc(self.h, C.byref(p), nbytes), "c2d_malloc")
        return p.value or 0

    def free(self, ptr: int):
        self._check(self.lib.c2d_free(self.h, C.c_void_p(ptr)), "c2d_free")

    def memset(self, ptr, value: int, nbytes: int, stream: int = 0):
        self._check(self.lib.c2d_memset(self.h, C.c_void_p(_ptr_of(ptr)), value, nbytes, C.c_void_p(stream)), "c2d_memset")

    def synchronize(self, stream: int = 0):
        self._check(self.lib.c2d_stream_synchronize(self.h, C.c_void_p(stream)), "c2d_stream_synchronize")

    # -- multi-GPU ----------------------------------------------------------
    def dist_rccl_version(self):
        """(ncclGetVersion code, path of the librccl that c2d_dist loaded) — c2d_dist_rccl_version"""
        v = C.c_int(0)
        buf = C.create_string_buffer(1024)
        st = self.lib.c2d_dist_rccl_version(C.byref(v), buf, 1024)
        if st != 0:
            raise C2DError(st, "c2d_dist_rccl_version", self.lib.c2d_status_string(st).decode())
        return int(v.value), buf.value.decode()

    def dist_unique_id(self) -> bytes:
        buf = C.create_string_buffer(DIST_ID_BYTES)
        st = self.lib.c2d_dist_unique_id(buf)
        if st != 0:
            raise C2DError(st, "c2d_dist_unique_id", self.lib.c2d_status_string(st).decode())
        return buf.raw

    def dist_init(self, rank: int, world_size: int, unique_id: bytes) -> Dist:
        if len(unique_id) != DIST_ID_BYTES:
            raise ValueError("the communicator id has 128 bytes")
        h = C.c_void_p()
        buf = C.create_string_buffer(unique_id, DIST_ID_BYTES)
        self._check(self.lib.c2d_dist_init(self.h, rank, world_size, buf, C.byref(h)), "c2d_dist_init")
        return Dist(self, h)

    def dist_init_file(self, rank: int, world_size: int, path: str, timeout_s: float = 300.0) -> Dist:
        h = C.c_void_p()
        self._check(self.lib.c2d_dist_init_file(self.h, rank, world_size, path.encode(), timeout_s, C.byref(h)), "c2d_dist_init_file")
        return Dist(self, h)

    def check_async(self):
        """Raise if a kernel of this ctx reported an argument error since the last check (c2d_ctx_check_async)."""
        self._check(self.lib.c2d_ctx_check_async(self.h), "c2d_ctx_check_async")

    def stream_create(self) -> int:
        s = C.c_void_p()
        self._check(self.lib.c2d_stream_create(self.h, C.byref(s)), "c2d_stream_create")
        return s.value or 0

    def stream_destroy(self, stream: int):
        self._check(self.lib.c2d_stream_destroy(self.h, C.c_void_p(stream)), "c2d_stream_destroy")

    def empty(self, shape, dtype) -> DeviceArray:
        if isinstance(shape, int):
            shape = (shape,)
        a = DeviceArray(self, 0, shape, dtype)
        a.ptr = self.malloc(max(a.nbytes, 1))
        return a

    def zeros(self, shape, dtype, stream: int = 0) -> DeviceArray:
        a = self.empty(shape, dtype)
        self.memset(a.ptr, 0, max(a.nbytes, 1), stream)
        return a

    def to_device(self, host: np.ndarray, stream: int = 0) -> DeviceArray:
        host = np.ascontiguousarray(host)
        a = self.empty(host.shape, host.dtype)
        if host.nbytes:
            self._check(self.lib.c2d_memcpy_h2d(self.h, C.c_void_p(a.ptr), C.c_void_p(host.ctypes.data), host.nbytes,
                                                C.c_void_p(stream)), "c2d_memcpy_h2d")
            self.synchronize(stream)
        return a

    def to_host(self, a: DeviceArray, stream: int = 0) -> np.ndarray:
        out = np.empty(a.shape, a.dtype)
        if out.nbytes:
            self._check(self.lib.c2d_memcpy_d2h(self.h, C.c_void_p(out.ctypes.data), C.c_void_p(a.ptr), out.nbytes,
                                                C.c_void_p(stream)), "c2d_memcpy_d2h")
            self.synchronize(stream)
        return out

    def read(self, ptr: int, shape, dtype, stream: int = 0) -> np.ndarray:
        return self.to_host(DeviceArray(self, ptr, shape, dtype), stream)

    # -- geometry -------------------------------------------------------------
    def rects_from_poses(self, cx, cy, w, h, theta, n: int, out_planes: Sequence, stream: int = 0):
        arr = (C.c_void_p * 8)(*[_ptr_of(p) for p in out_planes])
        self._check(self.lib.c2d_rects_from_poses(self.h, _ptr_of(cx), _ptr_of(cy), _ptr_of(w), _ptr_of(h), _ptr_of(theta),
                                                  n, arr, C.c_void_p(stream)), "c2d_rects_from_poses")

    def sat_rect_pairs_verts(self, planes: Sequence, n: int, out, count=None, stream: int = 0):
        if len(planes) != 16:
            raise ValueError("need 16 vertex planes")
        arr = (C.c_void_p * 16)(*[_ptr_of(p) for p in planes])
        self._check(self.lib.c2d_sat_rect_pairs_verts(self.h, arr, n, _ptr_of(out), _ptr_of(count), C.c_void_p(stream)),
                    "c2d_sat_rect_pairs_verts")

    def sat_rect_pairs_aos(self, r1, r2, n: int, out, count=None, stream: int = 0):
        self._check(self.lib.c2d_sat_rect_pairs_aos(self.h, _ptr_of(r1), _ptr_of(r2), n, _ptr_of(out), _ptr_of(count),
                                                    C.c_void_p(stream)), "c2d_sat_rect_pairs_aos")

    def sat_rect_pairs_verts_mask(self, planes: Sequence, n: int, mask, count=None, stream: int = 0):
        if len(planes) != 16:
            raise ValueError("need 16 vertex planes")
        arr = (C.c_void_p * 16)(*[_ptr_of(p) for p in planes])
        self._check(self.lib.c2d_sat_rect_pairs_verts_mask(self.h, arr, n, _ptr_of(mask), _ptr_of(count), C.c_void_p(stream)),
                    "c2d_sat_rect_pairs_verts_mask")

    # -- the host conveniences of the N x M pair lists ------------------------------------------------------
    def _to_device_all(self, hosts: Sequence) -> list:
        """to_device of every array (None stays None); what was uploaded is freed again if a later upload fails"""
        out = []
        try:
            for x in hosts:
                out.append(None if x is None else self.to_device(x))
        except BaseException:
            for d in out:
                if d is not None:
                    d.free()
            raise
        return out

    def _pairs_sized_exactly(self, name: str, arrays: Sequence, list_call, count_call=None, check_async: bool = False) -> np.ndarray:
        """The one shape of the *_pairs_host functions: count, size the list exactly, list, compare the two totals.
        list_call(pairs, capacity, count) makes the list call; count_call(count) counts another way (default: the list call
        without a buffer).  Frees `arrays` (the caller's uploads; None entries are skipped) and its own on every way out."""
        arrays = [x for x in arrays if x is not None]
        try:
            d_cnt = self.zeros(1, np.uint64)
            arrays.append(d_cnt)
            if count_call is None:
                list_call(None, 0, d_cnt)
            else:
                count_call(d_cnt)
            total = int(d_cnt.get()[0])
            if check_async:
                self.check_async()
            if total == 0:
                return np.zeros((0, 2), np.uint32)
            d_pairs = self.empty((total, 2), np.uint32)
            arrays.append(d_pairs)
            self.memset(d_cnt, 0, 8)
            list_call(d_pairs, total, d_cnt)
            out = d_pairs.get()
            if int(d_cnt.get()[0]) != total:
                raise C2DError(-2, name, "the list call counted a different total than the count-only call" if count_call is None
                               else "the list form counted a different total than the mask form")
            return out
        finally:
            for x in arrays:
                x.free()

    # -- all pairs of two rectangle sets (include/c2d.h "all pairs of two rectangle sets") ------------------
    @staticmethod
    def _cross_planes(a_planes: Sequence, b_planes: Sequence):
        if len(a_planes) != 8 or len(b_planes) != 8:
            raise ValueError("need 8 vertex planes per set")
        return (C.c_void_p * 8)(*[_ptr_of(p) for p in a_planes]), (C.c_void_p * 8)(*[_ptr_of(p) for p in b_planes])

    def sat_rect_cross_mask(self, a_planes: Sequence, n_a: int, b_planes: Sequence, n_b: int, mask, ld_words: Optional[int] = None,
                            row_base: int = 0, col_base: int = 0, upper: bool = False, count=None, stream: int = 0):
        """c2d_sat_rect_cross_mask: bit (j & 63) of mask[i * ld_words + (j >> 6)] = rectangle A_i collides with B_j
        (ld_words defaults to ceil(n_b / 64))"""
        a, b = self._cross_planes(a_planes, b_planes)
        ld = (n_b + 63) // 64 if ld_words is None else ld_words
        self._check(self.lib.c2d_sat_rect_cross_mask(self.h, a, n_a, b, n_b, row_base, col_base, CROSS_UPPER if upper else 0, _ptr_of(mask), ld,
                                                     _ptr_of(count), C.c_void_p(stream)), "c2d_sat_rect_cross_mask")

    def sat_rect_cross_pairs(self, a_planes: Sequence, n_a: int, b_planes: Sequence, n_b: int, pairs, capacity: int, count,
                             row_base: int = 0, col_base: int = 0, upper: bool = False, stream: int = 0):
        """c2d_sat_rect_cross_pairs: the first `capacity` colliding pairs (row_base + i, col_base + j) in row-major order into
        pairs = u32[capacity][2]; count (required) is incremented by the total"""
        a, b = self._cross_planes(a_planes, b_planes)
        self._check(self.lib.c2d_sat_rect_cross_pairs(self.h, a, n_a, b, n_b, row_base, col_base, CROSS_UPPER if upper else 0, _ptr_of(pairs),
                                                      capacity, _ptr_of(count), C.c_void_p(stream)), "c2d_sat_rect_cross_pairs")

    def rect_cross_pairs_host(self, a_planes: np.ndarray, b_planes: np.ndarray, upper: bool = False) -> np.ndarray:
        """Host convenience: a_planes f32[8][n_a], b_planes f32[8][n_b] -> the colliding pairs as an int array [k, 2] in row-major
        order.  Counts with the mask form first, then sizes the list exactly."""
        a_planes, b_planes = np.asarray(a_planes, np.float32), np.asarray(b_planes, np.float32)
        if a_planes.ndim != 2 or b_planes.ndim != 2 or a_planes.shape[0] != 8 or b_planes.shape[0] != 8:
            raise ValueError("need float32 planes [8][n]")
        n_a, n_b = a_planes.shape[1], b_planes.shape[1]
        if n_a == 0 or n_b == 0:
            return np.zeros((0, 2), np.uint32)
        d_a, d_b = self._to_device_all([a_planes, b_planes])
        pa, pb = [d_a.row(k) for k in range(8)], [d_b.row(k) for k in range(8)]

        def count_with_mask(d_cnt):
            d_mask = self.empty((n_a, (n_b + 63) // 64), np.uint64)
            try:
                self.sat_rect_cross_mask(pa, n_a, pb, n_b, d_mask, upper=upper, count=d_cnt)
            finally:
                d_mask.free()

        return self._pairs_sized_exactly("rect_cross_pairs_host", [d_a, d_b],
                                         lambda pairs, cap, cnt: self.sat_rect_cross_pairs(pa, n_a, pb, n_b, pairs, cap, cnt, upper=upper),
                                         count_call=count_with_mask)

    def sat_rect_broad_pairs(self, a_planes: Sequence, n_a: int, b_planes: Sequence, n_b: int, pairs, capacity: int, count,
                             upper: bool = False, stream: int = 0):
        """c2d_sat_rect_broad_pairs: the list of sat_rect_cross_pairs (row_base = col_base = 0) through a broad phase: the first
        `capacity` colliding pairs (i, j) in row-major order into pairs = u32[capacity][2]; count (required) is incremented by
        the total"""
        a, b = self._cross_planes(a_planes, b_planes)
        self._check(self.lib.c2d_sat_rect_broad_pairs(self.h, a, n_a, b, n_b, CROSS_UPPER if upper else 0, _ptr_of(pairs), capacity,
                                                      _ptr_of(count), C.c_void_p(stream)), "c2d_sat_rect_broad_pairs")

    def rect_broad_pairs_host(self, a_planes: np.ndarray, b_planes: Optional[np.ndarray] = None, upper: bool = False) -> np.ndarray:
        """Host convenience: a_planes f32[8][n_a], b_planes f32[8][n_b] (None: the same set, uploaded once) -> the colliding pairs
        as an int array [k, 2] in row-major order.  A count-only call first, then the list sized exactly."""
        a_planes = np.asarray(a_planes, np.float32)
        b_planes = None if b_planes is None else np.asarray(b_planes, np.float32)
        for p in (a_planes, a_planes if b_planes is None else b_planes):
            if p.ndim != 2 or p.shape[0] != 8:
                raise ValueError("need float32 planes [8][n]")
        n_a = a_planes.shape[1]
        n_b = n_a if b_planes is None else b_planes.shape[1]
        if n_a == 0 or n_b == 0:
            return np.zeros((0, 2), np.uint32)
        d_a, d_b = self._to_device_all([a_planes, b_planes])
        pa = [d_a.row(k) for k in range(8)]
        pb = pa if d_b is None else [d_b.row(k) for k in range(8)]
        return self._pairs_sized_exactly("rect_broad_pairs_host", [d_a, d_b],
                                         lambda pairs, cap, cnt: self.sat_rect_broad_pairs(pa, n_a, pb, n_b, pairs, cap, cnt, upper=upper))

    def sat_rect_pairs_pose(self, planes: Sequence, n: int, out, count=None, stream: int = 0):
        if len(planes) != 10:
            raise ValueError("need 10 pose planes")
        arr = (C.c_void_p * 10)(*[_ptr_of(p) for p in planes])
        self._check(self.lib.c2d_sat_rect_pairs_pose(self.h, arr, n, _ptr_of(out), _ptr_of(count), C.c_void_p(stream)),
                    "c2d_sat_rect_pairs_pose")

    def sat_rect_pairs_host(self, planes, out: np.ndarray, fmt: str = "verts") -> int:
        """c2d_sat_rect_pairs_verts_host / _pose_host: planes = 16 (10) host pointers or 1-D float32 arrays of n elements each, out = host u8[n]
        (numpy arrays or the arrays of host_empty()); returns the number of colliding pairs"""
        want = 16 if fmt == "verts" else 10
        if len(planes) != want:
            raise ValueError("need %d planes" % want)
        n = out.shape[0]
        ptrs = [(p.ctypes.data if isinstance(p, np.ndarray) else int(p)) for p in planes]
        arr = (C.c_void_p * want)(*ptrs)
        cnt = C.c_ulonglong(0)
        fn = self.lib.c2d_sat_rect_pairs_verts_host if fmt == "verts" else self.lib.c2d_sat_rect_pairs_pose_host
        self._check(fn(self.h, arr, n, C.c_void_p(out.ctypes.data), C.byref(cnt)), "c2d_sat_rect_pairs_%s_host" % fmt)
        return int(cnt.value)

    def host_empty(self, shape, dtype) -> np.ndarray:
        """a numpy array in page-locked host memory (c2d_malloc_host); free it with host_free(array)"""
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        p = C.c_void_p()
        self._check(self.lib.c2d_malloc_host(self.h, C.byref(p), max(nbytes, 1)), "c2d_malloc_host")
        buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        if p:
            self._check(self.lib.c2d_free_host(self.h, C.c_void_p(p)), "c2d_free_host")

    def sat_poly_pairs_rows(self, vx, vy, k, n: int, rows: int, out, count=None, stream: int = 0):
        self._check(self.lib.c2d_sat_poly_pairs_rows(self.h, _ptr_of(vx), _ptr_of(vy), _ptr_of(k), n, rows, _ptr_of(out), _ptr_of(count),
                                                     C.c_void_p(stream)), "c2d_sat_poly_pairs_rows")

    def sat_poly_pairs(self, vx, vy, k, n: int, out, count=None, stream: int = 0):
        self._check(self.lib.c2d_sat_poly_pairs(self.h, _ptr_of(vx), _ptr_of(vy), _ptr_of(k), n, _ptr_of(out), _ptr_of(count),
                                                C.c_void_p(stream)), "c2d_sat_poly_pairs")

    # -- all pairs of two convex polygon sets (include/c2d.h "all pairs of two convex polygon sets") ----------
    @staticmethod
    def poly_set(vx, vy, k, n: int, rows: int = KMAX, stride: int = 0) -> _PolySet:
        """A c2d_poly_set from device pointers (or DeviceArrays): vx, vy f32[rows][stride], k u8[n] or None (every polygon has
        `rows` vertices); stride 0 = n"""
        return _PolySet(rows, n, stride, _ptr_of(vx), _ptr_of(vy), _ptr_of(k))

    def sat_poly_cross_mask(self, a: _PolySet, b: _PolySet, mask, ld_words: Optional[int] = None, row_base: int = 0, col_base: int = 0,
                            upper: bool = False, count=None, stream: int = 0):
        """c2d_sat_poly_cross_mask: bit (j & 63) of mask[i * ld_words + (j >> 6)] = polygon A_i collides with B_j
        (ld_words defaults to ceil(n_b / 64)); a, b from poly_set()"""
        ld = (b.n + 63) // 64 if ld_words is None else ld_words
        self._check(self.lib.c2d_sat_poly_cross_mask(self.h, C.byref(a), C.byref(b), row_base, col_base, CROSS_UPPER if upper else 0, _ptr_of(mask), ld,
                                                     _ptr_of(count), C.c_void_p(stream)), "c2d_sat_poly_cross_mask")

    def sat_poly_cross_pairs(self, a: _PolySet, b: _PolySet, pairs, capacity: int, count, row_base: int = 0, col_base: int = 0,
                             upper: bool = False, stream: int = 0):
        """c2d_sat_poly_cross_pairs: the first `capacity` colliding pairs (row_base + i, col_base + j) in row-major order into
        pairs = u32[capacity][2]; count (required) is incremented by the total"""
        self._check(self.lib.c2d_sat_poly_cross_pairs(self.h, C.byref(a), C.byref(b), row_base, col_base, CROSS_UPPER if upper else 0, _ptr_of(pairs),
                                                      capacity, _ptr_of(count), C.c_void_p(stream)), "c2d_sat_poly_cross_pairs")

    @staticmethod
    def _host_poly_set(vx, vy, k):
        vx, vy = np.asarray(vx, np.float32), np.asarray(vy, np.float32)
        if vx.ndim != 2 or vx.shape != vy.shape or not 1 <= vx.shape[0] <= KMAX:
            raise ValueError("need float32 vertex planes vx, vy [rows][n] of one shape, 1 <= rows <= %d" % KMAX)
        if k is not None:
            k = np.asarray(k)
            if k.shape != (vx.shape[1],):
                raise ValueError("need vertex counts k [n] for planes [rows][n]")
            k = k.astype(np.uint8)
        return vx, vy, k

    def poly_cross_pairs_host(self, vx_a, vy_a, k_a, vx_b, vy_b, k_b, upper: bool = False) -> np.ndarray:
        """Host convenience: vx, vy f32[rows][n] and k u8[n] (or None) per set -> the colliding pairs as u32 [total][2] in row-major
        order.  A count-only call first, then the list sized exactly."""
        vx_a, vy_a, k_a = self._host_poly_set(vx_a, vy_a, k_a)
        vx_b, vy_b, k_b = self._host_poly_set(vx_b, vy_b, k_b)
        n_a, n_b = vx_a.shape[1], vx_b.shape[1]
        if n_a == 0 or n_b == 0:
            return np.zeros((0, 2), np.uint32)
        arrays = self._to_device_all([vx_a, vy_a, k_a, vx_b, vy_b, k_b])
        a = self.poly_set(*arrays[:3], n_a, vx_a.shape[0])
        b = self.poly_set(*arrays[3:], n_b, vx_b.shape[0])
        return self._pairs_sized_exactly("poly_cross_pairs_host", arrays,
                                         lambda pairs, cap, cnt: self.sat_poly_cross_pairs(a, b, pairs, cap, cnt, upper=upper), check_async=True)

    def sat_poly_broad_pairs(self, a: _PolySet, b: _PolySet, pairs, capacity: int, count, upper: bool = False, stream: int = 0):
        """c2d_sat_poly_broad_pairs: the list of sat_poly_cross_pairs (row_base = col_base = 0) through a broad phase: the first
        `capacity` colliding pairs (i, j) in row-major order into pairs = u32[capacity][2]; count (required) is incremented by
        the total; a, b from poly_set() (the same set twice: boxes and sort are made once)"""
        if not isinstance(a, _PolySet) or not isinstance(b, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        self._check(self.lib.c2d_sat_poly_broad_pairs(self.h, C.byref(a), C.byref(b), CROSS_UPPER if upper else 0, _ptr_of(pairs), capacity,
                                                      _ptr_of(count), C.c_void_p(stream)), "c2d_sat_poly_broad_pairs")

    def poly_broad_pairs_host(self, vx_a, vy_a, k_a, vx_b=None, vy_b=None, k_b=None, upper: bool = False) -> np.ndarray:
        """Host convenience: vx, vy f32[rows][n] and k u8[n] (or None) per set (vx_b None: the same set, uploaded once) -> the
        colliding pairs as u32 [total][2] in row-major order.  A count-only call first, then the list sized exactly."""
        vx_a, vy_a, k_a = self._host_poly_set(vx_a, vy_a, k_a)
        same = vx_b is None
        if same:
            if vy_b is not None or k_b is not None:
                raise ValueError("set B needs vx_b and vy_b (or none of vx_b, vy_b, k_b: the same set)")
        else:
            if vy_b is None:
                raise ValueError("set B needs vx_b and vy_b")
            vx_b, vy_b, k_b = self._host_poly_set(vx_b, vy_b, k_b)
        n_a = vx_a.shape[1]
        n_b = n_a if same else vx_b.shape[1]
        if n_a == 0 or n_b == 0:
            return np.zeros((0, 2), np.uint32)
        arrays = self._to_device_all([vx_a, vy_a, k_a] + ([] if same else [vx_b, vy_b, k_b]))
        a = self.poly_set(*arrays[:3], n_a, vx_a.shape[0])
        b = a if same else self.poly_set(*arrays[3:], n_b, vx_b.shape[0])
        return self._pairs_sized_exactly("poly_broad_pairs_host", arrays,
                                         lambda pairs, cap, cnt: self.sat_poly_broad_pairs(a, b, pairs, cap, cnt, upper=upper), check_async=True)

    # -- contact queries (include/c2d.h "contact queries: depth and normal for listed pairs") -----------------
    def poly_pair_contacts(self, a: _PolySet, b: _PolySet, pairs, n_pairs: int, out, n_pairs_dev=None, row_base: int = 0, col_base: int = 0,
                           stream: int = 0):
        """c2d_poly_pair_contacts: out[p] (CONTACT_DT[n_pairs], 16-byte aligned) = the contact of list entry p = (row_base + i,
        col_base + j) of pairs = u32[n_pairs][2]; with n_pairs_dev (a device u64, the count a list call filled) only the first
        min(n_pairs, *n_pairs_dev) entries are processed and nothing beyond them is touched; a, b from poly_set()"""
        if not isinstance(a, _PolySet) or not isinstance(b, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        self._check(self.lib.c2d_poly_pair_contacts(self.h, C.byref(a), C.byref(b), _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base, col_base,
                                                    _ptr_of(out), C.c_void_p(stream)), "c2d_poly_pair_contacts")

    def rect_pair_contacts(self, a_planes: Sequence, n_a: int, b_planes: Sequence, n_b: int, pairs, n_pairs: int, out, n_pairs_dev=None,
                           row_base: int = 0, col_base: int = 0, stream: int = 0):
        """c2d_rect_pair_contacts: poly_pair_contacts for two rectangle sets given as 8 vertex planes each"""
        a, b = self._cross_planes(a_planes, b_planes)
        self._check(self.lib.c2d_rect_pair_contacts(self.h, a, n_a, b, n_b, _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base, col_base,
                                                    _ptr_of(out), C.c_void_p(stream)), "c2d_rect_pair_contacts")

    def poly_pair_manifolds(self, a: _PolySet, b: _PolySet, pairs, n_pairs: int, contacts, manifolds, n_pairs_dev=None, row_base: int = 0,
                            col_base: int = 0, stream: int = 0):
        """c2d_poly_pair_manifolds: poly_pair_contacts into contacts[p] (CONTACT_DT[n_pairs]) and, in the same device call, the
        manifold of list entry p into manifolds[p] (MANIFOLD_DT[n_pairs]); both outputs required and 16-byte aligned"""
        if not isinstance(a, _PolySet) or not isinstance(b, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        self._check(self.lib.c2d_poly_pair_manifolds(self.h, C.byref(a), C.byref(b), _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base, col_base,
                                                     _ptr_of(contacts), _ptr_of(manifolds), C.c_void_p(stream)), "c2d_poly_pair_manifolds")

    # -- distance queries (include/c2d.h "distance queries: separation and closest points for listed pairs") -----------------
    def poly_pair_distances(self, a: _PolySet, b: _PolySet, pairs, n_pairs: int, out, n_pairs_dev=None, row_base: int = 0, col_base: int = 0,
                            stream: int = 0):
        """c2d_poly_pair_distances: out[p] (DISTANCE_DT[n_pairs], 16-byte aligned) = the pairwise boolean of list entry p and, when it
        is not hit, the distance of the two polygons with its two closest points; the list, n_pairs_dev and the bases as for
        poly_pair_contacts"""
        if not isinstance(a, _PolySet) or not isinstance(b, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        self._check(self.lib.c2d_poly_pair_distances(self.h, C.byref(a), C.byref(b), _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base, col_base,
                                                     _ptr_of(out), C.c_void_p(stream)), "c2d_poly_pair_distances")

    def rect_pair_distances(self, a_planes: Sequence, n_a: int, b_planes: Sequence, n_b: int, pairs, n_pairs: int, out, n_pairs_dev=None,
                            row_base: int = 0, col_base: int = 0, stream: int = 0):
        """c2d_rect_pair_distances: poly_pair_distances for two rectangle sets given as 8 vertex planes each"""
        a, b = self._cross_planes(a_planes, b_planes)
        self._check(self.lib.c2d_rect_pair_distances(self.h, a, n_a, b, n_b, _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base, col_base,
                                                     _ptr_of(out), C.c_void_p(stream)), "c2d_rect_pair_distances")

    # -- overlap queries (include/c2d.h "overlap queries: area, centroid and IoU of the intersection for listed pairs") -----------------
    def poly_pair_overlaps(self, a: _PolySet, b: _PolySet, pairs, n_pairs: int, out, n_pairs_dev=None, row_base: int = 0, col_base: int = 0,
                           stream: int = 0):
        """c2d_poly_pair_overlaps: out[p] (OVERLAP_DT[n_pairs], 16-byte aligned) = the pairwise boolean of list entry p and, when it
        is hit, the area of the intersection of the two polygons with its centroid, their own areas and the IoU; the list,
        n_pairs_dev and the bases as for poly_pair_contacts"""
        if not isinstance(a, _PolySet) or not isinstance(b, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        self._check(self.lib.c2d_poly_pair_overlaps(self.h, C.byref(a), C.byref(b), _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base, col_base,
                                                    _ptr_of(out), C.c_void_p(stream)), "c2d_poly_pair_overlaps")

    def rect_pair_overlaps(self, a_planes: Sequence, n_a: int, b_planes: Sequence, n_b: int, pairs, n_pairs: int, out, n_pairs_dev=None,
                           row_base: int = 0, col_base: int = 0, stream: int = 0):
        """c2d_rect_pair_overlaps: poly_pair_overlaps for two rectangle sets given as 8 vertex planes each"""
        a, b = self._cross_planes(a_planes, b_planes)
        self._check(self.lib.c2d_rect_pair_overlaps(self.h, a, n_a, b, n_b, _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base, col_base,
                                                    _ptr_of(out), C.c_void_p(stream)), "c2d_rect_pair_overlaps")

    # -- ray queries (include/c2d.h "ray queries: the nearest hit of every segment against a polygon set") -----------------
    def poly_ray_casts(self, rays: Sequence, n_rays: int, b: _PolySet, out, col_base: int = 0, stream: int = 0):
        """c2d_poly_ray_casts: out[r] (RAY_HIT_DT[n_rays], 16-byte aligned) = the first polygon of b that the segment from
        (ox, oy)[r] to (ox + dx, oy + dy)[r] touches, with t, the edge and u; rays = the four planes ox, oy, dx, dy (f32[n_rays]
        each); b from poly_set(); a hit reports col_base + j"""
        if rays is None or len(rays) != 4:
            raise ValueError("need the four ray planes ox, oy, dx, dy")
        if not isinstance(b, _PolySet):
            raise ValueError("need a poly_set() description")
        planes = (C.c_void_p * 4)(*[_ptr_of(p) for p in rays])
        self._check(self.lib.c2d_poly_ray_casts(self.h, planes, n_rays, C.byref(b), col_base, _ptr_of(out), C.c_void_p(stream)), "c2d_poly_ray_casts")

    def poly_ray_casts_grid(self, rays: Sequence, n_rays: int, b: _PolySet, out, col_base: int = 0, stream: int = 0):
        """c2d_poly_ray_casts_grid: poly_ray_casts through a uniform grid over b, for many polygons and short segments; per ray the
        pick of poly_ray_casts among the polygons whose vertex box the ray meets (include/c2d.h "ray queries through a grid").
        Uses the ctx scratch."""
        if rays is None or len(rays) != 4:
            raise ValueError("need the four ray planes ox, oy, dx, dy")
        if not isinstance(b, _PolySet):
            raise ValueError("need a poly_set() description")
        planes = (C.c_void_p * 4)(*[_ptr_of(p) for p in rays])
        self._check(self.lib.c2d_poly_ray_casts_grid(self.h, planes, n_rays, C.byref(b), col_base, _ptr_of(out), C.c_void_p(stream)),
                    "c2d_poly_ray_casts_grid")

    def poly_ray_casts_grid_stats(self) -> dict:
        """c2d_poly_ray_casts_grid_stats: the counters of the last poly_ray_casts_grid call with polygons (synchronise first)"""
        out = (C.c_ulonglong * 4)()
        self._check(self.lib.c2d_poly_ray_casts_grid_stats(self.h, out), "c2d_poly_ray_casts_grid_stats")
        return {"listed": int(out[0]), "visited": int(out[1]), "candidates": int(out[2]), "outliers": int(out[3])}

    # -- clearance queries (include/c2d.h "clearance queries: the nearest polygon of a set for every query polygon") -----------------
    def poly_set_clearances(self, a_set: _PolySet, b_set: _PolySet, d_out, row_base: int = 0, col_base: int = 0, flags: int = 0, stream: int = 0):
        """c2d_poly_set_clearances: d_out[i] (CLEARANCE_DT[n_a], 16-byte aligned) = the polygon of b_set nearest to polygon i of a_set by
        the distance contract, as col_base + j, with that pair's distance record; a_set, b_set from poly_set() (they may describe the
        same memory); flags: 0 or CLEARANCE_SKIP_SELF (the pair with row_base + i == col_base + j is not considered)"""
        if not isinstance(a_set, _PolySet) or not isinstance(b_set, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        if d_out is None:
            raise ValueError("need an output of CLEARANCE_DT[n_a]")
        if isinstance(d_out, DeviceArray) and d_out.nbytes < CLEARANCE_DT.itemsize * a_set.n:
            raise ValueError("the output holds fewer than n_a records")
        if row_base < 0 or col_base < 0 or flags & ~CLEARANCE_SKIP_SELF:
            raise ValueError("bases are not negative, and flags is 0 or CLEARANCE_SKIP_SELF")
        self._check(self.lib.c2d_poly_set_clearances(self.h, C.byref(a_set), C.byref(b_set), row_base, col_base, flags, _ptr_of(d_out), C.c_void_p(stream)),
                    "c2d_poly_set_clearances")

    def poly_set_clearances_grid(self, a_set: _PolySet, b_set: _PolySet, max_dist: float, d_out, row_base: int = 0, col_base: int = 0, flags: int = 0,
                                 stream: int = 0):
        """c2d_poly_set_clearances_grid: poly_set_clearances among the polygons of b_set that are hit or no farther than max_dist (finite,
        0 <= max_dist < 2^60), found through the grid of the pair searches; a query with nothing within max_dist gets the
        CLEARANCE_NONE record.  d_out: CLEARANCE_DT[n_a], 16-byte aligned; flags: 0 or CLEARANCE_SKIP_SELF"""
        if not isinstance(a_set, _PolySet) or not isinstance(b_set, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        if d_out is None:
            raise ValueError("need an output of CLEARANCE_DT[n_a]")
        if isinstance(d_out, DeviceArray) and d_out.nbytes < CLEARANCE_DT.itemsize * a_set.n:
            raise ValueError("the output holds fewer than n_a records")
        if row_base < 0 or col_base < 0 or flags & ~CLEARANCE_SKIP_SELF:
            raise ValueError("bases are not negative, and flags is 0 or CLEARANCE_SKIP_SELF")
        self._check(self.lib.c2d_poly_set_clearances_grid(self.h, C.byref(a_set), C.byref(b_set), C.c_float(max_dist), row_base, col_base, flags,
                                                          _ptr_of(d_out), C.c_void_p(stream)), "c2d_poly_set_clearances_grid")

    def poly_set_clearances_grid_stats(self) -> dict:
        """c2d_poly_set_clearances_grid_stats: the counters of the last poly_set_clearances_grid call with obstacles (synchronise first)"""
        out = (C.c_ulonglong * 5)()
        self._check(self.lib.c2d_poly_set_clearances_grid_stats(self.h, out), "c2d_poly_set_clearances_grid_stats")
        return {"listed": int(out[0]), "walked": int(out[1]), "candidates": int(out[2]), "tested": int(out[3]), "walks": int(out[4])}

    # -- swept queries (include/c2d.h "swept queries: time of impact for listed pairs in linear motion") -----------------
    @staticmethod
    def _motion(motion, which: str):
        """a set's motion -> its two plane pointers: None (the set stands still) or the pair (dx, dy) of device f32[n] planes"""
        if motion is None:
            return None, None
        if isinstance(motion, (str, bytes)) or not hasattr(motion, "__len__") or len(motion) != 2 or motion[0] is None or motion[1] is None:
            raise ValueError(f"{which}_motion is None or the two planes (dx, dy)")
        return _ptr_of(motion[0]), _ptr_of(motion[1])

    def poly_pair_sweeps(self, a: _PolySet, b: _PolySet, pairs, n_pairs: int, out, a_motion=None, b_motion=None, n_pairs_dev=None, row_base: int = 0,
                         col_base: int = 0, stream: int = 0):
        """c2d_poly_pair_sweeps: out[p] (SWEEP_DT[n_pairs], 16-byte aligned) = whether the two polygons of list entry p touch while
        both translate over the step t = 0 .. 1, the first time they do and the normal from A to B there; a_motion / b_motion: the
        pair (dx, dy) of device planes f32[n] of a set's displacements, or None for a set that stands still; the list, n_pairs_dev
        and the bases as for poly_pair_contacts"""
        if not isinstance(a, _PolySet) or not isinstance(b, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        adx, ady = self._motion(a_motion, "a")
        bdx, bdy = self._motion(b_motion, "b")
        self._check(self.lib.c2d_poly_pair_sweeps(self.h, C.byref(a), C.byref(b), adx, ady, bdx, bdy, _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base,
                                                  col_base, _ptr_of(out), C.c_void_p(stream)), "c2d_poly_pair_sweeps")

    def rect_pair_sweeps(self, a_planes: Sequence, n_a: int, b_planes: Sequence, n_b: int, pairs, n_pairs: int, out, a_motion=None, b_motion=None,
                         n_pairs_dev=None, row_base: int = 0, col_base: int = 0, stream: int = 0):
        """c2d_rect_pair_sweeps: poly_pair_sweeps for two rectangle sets given as 8 vertex planes each"""
        a, b = self._cross_planes(a_planes, b_planes)
        adx, ady = self._motion(a_motion, "a")
        bdx, bdy = self._motion(b_motion, "b")
        self._check(self.lib.c2d_rect_pair_sweeps(self.h, a, n_a, b, n_b, adx, ady, bdx, bdy, _ptr_of(pairs), n_pairs, _ptr_of(n_pairs_dev), row_base,
                                                  col_base, _ptr_of(out), C.c_void_p(stream)), "c2d_rect_pair_sweeps")

    # -- shape casts (include/c2d.h "shape casts: the first touch of each moving polygon against a set") -----------------
    def poly_set_casts(self, a_set: _PolySet, b_set: _PolySet, a_motion=None, b_motion=None, row_base: int = 0, col_base: int = 0, flags: int = 0, out=None,
                       stream: int = 0):
        """c2d_poly_set_casts: out[i] (CAST_DT[n_a], 8-byte aligned) = the polygon of b_set that polygon i of a_set touches first while
        both translate over the step t = 0 .. 1, as col_base + j, with that pair's sweep record; a_set, b_set from poly_set() (they
        may describe the same memory); a_motion / b_motion as for poly_pair_sweeps: None or the pair (dx, dy) of device planes f32[n];
        flags: 0 or CAST_SKIP_SELF (the pair with row_base + i == col_base + j is not considered)"""
        if not isinstance(a_set, _PolySet) or not isinstance(b_set, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        if out is None:
            raise ValueError("need an output of CAST_DT[n_a]")
        if isinstance(out, DeviceArray) and out.nbytes < CAST_DT.itemsize * a_set.n:
            raise ValueError("the output holds fewer than n_a records")
        if row_base < 0 or col_base < 0 or flags & ~CAST_SKIP_SELF:
            raise ValueError("bases are not negative, and flags is 0 or CAST_SKIP_SELF")
        adx, ady = self._motion(a_motion, "a")
        bdx, bdy = self._motion(b_motion, "b")
        self._check(self.lib.c2d_poly_set_casts(self.h, C.byref(a_set), C.byref(b_set), adx, ady, bdx, bdy, row_base, col_base, flags, _ptr_of(out),
                                                C.c_void_p(stream)), "c2d_poly_set_casts")

    def poly_set_casts_grid(self, a_set: _PolySet, b_set: _PolySet, a_motion=None, b_motion=None, row_base: int = 0, col_base: int = 0, flags: int = 0,
                            out=None, stream: int = 0):
        """c2d_poly_set_casts_grid: poly_set_casts found through the grid of the pair searches on swept boxes; the arguments and the
        output are those of poly_set_casts, byte for byte (out: CAST_DT[n_a], 8-byte aligned; flags: 0 or CAST_SKIP_SELF).  The same
        set twice with the same motion planes: boxes and sort are made once"""
        if not isinstance(a_set, _PolySet) or not isinstance(b_set, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        if out is None:
            raise ValueError("need an output of CAST_DT[n_a]")
        if isinstance(out, DeviceArray) and out.nbytes < CAST_DT.itemsize * a_set.n:
            raise ValueError("the output holds fewer than n_a records")
        if row_base < 0 or col_base < 0 or flags & ~CAST_SKIP_SELF:
            raise ValueError("bases are not negative, and flags is 0 or CAST_SKIP_SELF")
        adx, ady = self._motion(a_motion, "a")
        bdx, bdy = self._motion(b_motion, "b")
        self._check(self.lib.c2d_poly_set_casts_grid(self.h, C.byref(a_set), C.byref(b_set), adx, ady, bdx, bdy, row_base, col_base, flags, _ptr_of(out),
                                                     C.c_void_p(stream)), "c2d_poly_set_casts_grid")

    def poly_set_casts_grid_stats(self) -> dict:
        """c2d_poly_set_casts_grid_stats: the counters of the last poly_set_casts_grid call with obstacles (synchronise first)"""
        out = (C.c_ulonglong * 5)()
        self._check(self.lib.c2d_poly_set_casts_grid_stats(self.h, out), "c2d_poly_set_casts_grid_stats")
        return {"listed": int(out[0]), "walked": int(out[1]), "candidates": int(out[2]), "walks": int(out[3])}

    # -- swept broad phase (include/c2d.h "swept broad-phase pair search of two convex polygon sets") -----------------
    def poly_sweep_broad_pairs(self, a: _PolySet, b: _PolySet, pairs, capacity: int, count, a_motion=None, b_motion=None, upper: bool = False,
                               stream: int = 0):
        """c2d_poly_sweep_broad_pairs: every pair (i, j) whose poly_pair_sweeps record has hit == 1 (row_base = col_base = 0), found
        through the broad phase on swept boxes: the first `capacity` pairs in row-major order into pairs = u32[capacity][2]; count
        (required) is incremented by the total; a, b from poly_set(); a_motion / b_motion as for poly_pair_sweeps: None or the pair
        (dx, dy) of device planes f32[n] (the same set twice with the same planes: boxes and sort are made once)"""
        if not isinstance(a, _PolySet) or not isinstance(b, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        adx, ady = self._motion(a_motion, "a")
        bdx, bdy = self._motion(b_motion, "b")
        self._check(self.lib.c2d_poly_sweep_broad_pairs(self.h, C.byref(a), C.byref(b), adx, ady, bdx, bdy, CROSS_UPPER if upper else 0, _ptr_of(pairs),
                                                        capacity, _ptr_of(count), C.c_void_p(stream)), "c2d_poly_sweep_broad_pairs")

    @staticmethod
    def _host_motion(motion, n: int, which: str):
        if motion is None:
            return None
        if isinstance(motion, (str, bytes)) or not hasattr(motion, "__len__") or len(motion) != 2:
            raise ValueError(f"{which}_motion is None or the two planes (dx, dy)")
        dx, dy = np.ascontiguousarray(motion[0], np.float32), np.ascontiguousarray(motion[1], np.float32)
        if dx.shape != (n,) or dy.shape != (n,):
            raise ValueError(f"{which}_motion needs two planes f32[{n}]")
        return dx, dy

    def poly_sweep_broad_pairs_host(self, vx_a, vy_a, k_a, a_motion=None, vx_b=None, vy_b=None, k_b=None, b_motion=None, upper: bool = False) -> np.ndarray:
        """Host convenience: vx, vy f32[rows][n], k u8[n] (or None) and a motion (None, or the two planes dx, dy f32[n]) per set
        (vx_b None: the same set with the same motion, uploaded once) -> the pairs that touch during the step as u32 [total][2] in
        row-major order.  A count-only call first, then the list sized exactly."""
        vx_a, vy_a, k_a = self._host_poly_set(vx_a, vy_a, k_a)
        same = vx_b is None
        if same:
            if vy_b is not None or k_b is not None or b_motion is not None:
                raise ValueError("set B needs vx_b and vy_b (or none of vx_b, vy_b, k_b, b_motion: the same set)")
        else:
            if vy_b is None:
                raise ValueError("set B needs vx_b and vy_b")
            vx_b, vy_b, k_b = self._host_poly_set(vx_b, vy_b, k_b)
        n_a = vx_a.shape[1]
        n_b = n_a if same else vx_b.shape[1]
        mot_a = self._host_motion(a_motion, n_a, "a")
        mot_b = None if same else self._host_motion(b_motion, n_b, "b")
        if n_a == 0 or n_b == 0:
            return np.zeros((0, 2), np.uint32)
        host = [vx_a, vy_a, k_a] + ([] if same else [vx_b, vy_b, k_b])
        n_sets = len(host)
        host += list(mot_a or ()) + list(mot_b or ())
        arrays = self._to_device_all(host)
        a = self.poly_set(*arrays[:3], n_a, vx_a.shape[0])
        b = a if same else self.poly_set(*arrays[3:6], n_b, vx_b.shape[0])
        d_mot_a = tuple(arrays[n_sets:n_sets + 2]) if mot_a else None
        d_mot_b = d_mot_a if same else (tuple(arrays[-2:]) if mot_b else None)
        return self._pairs_sized_exactly("poly_sweep_broad_pairs_host", arrays,
                                         lambda pairs, cap, cnt: self.poly_sweep_broad_pairs(a, b, pairs, cap, cnt, d_mot_a, d_mot_b, upper=upper),
                                         check_async=True)

    # -- proximity pair search (include/c2d.h "proximity pair search of two convex polygon sets: every pair within a distance") ---------
    def poly_near_broad_pairs(self, a: _PolySet, b: _PolySet, max_dist: float, pairs, capacity: int, count, upper: bool = False, stream: int = 0):
        """c2d_poly_near_broad_pairs: every pair (i, j) whose poly_pair_distances record has hit == 1 or dist <= max_dist (row_base =
        col_base = 0), found through the broad phase on boxes that hold the margin: the first `capacity` pairs in row-major order into
        pairs = u32[capacity][2]; count (required) is incremented by the total; a, b from poly_set() (the same set twice: boxes and
        sort are made once); max_dist: finite, 0 <= max_dist < 2^60"""
        if not isinstance(a, _PolySet) or not isinstance(b, _PolySet):
            raise ValueError("need two poly_set() descriptions")
        self._check(self.lib.c2d_poly_near_broad_pairs(self.h, C.byref(a), C.byref(b), C.c_float(max_dist), CROSS_UPPER if upper else 0, _ptr_of(pairs),
                                                       capacity, _ptr_of(count), C.c_void_p(stream)), "c2d_poly_near_broad_pairs")

    def poly_near_broad_pairs_host(self, vx_a, vy_a, k_a, max_dist: float, vx_b=None, vy_b=None, k_b=None, upper: bool = False) -> np.ndarray:
        """Host convenience: vx, vy f32[rows][n] and k u8[n] (or None) per set (vx_b None: the same set, uploaded once) -> the pairs
        that are hit or within max_dist as u32 [total][2] in row-major order.  A count-only call first, then the list sized exactly."""
        vx_a, vy_a, k_a = self._host_poly_set(vx_a, vy_a, k_a)
        same = vx_b is None
        if same:
            if vy_b is not None or k_b is not None:
                raise ValueError("set B needs vx_b and vy_b (or none of vx_b, vy_b, k_b: the same set)")
        else:
            if vy_b is None:
                raise ValueError("set B needs vx_b and vy_b")
            vx_b, vy_b, k_b = self._host_poly_set(vx_b, vy_b, k_b)
        n_a = vx_a.shape[1]
        n_b = n_a if same else vx_b.shape[1]
        if n_a == 0 or n_b == 0:
            return np.zeros((0, 2), np.uint32)
        arrays = self._to_device_all([vx_a, vy_a, k_a] + ([] if same else [vx_b, vy_b, k_b]))
        a = self.poly_set(*arrays[:3], n_a, vx_a.shape[0])
        b = a if same else self.poly_set(*arrays[3:], n_b, vx_b.shape[0])
        return self._pairs_sized_exactly("poly_near_broad_pairs_host", arrays,
                                         lambda pairs, cap, cnt: self.poly_near_broad_pairs(a, b, max_dist, pairs, cap, cnt, upper=upper),
                                         check_async=True)

    def _contacts_of_list(self, name: str, arrays: Sequence, list_call, contacts_call, check_async: bool = False, manifolds: bool = False):
        """The one shape of the *_contacts_host functions: a count-only list call sizes the buffers, then the list call and the
        contacts call run back to back on the list's DEVICE count (no read-back between them).  list_call(pairs, capacity, count),
        contacts_call(pairs, capacity, count, out).  Frees `arrays` and its own on every way out.  -> (pairs, contacts)
        manifolds: contacts_call(pairs, capacity, count, out, manifolds_out) fills a second output; -> (pairs, contacts, manifolds)"""
        arrays = [x for x in arrays if x is not None]
        try:
            d_cnt = self.zeros(1, np.uint64)
            arrays.append(d_cnt)
            list_call(None, 0, d_cnt)
            total = int(d_cnt.get()[0])
            if check_async:
                self.check_async()
            if total == 0:
                return (np.zeros((0, 2), np.uint32), np.zeros(0, CONTACT_DT)) + ((np.zeros(0, MANIFOLD_DT),) if manifolds else ())
            d_pairs, d_out = self.empty((total, 2), np.uint32), self.empty(total, CONTACT_DT)
            arrays += [d_pairs, d_out]
            outs = [d_out]
            if manifolds:
                outs.append(self.empty(total, MANIFOLD_DT))
                arrays.append(outs[1])
            self.memset(d_cnt, 0, 8)
            list_call(d_pairs, total, d_cnt)
            contacts_call(d_pairs, total, d_cnt, *outs)
            got = (d_pairs.get(),) + tuple(x.get() for x in outs)
            if int(d_cnt.get()[0]) != total:
                raise C2DError(-2, name, "the list call counted a different total than the count-only call")
            return got
        finally:
            for x in arrays:
                x.free()

    def poly_contacts_host(self, vx_a, vy_a, k_a, vx_b=None, vy_b=None, k_b=None, upper: bool = False, broad: bool = True):
        """Host convenience: the sets of poly_broad_pairs_host (vx_b None: the same set) -> (pairs u32 [total][2], contacts
        CONTACT_DT[total]): the colliding pairs through the broad phase (broad=False: the N x M list) and their contacts, computed
        on the list's device count."""
        return self._poly_contacts_host("poly_contacts_host", False, vx_a, vy_a, k_a, vx_b, vy_b, k_b, upper, broad)

    def poly_manifolds_host(self, vx_a, vy_a, k_a, vx_b=None, vy_b=None, k_b=None, upper: bool = False, broad: bool = True):
        """Host convenience: poly_contacts_host through c2d_poly_pair_manifolds -> (pairs u32 [total][2], contacts CONTACT_DT[total],
        manifolds MANIFOLD_DT[total])."""
        return self._poly_contacts_host("poly_manifolds_host", True, vx_a, vy_a, k_a, vx_b, vy_b, k_b, upper, broad)

    def _poly_contacts_host(self, name: str, manifolds: bool, vx_a, vy_a, k_a, vx_b, vy_b, k_b, upper: bool, broad: bool):
        vx_a, vy_a, k_a = self._host_poly_set(vx_a, vy_a, k_a)
        same = vx_b is None
        if same:
            if vy_b is not None or k_b is not None:
                raise ValueError("set B needs vx_b and vy_b (or none of vx_b, vy_b, k_b: the same set)")
        else:
            if vy_b is None:
                raise ValueError("set B needs vx_b and vy_b")
            vx_b, vy_b, k_b = self._host_poly_set(vx_b, vy_b, k_b)
        n_a = vx_a.shape[1]
        n_b = n_a if same else vx_b.shape[1]
        if n_a == 0 or n_b == 0:
            return (np.zeros((0, 2), np.uint32), np.zeros(0, CONTACT_DT)) + ((np.zeros(0, MANIFOLD_DT),) if manifolds else ())
        arrays = self._to_device_all([vx_a, vy_a, k_a] + ([] if same else [vx_b, vy_b, k_b]))
        a = self.poly_set(*arrays[:3], n_a, vx_a.shape[0])
        b = a if same else self.poly_set(*arrays[3:], n_b, vx_b.shape[0])
        lister = self.sat_poly_broad_pairs if broad else self.sat_poly_cross_pairs
        call = self.poly_pair_manifolds if manifolds else self.poly_pair_contacts
        return self._contacts_of_list(name, arrays, lambda pairs, cap, cnt: lister(a, b, pairs, cap, cnt, upper=upper),
                                      lambda pairs, cap, cnt, *outs: call(a, b, pairs, cap, *outs, n_pairs_dev=cnt), check_async=True, manifolds=manifolds)

    def rect_contacts_host(self, a_planes: np.ndarray, b_planes: Optional[np.ndarray] = None, upper: bool = False, broad: bool = True):
        """Host convenience: the sets of rect_broad_pairs_host (b_planes None: the same set) -> (pairs u32 [total][2], contacts
        CONTACT_DT[total]), through the broad phase (broad=False: the N x M list) and the contacts call on the list's device count."""
        a_planes = np.asarray(a_planes, np.float32)
        b_planes = None if b_planes is None else np.asarray(b_planes, np.float32)
        for p in (a_planes, a_planes if b_planes is None else b_planes):
            if p.ndim != 2 or p.shape[0] != 8:
                raise ValueError("need float32 planes [8][n]")
        n_a = a_planes.shape[1]
        n_b = n_a if b_planes is None else b_planes.shape[1]
        if n_a == 0 or n_b == 0:
            return np.zeros((0, 2), np.uint32), np.zeros(0, CONTACT_DT)
        d_a, d_b = self._to_device_all([a_planes, b_planes])
        pa = [d_a.row(k) for k in range(8)]
        pb = pa if d_b is None else [d_b.row(k) for k in range(8)]
        lister = self.sat_rect_broad_pairs if broad else self.sat_rect_cross_pairs
        return self._contacts_of_list("rect_contacts_host", [d_a, d_b], lambda pairs, cap, cnt: lister(pa, n_a, pb, n_b, pairs, cap, cnt, upper=upper),
                                      lambda pairs, cap, cnt, out: self.rect_pair_contacts(pa, n_a, pb, n_b, pairs, cap, out, n_pairs_dev=cnt))

    # -- binned polygon batches (include/c2d.h "binned polygon batches") ---------------
    def poly_bins_create(self, bins) -> "PolyBins":
        """bins: sequence of dicts with rows_a, rows_b, n, ax, ay, bx, by, out and optionally ka, kb, stride
        (device pointers or DeviceArrays)."""
        arr = (_PolyBin * max(len(bins), 1))()
        for i, b in enumerate(bins):
            arr[i] = _PolyBin(b["rows_a"], b["rows_b"], b["n"], b.get("stride", 0), _ptr_of(b["ax"]), _ptr_of(b["ay"]), _ptr_of(b["bx"]),
                              _ptr_of(b["by"]), _ptr_of(b.get("ka")), _ptr_of(b.get("kb")), _ptr_of(b["out"]))
        h = C.c_void_p()
        self._check(self.lib.c2d_poly_bins_create(self.h, arr, len(bins), C.byref(h)), "c2d_poly_bins_create")
        return PolyBins(self, h)

    def poly_bins_from_padded(self, vx, vy, k, n: int, rows: int, granularity: int, stream: int = 0) -> "PolyBins":
        h = C.c_void_p()
        st = self.lib.c2d_poly_bins_from_padded(self.h, _ptr_of(vx), _ptr_of(vy), _ptr_of(k), n, rows, granularity, C.byref(h), C.c_void_p(stream))
        if st != 0:
            if h.value:
                self.lib.c2d_poly_bins_destroy(self.h, h)
            self._check(st, "c2d_poly_bins_from_padded")
        return PolyBins(self, h)

    def sat_poly_pairs_binned(self, bins: "PolyBins", count=None, stream: int = 0):
        self._check(self.lib.c2d_sat_poly_pairs_binned(self.h, bins.h, _ptr_of(count), C.c_void_p(stream)), "c2d_sat_poly_pairs_binned")

    # -- random stream / Monte-Carlo ------------------------------------------------
    def philox_normals(self, seed: int, scene_id: int, sample_begin: int, n: int, normals, raw=None, stream: int = 0):
        self._check(self.lib.c2d_philox_normals(self.h, seed, scene_id, sample_begin, n, _ptr_of(normals), _ptr_of(raw),
                                                C.c_void_p(stream)), "c2d_philox_normals")

    MATH_LOG, MATH_SINCOS, MATH_SINCOS_U32, MATH_SQRT, MATH_BOX_MULLER = range(5)

    def math_eval(self, fn: int, in_bits, n: int, out0, out1=None, stream: int = 0):
        self._check(self.lib.c2d_math_eval(self.h, fn, _ptr_of(in_bits), n, _ptr_of(out0), _ptr_of(out1), C.c_void_p(stream)),
                    "c2d_math_eval")

    def mc_pair(self, robot_w, robot_h, pos, pose, std_dev, seed, scene_id, sample_begin, n_samples, hits, stream: int = 0):
        self._check(self.lib.c2d_mc_pair(self.h, robot_w, robot_h, C.byref(_Position(*pos)), C.byref(_Pose(*pose)),
                                         C.byref(_StdDev(*std_dev)), seed, scene_id, sample_begin, n_samples,
                                         _ptr_of(hits), C.c_void_p(stream)), "c2d_mc_pair")

    @staticmethod
    def _mc_scenes_args(poses, num_poses, std_devs, num_std_devs, scenes, n_scenes, robot_w, robot_h, accuracy_bins, bin_accuracy,
                        max_samples, seed, scene_id_base, schedule, hits, n_used, rows, host_outputs: bool):
        """-> (c2d_mc_scenes_args, total, iters): the argument block of the adaptive entry points, with the two host outputs
        behind it when host_outputs (NULL otherwise: the loop is only enqueued).  The block keeps what it points to alive."""
        bins = np.ascontiguousarray(accuracy_bins, dtype=np.float32)
        acc = np.ascontiguousarray(bin_accuracy, dtype=np.float32)
        if len(acc) != len(bins) - 1:
            raise ValueError("bin_accuracy must have len(accuracy_bins) - 1 entries")
        total, iters = C.c_uint64(0), C.c_uint32(0)
        a = _McScenesArgs(_ptr_of(poses), num_poses, _ptr_of(std_devs), num_std_devs, _ptr_of(scenes), n_scenes, robot_w,
                          robot_h, bins.ctypes.data_as(C.POINTER(C.c_float)), acc.ctypes.data_as(C.POINTER(C.c_float)),
                          len(bins), max_samples, seed, scene_id_base, schedule[0], schedule[1], schedule[2],
                          _ptr_of(hits), _ptr_of(n_used), _ptr_of(rows),
                          C.pointer(total) if host_outputs else None, C.pointer(iters) if host_outputs else None)
        a.keep_alive = (bins, acc)
        return a, total, iters

    def mc_scenes(self, poses, num_poses, std_devs, num_std_devs, scenes, n_scenes, robot_w, robot_h, accuracy_bins,
                  bin_accuracy, max_samples, seed, scene_id_base, hits, n_used, rows=None, stream: int = 0,
                  schedule=(0, 0, 0)):
        a, total, iters = self._mc_scenes_args(poses, num_poses, std_devs, num_std_devs, scenes, n_scenes, robot_w, robot_h, accuracy_bins,
                                               bin_accuracy, max_samples, seed, scene_id_base, schedule, hits, n_used, rows, True)
        self._check(self.lib.c2d_mc_scenes(self.h, C.byref(a), C.c_void_p(stream)), "c2d_mc_scenes")
        return int(total.value), int(iters.value)

    def mc_scenes_async(self, poses, num_poses, std_devs, num_std_devs, scenes, n_scenes, robot_w, robot_h, accuracy_bins,
                        bin_accuracy, max_samples, seed, scene_id_base, hits, n_used, rows=None, stream: int = 0,
                        schedule=(0, 0, 0)):
        """c2d_mc_scenes without host outputs: the whole adaptive loop is only enqueued (no synchronisation)."""
        a, _, _ = self._mc_scenes_args(poses, num_poses, std_devs, num_std_devs, scenes, n_scenes, robot_w, robot_h, accuracy_bins,
                                       bin_accuracy, max_samples, seed, scene_id_base, schedule, hits, n_used, rows, False)
        self._check(self.lib.c2d_mc_scenes(self.h, C.byref(a), C.c_void_p(stream)), "c2d_mc_scenes")

    def mc_poly_pair(self, robot, pos, robot_theta, obstacle, std_dev, seed, scene_id, sample_begin, n_samples, hits, stream: int = 0):
        """robot, obstacle: (xs, ys) tuples, POLY_DT records or make_polygon() results"""
        r = make_polygon(*robot) if isinstance(robot, tuple) else make_polygon(robot)
        o = make_polygon(*obstacle) if isinstance(obstacle, tuple) else make_polygon(obstacle)
        self._check(self.lib.c2d_mc_poly_pair(self.h, C.byref(r), C.byref(_Position(*pos)), robot_theta, C.byref(o), C.byref(_StdDev(*std_dev)),
                                              seed, scene_id, sample_begin, n_samples, _ptr_of(hits), C.c_void_p(stream)), "c2d_mc_poly_pair")

    def mc_poly_scenes(self, robot, poly_poses, num_poly_poses, std_devs, num_std_devs, scenes, n_scenes, accuracy_bins, bin_accuracy, max_samples,
                       seed, scene_id_base, hits, n_used, rows=None, stream: int = 0, schedule=(0, 0, 0), host_outputs: bool = True):
        """c2d_mc_poly_scenes; with host_outputs=False the loop is only enqueued (no synchronisation) and None is returned"""
        base, total, iters = self._mc_scenes_args(None, 0, std_devs, num_std_devs, scenes, n_scenes, 0.0, 0.0, accuracy_bins, bin_accuracy,
                                                  max_samples, seed, scene_id_base, schedule, hits, n_used, rows, host_outputs)
        r = None if robot is None else (make_polygon(*robot) if isinstance(robot, tuple) else make_polygon(robot))
        a = _McPolyScenesArgs(base, C.pointer(r) if r is not None else None, _ptr_of(poly_poses), num_poly_poses)
        self._check(self.lib.c2d_mc_poly_scenes(self.h, C.byref(a), C.c_void_p(stream)), "c2d_mc_poly_scenes")
        return (int(total.value), int(iters.value)) if host_outputs else None

    def sample_scenes(self, poses, num_poses, std_devs, num_std_devs, robot_w, robot_h, spread, seed, scene_id_base,
                      n_scenes, scenes, stream: int = 0):
        self._check(self.lib.c2d_sample_scenes(self.h, _ptr_of(poses), num_poses, _ptr_of(std_devs), num_std_devs, robot_w,
                                               robot_h, spread, seed, scene_id_base, n_scenes, _ptr_of(scenes),
                                               C.c_void_p(stream)), "c2d_sample_scenes")

    def uniform_table_minstd(self, out, rows: int, dims: int, lo, hi, first_draw: int = 0, stream: int = 0):
        lo_, hi_ = np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(hi, dtype=np.float32)
        self._check(self.lib.c2d_uniform_table_minstd(self.h, _ptr_of(out), rows, dims, lo_.ctypes.data_as(C.POINTER(C.c_float)),
                                                      hi_.ctypes.data_as(C.POINTER(C.c_float)), first_draw, C.c_void_p(stream)), "c2d_uniform_table_minstd")

    def sqrt_f32(self, src, dst, n: int, stream: int = 0):
        self._check(self.lib.c2d_sqrt_f32(self.h, _ptr_of(src), _ptr_of(dst), n, C.c_void_p(stream)), "c2d_sqrt_f32")

    def calc_slack(self, n: int, k: int) -> float:
        return float(self.lib.c2d_calc_slack(n, k))

    def get_bin(self, p: float, bins) -> int:
        b = np.ascontiguousarray(bins, dtype=np.float32)
        return int(self.lib.c2d_get_bin(p, b.ctypes.data_as(C.POINTER(C.c_float)), len(b)))
