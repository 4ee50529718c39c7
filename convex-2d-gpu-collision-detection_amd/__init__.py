"""convex-2d-gpu-collision-detection_amd — MI355X-native batched 2D SAT collision engine.

The product is ``lib/libc2d.so`` (hand-written HIP for gfx950 behind the C-ABI of
``include/c2d.h``) plus the C++ host drivers in ``csrc/``.  This Python package is
only the thin ctypes mirror of that C-ABI used by the test-suite and ``bench.py``;
it holds no compute of its own and raises if the HIP library is missing — there is
no CPU fallback.

The directory name contains hyphens (it is the reference's repository name), so
load it with ``__graft_entry__.load_package()`` rather than a plain ``import``.
"""
from .binding import (  # noqa: F401
    C2DError,
    Engine,
    Dist,
    PolyBins,
    DeviceArray,
    KMAX,
    CROSS_UPPER,
    POSE_DT,
    STD_DT,
    SCENE_DT,
    ROW_DT,
    POLY_DT,
    POLY_POSE_DT,
    CONTACT_DT,
    MANIFOLD_DT,
    MANIFOLD_REF_IS_B,
    MANIFOLD_P0_CLIPPED,
    MANIFOLD_P1_CLIPPED,
    MANIFOLD_OUTSIDE_SLAB,
    DISTANCE_DT,
    DISTANCE_EDGE_ON_B,
    DISTANCE_INTERIOR,
    DISTANCE_NO_CANDIDATE,
    DISTANCE_BAD_PAIR,
    OVERLAP_DT,
    OVERLAP_DEGENERATE,
    OVERLAP_CLAMPED,
    OVERLAP_NO_CENTROID,
    OVERLAP_BAD_PAIR,
    RAY_HIT_DT,
    RAY_START_INSIDE,
    CLEARANCE_DT,
    CLEARANCE_SKIP_SELF,
    CLEARANCE_NONE,
    SWEEP_DT,
    SWEEP_START_OVERLAP,
    SWEEP_BAD_PAIR,
    CAST_DT,
    CAST_SKIP_SELF,
    make_polygon,
    library_path,
    load_library,
)
