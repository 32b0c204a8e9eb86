"""Mesh extraction, the Python host: the grid and the mesh of Context.sdf_grid / extract_mesh / mesh_from_values
(include/hip_raymarch.h "mesh extraction"), and writers for the two formats other tools read."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from . import abi


class Grid:
    """`n` = (nx, ny, nz) CELLS between the corners `lo` and `hi`: an axis has n + 1 corners.  Checked as the library checks an RmGrid.
    slabs=True lifts the bound of 2^28 corners, and nothing else: such a grid is for extract_mesh / mesh_from_values with `slabs`
    (include/hip_raymarch.h "slabbed extraction")."""

    def __init__(self, lo, hi, n, slabs=False):
        self.slabs = bool(slabs)
        self.lo, self.hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        self.n = tuple(int(v) for v in n)
        if not (len(self.lo) == len(self.hi) == len(self.n) == 3):
            raise ValueError("grid: lo, hi and n take three values each")
        if any(isinstance(v, bool) or int(v) != v for v in n):
            raise ValueError("grid: n must be integers")
        if not all(1 <= v <= 1024 for v in self.n):
            raise ValueError("grid: n must be in 1..1024 cells per axis")
        f = np.float32
        with np.errstate(all="ignore"):
            h = [(f(b) - f(a)) / f(k) for a, b, k in zip(self.lo, self.hi, self.n)]
        if not all(math.isfinite(f(v)) for v in self.lo + self.hi) or not all(math.isfinite(v) and v > 0 for v in h):
            raise ValueError("grid: lo, hi and the cell size (hi - lo) / n must be finite, the cell size > 0")
        if not self.slabs and self.corners > 1 << 28:
            raise ValueError("grid: at most 2^28 corners")

    @property
    def shape(self):
        """Of the corner values: (nz + 1, ny + 1, nx + 1), x fastest."""
        return (self.n[2] + 1, self.n[1] + 1, self.n[0] + 1)

    @property
    def corners(self) -> int:
        return (self.n[0] + 1) * (self.n[1] + 1) * (self.n[2] + 1)

    @property
    def cells(self) -> int:
        return self.n[0] * self.n[1] * self.n[2]

    def to_c(self) -> abi.RmGrid:
        return abi.RmGrid(lo=(abi.C.c_float * 3)(*self.lo), hi=(abi.C.c_float * 3)(*self.hi), n=(abi.C.c_int32 * 3)(*self.n), reserved=0)

    def axis(self, a: int) -> np.ndarray:
        """The n[a] + 1 corner coordinates of axis a (rm_grid_axis: the library's host arithmetic)."""
        from . import native

        out = np.empty(self.n[a] + 1, np.float32)
        g = self.to_c()
        if self.slabs:  # (rm_grid_axis keeps the bound on the corners; an axis depends on nothing but itself)
            for other in range(3):
                if other != int(a):
                    g.n[other] = 1
        if native.load_library().rm_grid_axis(abi.C.byref(g), int(a), native._fp(out)) != abi.RM_OK:
            raise ValueError("grid: refused by rm_grid_axis")
        return out


def mesh_params(iso=0.0, normals=True, colours=False, flags=0, normal_delta=1e-5) -> abi.RmMeshParams:
    """The abi.RmMeshParams of an extraction, checked as the library checks it: ValueError otherwise."""
    for name, v in (("iso", iso), ("normal_delta", normal_delta)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"mesh: {name} must be a number")
    if not math.isfinite(np.float32(iso)):
        raise ValueError("mesh: iso must be finite")
    for name, v in (("normals", normals), ("colours", colours)):
        if not (isinstance(v, (bool, int, np.integer)) and int(v) in (0, 1)):
            raise ValueError(f"mesh: {name} must be True or False")
    if normals and not (math.isfinite(np.float32(normal_delta)) and np.float32(normal_delta) > 0):
        raise ValueError("mesh: normal_delta must be finite and > 0")
    if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or int(flags) & ~(abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL):
        raise ValueError("mesh: flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both")
    return abi.RmMeshParams(iso=float(iso), normals=int(normals), normal_delta=float(normal_delta), colours=int(colours), flags=int(flags), reserved=0)


def mesh_sharp(**fields) -> abi.RmMeshSharp:
    """The abi.RmMeshSharp of Context.extract_mesh(..., sharp=...), over abi.MESH_SHARP_DEFAULTS: refine (bisection rounds per edge crossing,
    0..16), normal_delta (the step of the normals at the crossings, > 0) and threshold (eigenvalues at or below threshold * the largest are
    dropped from the QEF, in [0, 1)).  Checked as the library checks it: ValueError otherwise, and for unknown keys."""
    unknown = set(fields) - set(abi.MESH_SHARP_DEFAULTS)
    if unknown:
        raise ValueError(f"mesh: unknown sharp parameter {sorted(unknown)[0]}")
    p = {**abi.MESH_SHARP_DEFAULTS, **fields}
    refine = p["refine"]
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= int(refine) <= 16:
        raise ValueError("mesh: sharp refine must be an integer in 0..16")
    for name in ("normal_delta", "threshold"):
        if isinstance(p[name], bool) or not isinstance(p[name], (int, float, np.integer, np.floating)):
            raise ValueError(f"mesh: sharp {name} must be a number")
    with np.errstate(over="ignore"):
        delta, threshold = np.float32(p["normal_delta"]), np.float32(p["threshold"])
    if not (math.isfinite(delta) and delta > 0):
        raise ValueError("mesh: sharp normal_delta must be finite and > 0")
    if not (math.isfinite(threshold) and 0 <= threshold < 1):
        raise ValueError("mesh: sharp threshold must be finite and in [0, 1)")
    return abi.RmMeshSharp(refine=int(refine), normal_delta=float(p["normal_delta"]), threshold=float(p["threshold"]), reserved=0)


def mesh_slabs(layers=0) -> abi.RmMeshSlabs:
    """The abi.RmMeshSlabs of Context.extract_mesh(..., slabs=...) / mesh_from_values(..., slabs=...): the cell layers per slab, 0 = chosen by
    the library; above the grid's nz it means nz.  Checked as the library checks it, but for the window's size, which needs the grid:
    ValueError otherwise."""
    if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or not 0 <= int(layers) <= 0x7FFFFFFF:
        raise ValueError("mesh: slabs layers must be an integer >= 0")
    return abi.RmMeshSlabs(layers=int(layers), reserved=0)


def mesh_keep(**fields) -> abi.RmMeshKeep:
    """The abi.RmMeshKeep of Context.extract_mesh(..., keep=...) / mesh_from_values(..., keep=...), over abi.MESH_KEEP_DEFAULTS: min_triangles (a
    component passes with at least that many triangles, >= 0) and largest (0 keeps every passing component, k > 0 only the k with the most
    triangles, the lower component index first among equals).  Checked as the library checks it: ValueError otherwise, and for unknown keys."""
    unknown = set(fields) - set(abi.MESH_KEEP_DEFAULTS)
    if unknown:
        raise ValueError(f"mesh: unknown keep parameter {sorted(unknown)[0]}")
    p = {**abi.MESH_KEEP_DEFAULTS, **fields}
    for name in ("min_triangles", "largest"):
        v = p[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0x7FFFFFFF:
            raise ValueError(f"mesh: keep {name} must be an integer in 0..2^31 - 1")
    return abi.RmMeshKeep(min_triangles=int(p["min_triangles"]), largest=int(p["largest"]))


def mesh_simplify(grid, keep_duplicates=False) -> tuple:
    """The (abi.RmGrid, abi.RmMeshSimplify) of Context.extract_mesh(..., simplify=...) / mesh_from_values(..., simplify=...): `grid` is the
    Grid of clusters (one output vertex per occupied cell, it need not be related to the sampling grid), keep_duplicates keeps the triangles
    that repeat an earlier one.  Checked as the library checks them: ValueError otherwise."""
    if not isinstance(grid, Grid):
        raise ValueError("mesh: simplify grid must be a mesh.Grid")
    if not (isinstance(keep_duplicates, (bool, int, np.integer)) and int(keep_duplicates) in (0, 1)):
        raise ValueError("mesh: simplify keep_duplicates must be True or False")
    return grid.to_c(), abi.RmMeshSimplify(keep_duplicates=int(keep_duplicates))


def mesh_quadric(threshold=abi.MESH_QUADRIC_DEFAULTS["threshold"]) -> abi.RmMeshQuadric:
    """The abi.RmMeshQuadric of Context.extract_mesh(..., simplify=..., quadric=...) / mesh_from_values(..., simplify=..., quadric=...): the
    cluster vertices are placed at the minimisers of their clusters' plane quadrics (rm_mesh_simplify_quadric); eigenvalues at or below
    threshold * the largest are dropped from the solve, in [0, 1).  Checked as the library checks it: ValueError otherwise."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError("mesh: quadric threshold must be a number")
    with np.errstate(over="ignore"):
        t = np.float32(threshold)
    if not (math.isfinite(t) and 0 <= t < 1):
        raise ValueError("mesh: quadric threshold must be finite and in [0, 1)")
    return abi.RmMeshQuadric(threshold=float(threshold))


def mesh_occlusion(**fields) -> abi.RmMeshOcclusion:
    """The abi.RmMeshOcclusion of Context.extract_mesh(..., occlusion=...), over abi.MESH_OCCLUSION_DEFAULTS: radius (the first tap's distance,
    in [2^-64, 2^64]), directions (1, 2, 4, ... 64 over every vertex), taps (1, 2, 4 or 8 along each, halving the distance), normal_delta (the
    step of the normal that gives the frame, > 0), strength (ao = 1 - strength * occlusion, in [0, 4]) and flags (rm_sdf_grid's).  Checked as
    the library checks it: ValueError otherwise, and for unknown keys."""
    unknown = set(fields) - set(abi.MESH_OCCLUSION_DEFAULTS)
    if unknown:
        raise ValueError(f"mesh: unknown occlusion parameter {sorted(unknown)[0]}")
    p = {**abi.MESH_OCCLUSION_DEFAULTS, **fields}
    for name in ("radius", "normal_delta", "strength"):
        if isinstance(p[name], bool) or not isinstance(p[name], (int, float, np.integer, np.floating)):
            raise ValueError(f"mesh: occlusion {name} must be a number")
    with np.errstate(over="ignore"):
        radius, delta, strength = np.float32(p["radius"]), np.float32(p["normal_delta"]), np.float32(p["strength"])
    if not (math.isfinite(radius) and 2.0 ** -64 <= radius <= 2.0 ** 64):
        raise ValueError("mesh: occlusion radius must be finite and in [2^-64, 2^64]")
    for name, allowed in (("directions", (1, 2, 4, 8, 16, 32, 64)), ("taps", (1, 2, 4, 8))):
        v = p[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in allowed:
            raise ValueError(f"mesh: occlusion {name} must be one of {', '.join(str(a) for a in allowed)}")
    if not (math.isfinite(delta) and delta > 0):
        raise ValueError("mesh: occlusion normal_delta must be finite and > 0")
    if not (math.isfinite(strength) and 0 <= strength <= 4):
        raise ValueError("mesh: occlusion strength must be finite and in [0, 4]")
    flags = p["flags"]
    if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or int(flags) & ~(abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL):
        raise ValueError("mesh: occlusion flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both")
    return abi.RmMeshOcclusion(radius=float(p["radius"]), directions=int(p["directions"]), taps=int(p["taps"]), normal_delta=float(p["normal_delta"]),
                               strength=float(p["strength"]), flags=int(flags))


def mesh_project(**fields) -> abi.RmMeshProject:
    """The abi.RmMeshProject of Context.extract_mesh(..., project=...), over abi.MESH_PROJECT_DEFAULTS: iso (the level to project onto), rounds
    (1..16), relax (the fraction of the Newton step taken, in (0, 1]), tolerance (a vertex within it of the level does not move, >= 0), reach
    (per axis, how far a vertex may end from where it started, >= 0; 0 = no limit), normal_delta (the step of the normal that gives the
    direction, > 0) and flags (rm_sdf_grid's).  Checked as the library checks it: ValueError otherwise, and for unknown keys."""
    unknown = set(fields) - set(abi.MESH_PROJECT_DEFAULTS)
    if unknown:
        raise ValueError(f"mesh: unknown project parameter {sorted(unknown)[0]}")
    p = {**abi.MESH_PROJECT_DEFAULTS, **fields}
    for name in ("iso", "relax", "tolerance", "reach", "normal_delta"):
        if isinstance(p[name], bool) or not isinstance(p[name], (int, float, np.integer, np.floating)):
            raise ValueError(f"mesh: project {name} must be a number")
    with np.errstate(over="ignore"):
        iso, relax, tolerance, reach, delta = (np.float32(p[name]) for name in ("iso", "relax", "tolerance", "reach", "normal_delta"))
    if not math.isfinite(iso):
        raise ValueError("mesh: project iso must be finite")
    rounds = p["rounds"]
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 1 <= int(rounds) <= 16:
        raise ValueError("mesh: project rounds must be an integer in 1..16")
    if not (math.isfinite(relax) and 0 < relax <= 1):
        raise ValueError("mesh: project relax must be finite and in (0, 1]")
    if not (math.isfinite(tolerance) and tolerance >= 0):
        raise ValueError("mesh: project tolerance must be finite and >= 0")
    if not (math.isfinite(reach) and reach >= 0):
        raise ValueError("mesh: project reach must be finite and >= 0")
    if not (math.isfinite(delta) and delta > 0):
        raise ValueError("mesh: project normal_delta must be finite and > 0")
    flags = p["flags"]
    if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or int(flags) & ~(abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL):
        raise ValueError("mesh: project flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both")
    return abi.RmMeshProject(iso=float(p["iso"]), rounds=int(rounds), relax=float(p["relax"]), tolerance=float(p["tolerance"]), reach=float(p["reach"]),
                             normal_delta=float(p["normal_delta"]), flags=int(flags), reserved=0)


def mesh_deviation(**fields) -> abi.RmMeshDeviation:
    """The abi.RmMeshDeviation of Context.extract_mesh(..., deviation=...), over abi.MESH_DEVIATION_DEFAULTS: iso (the level the mesh stands
    for), order (n = 1, 2, 4 or 8: n * n samples per triangle), tolerance (a triangle whose largest |distance - iso| exceeds it is counted as
    over, >= 0) and flags (rm_sdf_grid's).  Checked as the library checks it: ValueError otherwise, and for unknown keys."""
    unknown = set(fields) - set(abi.MESH_DEVIATION_DEFAULTS)
    if unknown:
        raise ValueError(f"mesh: unknown deviation parameter {sorted(unknown)[0]}")
    p = {**abi.MESH_DEVIATION_DEFAULTS, **fields}
    for name in ("iso", "tolerance"):
        if isinstance(p[name], bool) or not isinstance(p[name], (int, float, np.integer, np.floating)):
            raise ValueError(f"mesh: deviation {name} must be a number")
    with np.errstate(over="ignore"):
        iso, tolerance = np.float32(p["iso"]), np.float32(p["tolerance"])
    if not math.isfinite(iso):
        raise ValueError("mesh: deviation iso must be finite")
    order = p["order"]
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or int(order) not in (1, 2, 4, 8):
        raise ValueError("mesh: deviation order must be 1, 2, 4 or 8")
    if not (math.isfinite(tolerance) and tolerance >= 0):
        raise ValueError("mesh: deviation tolerance must be finite and >= 0")
    flags = p["flags"]
    if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or int(flags) & ~(abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL):
        raise ValueError("mesh: deviation flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both")
    return abi.RmMeshDeviation(iso=float(p["iso"]), order=int(order), tolerance=float(p["tolerance"]), flags=int(flags))


def mesh_refine(**fields) -> abi.RmMeshRefine:
    """The abi.RmMeshRefine of Context.extract_mesh(..., refine=...), over abi.MESH_REFINE_DEFAULTS: iso (the level the mesh stands for),
    tolerance (an edge is split iff its midpoint's |distance - iso| exceeds it, >= 0), min_edge (... and its length exceeds it, >= 0), rounds
    (1..8), max_triangles (a round that would give more is not applied; 0 = the kernels' own limit) and flags (rm_sdf_grid's).  Checked as the
    library checks it: ValueError otherwise, and for unknown keys."""
    unknown = set(fields) - set(abi.MESH_REFINE_DEFAULTS)
    if unknown:
        raise ValueError(f"mesh: unknown refine parameter {sorted(unknown)[0]}")
    p = {**abi.MESH_REFINE_DEFAULTS, **fields}
    for name in ("iso", "tolerance", "min_edge"):
        if isinstance(p[name], bool) or not isinstance(p[name], (int, float, np.integer, np.floating)):
            raise ValueError(f"mesh: refine {name} must be a number")
    with np.errstate(over="ignore"):
        iso, tolerance, min_edge = (np.float32(p[name]) for name in ("iso", "tolerance", "min_edge"))
    if not math.isfinite(iso):
        raise ValueError("mesh: refine iso must be finite")
    if not (math.isfinite(tolerance) and tolerance >= 0):
        raise ValueError("mesh: refine tolerance must be finite and >= 0")
    if not (math.isfinite(min_edge) and min_edge >= 0):
        raise ValueError("mesh: refine min_edge must be finite and >= 0")
    rounds = p["rounds"]
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 1 <= int(rounds) <= 8:
        raise ValueError("mesh: refine rounds must be an integer in 1..8")
    most = p["max_triangles"]
    if isinstance(most, bool) or not isinstance(most, (int, np.integer)) or not 0 <= int(most) < 2 ** 64:
        raise ValueError("mesh: refine max_triangles must be an integer in 0..2^64 - 1")
    flags = p["flags"]
    if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or int(flags) & ~(abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL):
        raise ValueError("mesh: refine flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both")
    return abi.RmMeshRefine(iso=float(p["iso"]), tolerance=float(p["tolerance"]), min_edge=float(p["min_edge"]), rounds=int(rounds), max_triangles=int(most),
                            flags=int(flags), reserved=0)


def refine_tolerance(grid: Grid) -> float:
    """The tolerance extract_mesh(..., refine=...) takes when none is named: 1/64 of the smallest cell side of `grid`, min h[a] * 2^-6 with h in
    fp32 by RmGrid's rule -- the sagitta L^2 / (8 R) of a one-cell edge on a surface whose radius of curvature is 8 cells.  A default, not a
    test bar: what is fine enough is the caller's to say, and `deviation` measures what came of it."""
    f = np.float32
    return float(f(2.0 ** -6) * min((f(b) - f(a)) / f(k) for a, b, k in zip(grid.lo, grid.hi, grid.n)))


def project_reach(grid: Grid) -> float:
    """The reach extract_mesh(..., project=...) takes when none is given: half the smallest cell side of `grid`, 0.5f * min h[a] with h in
    fp32 by RmGrid's rule."""
    f = np.float32
    return float(f(0.5) * min((f(b) - f(a)) / f(k) for a, b, k in zip(grid.lo, grid.hi, grid.n)))


@dataclass
class Mesh:
    """A triangle mesh as numpy arrays: positions [V, 3] float32, triangles [T, 3] uint32 (counter-clockwise seen from outside), cells
    [V] uint32 (each vertex's linear cell index in `grid`), and normals / colours [V, 3] float32 or None.  labels [V] uint32 (each vertex's
    connected component) and component_sizes [C, 2] uint32 ((vertices, triangles) per component) only when the call asked for components.
    occlusion [V] float32 (1 = open; rm_mesh_occlusion) only when the call asked for it.  measures (rm_mesh_measure; only when the call asked
    for them): a dict of abi.RmMeshMeasures' fields plus component_edges, [C, 4] uint64 (edges, boundary, irregular, unbalanced)."""
    positions: np.ndarray
    triangles: np.ndarray
    cells: Optional[np.ndarray] = None
    normals: Optional[np.ndarray] = None
    colours: Optional[np.ndarray] = None
    grid: Optional[Grid] = None
    timings: Optional[dict] = None  # rm_mesh_timings: milliseconds of sampling, meshing, attributes (device events)
    labels: Optional[np.ndarray] = None
    component_sizes: Optional[np.ndarray] = None
    occlusion = None  # Optional[np.ndarray]; an attribute that the constructor takes by keyword (below): the dataclass's own fields stay as they were
    measures = None  # Optional[dict]; taken the same way
    projection = None  # Optional[dict]: abi.RmMeshProjection's fields (rm_mesh_project), only when the call asked for a projection; taken the same way
    residual = None  # Optional[np.ndarray]: [V] float32, the distance minus iso at the projected vertices; with `projection`
    deviation = None  # Optional[dict]: abi.RmMeshDeviationReport's fields (rm_mesh_deviation), only when the call asked for a deviation; taken the same way
    triangle_deviation = None  # Optional[np.ndarray]: [T] float32, each triangle's largest |distance - iso| over its samples; with `deviation`
    refinement = None  # Optional[dict]: abi.RmMeshRefinement's fields (rm_mesh_refine), only when the call asked for a refinement; taken the same way

    @property
    def vertices(self) -> int:
        return len(self.positions)


def _with_occlusion(init):
    def __init__(self, *args, occlusion=None, measures=None, projection=None, residual=None, deviation=None, triangle_deviation=None, refinement=None, **fields):
        init(self, *args, **fields)
        self.occlusion = occlusion
        self.measures = measures
        self.projection = projection
        self.residual = residual
        self.deviation = deviation
        self.triangle_deviation = triangle_deviation
        self.refinement = refinement

    __init__.__doc__, __init__.__wrapped__ = init.__doc__, init
    return __init__


Mesh.__init__ = _with_occlusion(Mesh.__init__)


def shaded(mesh: Mesh) -> Mesh:
    """A copy of the mesh whose colours are multiplied by its occlusion (fp32); a mesh without colours gets grey: the occlusion in all
    three channels.  ValueError for a mesh without an occlusion."""
    if mesh.occlusion is None:
        raise ValueError("mesh: shaded needs a mesh with an occlusion (extract_mesh(..., occlusion=...))")
    ao = np.asarray(mesh.occlusion, np.float32)[:, None]
    base = np.ones((mesh.vertices, 3), np.float32) if mesh.colours is None else np.asarray(mesh.colours, np.float32)
    return replace(mesh, colours=base * ao, occlusion=mesh.occlusion)


def _number(v) -> str:
    return "%.9g" % float(v)  # nine digits give every float32 back


def write_obj(mesh: Mesh, path) -> None:
    """Wavefront OBJ: `v` lines, `vn` lines when the mesh has normals, faces 1-based (`f a//a b//b c//c` with normals)."""
    lines = ["# hip_raymarch mesh: %d vertices, %d triangles" % (mesh.vertices, len(mesh.triangles))]
    lines += ["v " + " ".join(_number(c) for c in p) for p in mesh.positions]
    if mesh.normals is not None:
        lines += ["vn " + " ".join(_number(c) for c in n) for n in mesh.normals]
    face = "f {0}//{0} {1}//{1} {2}//{2}" if mesh.normals is not None else "f {0} {1} {2}"
    lines += [face.format(*(int(i) + 1 for i in t)) for t in mesh.triangles]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def colour_bytes(colours: np.ndarray) -> np.ndarray:
    """Colours as the PLY stores them: floor(clamp(c, 0, 1) * 255 + 0.5) in double, NaN as 0."""
    c = np.nan_to_num(np.asarray(colours, np.float64), nan=0.0, posinf=1.0, neginf=0.0)
    return np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def encode_ply(mesh: Mesh) -> bytes:
    """Binary little-endian PLY: x y z, then nx ny nz when the mesh has normals, then uchar red green blue when it has colours, then
    float quality when it has an occlusion; faces as a uchar count and uint indices."""
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", "comment hip_raymarch mesh", "element vertex %d" % mesh.vertices,
              "property float x", "property float y", "property float z"]
    if mesh.normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if mesh.colours is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    if mesh.occlusion is not None:
        fields += [("quality", "<f4")]
        header += ["property float quality"]
    header += ["element face %d" % len(mesh.triangles), "property list uchar uint vertex_indices", "end_header"]
    v = np.zeros(mesh.vertices, np.dtype(fields))
    for k, name in enumerate("xyz"):
        v[name] = mesh.positions[:, k]
        if mesh.normals is not None:
            v["n" + name] = mesh.normals[:, k]
    if mesh.colours is not None:
        rgb = colour_bytes(mesh.colours)
        for k, name in enumerate(("red", "green", "blue")):
            v[name] = rgb[:, k]
    if mesh.occlusion is not None:
        v["quality"] = mesh.occlusion
    f = np.zeros(len(mesh.triangles), np.dtype([("count", "u1"), ("a", "<u4"), ("b", "<u4"), ("c", "<u4")]))
    f["count"] = 3
    for k, name in enumerate("abc"):
        f[name] = mesh.triangles[:, k]
    return ("\n".join(header) + "\n").encode("ascii") + v.tobytes() + f.tobytes()


def write_ply(mesh: Mesh, path) -> None:
    with open(path, "wb") as f:
        f.write(encode_ply(mesh))


def encode_stl(mesh: Mesh) -> bytes:
    """Binary STL: 80 header bytes (`hip_raymarch mesh`, zero padded), uint32 T, then per triangle the facet normal, p0, p1, p2 as
    little-endian float32 and a uint16 0.  The normal is computed in double from the float32 coordinates, every operation rounded on its
    own: e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2, len = sqrt((cx cx + cy cy) + cz cz), c / len rounded to float32 -- and (0, 0, 0) where
    len is not > 0 or not finite.  js/index.js encodeStl gives the same bytes."""
    p = np.asarray(mesh.positions, np.float32).reshape(-1, 3)
    t = np.asarray(mesh.triangles, np.uint32).reshape(-1, 3)
    if len(t) >= 2 ** 32:
        raise ValueError("mesh: an STL file holds fewer than 2^32 triangles")
    corners = p[t.astype(np.int64)]  # [T, 3, 3]
    d = corners.astype(np.float64)
    e1, e2 = d[:, 1] - d[:, 0], d[:, 2] - d[:, 0]
    with np.errstate(all="ignore"):
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        length = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        good = (length > 0) & np.isfinite(length)
        normal = np.where(good[:, None], c / np.where(good, length, 1.0)[:, None], 0.0).astype(np.float32)
    facets = np.zeros(len(t), np.dtype([("normal", "<f4", 3), ("corners", "<f4", (3, 3)), ("attribute", "<u2")]))
    facets["normal"] = normal
    facets["corners"] = corners
    header = b"hip_raymarch mesh".ljust(80, b"\0")
    return header + np.uint32(len(t)).astype("<u4").tobytes() + facets.tobytes()


def write_stl(mesh: Mesh, path) -> None:
    with open(path, "wb") as f:
        f.write(encode_stl(mesh))
