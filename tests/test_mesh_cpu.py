"""Mesh extraction without a GPU: the numpy restatement's own invariants (tests/mesh_ref.py), rm_grid_axis against it, every refusal
that is made before the handles are looked at, the ABI, the file writers and the two hosts' parameter packing."""
import ctypes as C
import json
import re
import shutil
import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mesh_ref as MR
from raymarching_engine_amd import abi, mesh as M, native

ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
ENTRY_POINTS = ("rm_grid_axis", "rm_sdf_grid", "rm_sdf_grid_device", "rm_mesh_params_default", "rm_mesh_extract", "rm_mesh_from_values", "rm_mesh_counts", "rm_mesh_timings",
                "rm_mesh_download", "rm_mesh_device_ptr", "rm_mesh_destroy")

LO, HI, N = (-1.3, -1.2, -1.4), (1.25, 1.3, 1.35), (14, 13, 15)


def analytic_fields():
    p = MR.corner_positions(LO, HI, N).astype(np.float64)
    sphere = np.linalg.norm(p, axis=1) - 0.9
    torus = np.hypot(np.hypot(p[:, 0], p[:, 2]) - 0.8, p[:, 1]) - 0.3  # about y
    return {"sphere": sphere.astype(F), "torus": torus.astype(F)}


def special_field(n, seed, frac=0.04):
    """A random field with an all-outside border that carries +-inf, NaN, +0 and -0."""
    rng = np.random.default_rng(seed)
    shape = (n[2] + 1, n[1] + 1, n[0] + 1)
    v = rng.standard_normal(shape).astype(F)
    pick = rng.random(shape)
    for k, s in enumerate((np.inf, -np.inf, np.nan, 0.0, -0.0)):
        v[(pick >= k * frac) & (pick < (k + 1) * frac)] = F(s)
    for a in range(3):
        for side in (0, -1):
            idx = [slice(None)] * 3
            idx[a] = side
            v[tuple(idx)] = np.abs(rng.standard_normal(v[tuple(idx)].shape).astype(F)) + F(0.1)
    return v


# ---- 1, 2: the restatement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, chi", [("sphere", 2), ("torus", 0)])
def test_restatement_gives_a_closed_oriented_surface(name, chi):
    """A throwaway per-cell version of the header's text gave 444 / 884 (sphere) and 384 / 768 (torus) vertices / triangles on this grid."""
    pos, tri, cells = MR.surface_nets(LO, HI, N, analytic_fields()[name])
    print(f"{name}: {len(pos)} vertices, {len(tri)} triangles")
    (_, ucount), _, _ = MR.edge_counts(tri)
    assert len(tri) > 0 and (ucount == 2).all()
    assert MR.directed_balanced(tri)
    assert MR.euler(pos, tri) == chi
    assert MR.signed_volume(pos, tri) > 0
    assert MR.inside_cell_boxes(LO, HI, N, pos, cells)
    assert pos.dtype == F and tri.dtype == np.uint32 and cells.dtype == np.uint32 and (np.diff(cells.astype(np.int64)) > 0).all()


def test_restatement_on_a_field_of_special_values():
    n = (9, 8, 10)
    v = special_field(n, 7)
    assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and (v == 0).any() and np.signbit(v[v == 0]).any()
    pos, tri, cells = MR.surface_nets((-1, -1, -1), (1, 1.5, 2), n, v)
    (_, ucount), _, _ = MR.edge_counts(tri)
    assert len(tri) > 0 and (ucount % 2 == 0).all()  # (edges shared by 4 triangles occur: manifoldness is not claimed)
    assert MR.directed_balanced(tri)
    assert np.isfinite(pos).all() and MR.inside_cell_boxes((-1, -1, -1), (1, 1.5, 2), n, pos, cells)


# ---- 3: the grid ---------------------------------------------------------------------------------------------------------------

GRIDS = [(LO, HI, N), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 7, 1)),  # h = 1/3, 1/7: inexact
         ((-2.5, 0.1, -1e-3), (2.5, 0.7, 1e3), (1024, 1000, 3)), ((1e-30, -7.0, 5.0), (3e-30, -6.9999, 5.000001), (5, 2, 1))]


@pytest.mark.parametrize("lo, hi, n", GRIDS)
def test_grid_axis_is_the_restatement_bit_for_bit(lo, hi, n):
    g = M.Grid(lo, hi, n)
    for a in range(3):
        got, ref = g.axis(a), MR.axis(lo[a], hi[a], n[a])
        assert got.shape == (n[a] + 1,) and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (a, got, ref)
    assert g.shape == (n[2] + 1, n[1] + 1, n[0] + 1) and g.corners == (n[0] + 1) * (n[1] + 1) * (n[2] + 1) and g.cells == n[0] * n[1] * n[2]


def c_grid(lo=(0, 0, 0), hi=(1, 1, 1), n=(2, 2, 2), reserved=0):
    return abi.RmGrid(lo=(C.c_float * 3)(*lo), hi=(C.c_float * 3)(*hi), n=(C.c_int32 * 3)(*n), reserved=reserved)


BAD_GRIDS = [dict(n=(0, 2, 2)), dict(n=(2, 1025, 2)), dict(n=(2, 2, -1)), dict(lo=(float("nan"), 0, 0)), dict(hi=(1, float("inf"), 1)), dict(lo=(0, 0, -float("inf"))),
             dict(lo=(1, 0, 0)), dict(lo=(2, 0, 0)), dict(lo=(-3e38, 0, 0), hi=(3e38, 1, 1)), dict(n=(1024, 1024, 255)), dict(reserved=1)]


def test_grid_axis_refusals():
    lib = native.load_library()
    out = (C.c_float * 2048)()
    assert lib.rm_grid_axis(C.byref(c_grid()), 0, out) == abi.RM_OK
    assert lib.rm_grid_axis(C.byref(c_grid(n=(1023, 511, 511))), 0, out) == abi.RM_OK  # 2^28 corners exactly
    assert lib.rm_grid_axis(None, 0, out) == abi.RM_ERR_INVALID
    for axis in (-1, 3):
        assert lib.rm_grid_axis(C.byref(c_grid()), axis, out) == abi.RM_ERR_INVALID
    assert lib.rm_grid_axis(C.byref(c_grid()), 0, None) == abi.RM_ERR_INVALID
    for bad in BAD_GRIDS:
        assert lib.rm_grid_axis(C.byref(c_grid(**bad)), 0, out) == abi.RM_ERR_INVALID, bad
        assert lib.rm_last_error(None).decode().startswith("rm_grid_axis: grid"), bad
        if "reserved" not in bad:
            with pytest.raises(ValueError):
                M.Grid(bad.get("lo", (0, 0, 0)), bad.get("hi", (1, 1, 1)), bad.get("n", (2, 2, 2)))


# ---- 4: the refusals made before the handles are looked at -----------------------------------------------------------------------

def c_params(**fields):
    p = abi.RmMeshParams()
    native.load_library().rm_mesh_params_default(C.byref(p))
    for k, v in fields.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [(dict(iso=float("nan")), "iso"), (dict(iso=float("inf")), "iso"), (dict(normals=2), "normals"), (dict(normals=-1), "normals"), (dict(colours=2), "colours"),
              (dict(colours=-1), "colours"), (dict(normal_delta=0.0), "normal_delta"), (dict(normal_delta=-1e-5), "normal_delta"),
              (dict(normal_delta=float("nan")), "normal_delta"), (dict(normal_delta=float("inf")), "normal_delta"), (dict(flags=2), "flags"),
              (dict(flags=64), "flags"), (dict(flags=1 | 4), "flags"), (dict(flags=-1), "flags"), (dict(reserved=1), "reserved")]


def test_every_parameter_refusal_speaks_before_the_handles():
    """No context exists without a GPU: every call ends in RM_ERR_INVALID, and the text (rm_last_error(NULL)) tells which check spoke."""
    lib = native.load_library()
    out = C.c_void_p()
    last = lambda: lib.rm_last_error(None).decode()
    good, ok = c_grid(), c_params()
    # everything valid: the NULL handles are what is refused
    assert lib.rm_mesh_extract(None, None, C.byref(good), C.byref(ok), C.byref(out)) == abi.RM_ERR_INVALID and last() == "rm_mesh_extract: NULL argument"
    assert lib.rm_mesh_extract(None, None, C.byref(good), None, C.byref(out)) == abi.RM_ERR_INVALID and last() == "rm_mesh_extract: NULL argument"
    assert lib.rm_mesh_from_values(None, C.byref(good), None, 0.0, C.byref(out)) == abi.RM_ERR_INVALID and last() == "rm_mesh_from_values: NULL argument"
    assert lib.rm_sdf_grid(None, None, C.byref(good), 0, None) == abi.RM_ERR_INVALID and last() == "rm_sdf_grid: NULL argument"
    assert lib.rm_sdf_grid_device(None, None, C.byref(good), 0, None, None) == abi.RM_ERR_INVALID and last() == "rm_sdf_grid_device: NULL argument"
    for bad in BAD_GRIDS + [None]:
        g = C.byref(c_grid(**bad)) if bad is not None else None
        for who, call in (("rm_mesh_extract", lambda: lib.rm_mesh_extract(None, None, g, C.byref(ok), C.byref(out))),
                          ("rm_mesh_from_values", lambda: lib.rm_mesh_from_values(None, g, None, 0.0, C.byref(out))),
                          ("rm_sdf_grid", lambda: lib.rm_sdf_grid(None, None, g, 0, None)),
                          ("rm_sdf_grid_device", lambda: lib.rm_sdf_grid_device(None, None, g, 0, None, None))):
            assert call() == abi.RM_ERR_INVALID and re.match(rf"{who}: (grid|NULL grid)", last()), (who, bad, last())
    for fields, word in BAD_PARAMS:
        assert lib.rm_mesh_extract(None, None, C.byref(good), C.byref(c_params(**fields)), C.byref(out)) == abi.RM_ERR_INVALID
        assert last().startswith("rm_mesh_extract: " + word), (fields, last())
    # normal_delta is looked at only when normals are on; the allowed flags pass
    for fields in (dict(normals=0, normal_delta=-1.0), dict(flags=abi.RM_RENDER_FAST), dict(flags=abi.RM_RENDER_NO_CULL), dict(flags=abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL),
                   dict(colours=1), dict(iso=-0.25)):
        assert lib.rm_mesh_extract(None, None, C.byref(good), C.byref(c_params(**fields)), C.byref(out)) == abi.RM_ERR_INVALID and last() == "rm_mesh_extract: NULL argument", fields
    for iso in (float("nan"), float("inf"), -float("inf")):
        assert lib.rm_mesh_from_values(None, C.byref(good), None, iso, C.byref(out)) == abi.RM_ERR_INVALID and last() == "rm_mesh_from_values: iso must be finite"
    for flags in (2, 4, 64, 1 | 16, -1):
        assert lib.rm_sdf_grid(None, None, C.byref(good), flags, None) == abi.RM_ERR_INVALID and last().startswith("rm_sdf_grid: flags")
        assert lib.rm_sdf_grid_device(None, None, C.byref(good), flags, None, None) == abi.RM_ERR_INVALID and last().startswith("rm_sdf_grid_device: flags")
    # the handle-free ends of the mesh entries
    counts = (C.c_ulonglong * 2)()
    assert lib.rm_mesh_counts(None, counts) == abi.RM_ERR_INVALID and lib.rm_mesh_download(None, 0, None, 0) == abi.RM_ERR_INVALID
    assert lib.rm_mesh_device_ptr(None, 0) is None and lib.rm_mesh_timings(None, (C.c_float * 3)()) == abi.RM_ERR_INVALID
    lib.rm_mesh_destroy(None)


@pytest.mark.parametrize("bad", [dict(iso=float("nan")), dict(iso="0"), dict(normals=2), dict(colours="yes"), dict(normal_delta=0.0), dict(normal_delta=float("inf")),
                                 dict(flags=2), dict(flags=1.0), dict(flags=64)])
def test_python_refuses_bad_mesh_parameters(bad):
    with pytest.raises(ValueError):
        M.mesh_params(**bad)


# ---- 5, 6: the ABI -------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_declared():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void|void\*) {name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    listed = ("RmGrid", "RmMeshParams", "rm_mesh", "RM_MESH_POSITIONS") + ENTRY_POINTS
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in listed)
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    assert re.search(r"RM_MESH_POSITIONS = 0, RM_MESH_NORMALS = 1, RM_MESH_COLOURS = 2, RM_MESH_TRIANGLES = 3, RM_MESH_CELLS = 4", header)
    assert (abi.RM_MESH_POSITIONS, abi.RM_MESH_NORMALS, abi.RM_MESH_COLOURS, abi.RM_MESH_TRIANGLES, abi.RM_MESH_CELLS) == (0, 1, 2, 3, 4)
    declared = set(re.findall(r"^RM_API (?:int|void|void\*|const char\*)\s+(rm_[a-z_0-9]+)\(", header, re.M))
    assert declared == set(native.EXPORTS)
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-2] in "TDBVWR"}
    assert exported == declared, sorted(exported ^ declared)


def test_defaults_and_struct_sizes():
    lib = native.load_library()
    p = abi.RmMeshParams(iso=3.0, normals=0, normal_delta=1.0, colours=1, flags=1, reserved=9)
    lib.rm_mesh_params_default(C.byref(p))
    lib.rm_mesh_params_default(None)
    assert (p.iso, p.normals, p.normal_delta, p.colours, p.flags, p.reserved) == (0.0, 1, float(F(1e-5)), 0, 0, 0)
    assert bytes(p) == bytes(M.mesh_params()) and abi.MESH_DEFAULTS == dict(iso=0.0, normals=1, normal_delta=1e-5, colours=0, flags=0)
    assert (C.sizeof(abi.RmGrid), C.sizeof(abi.RmMeshParams)) == (40, 24)
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct sizes from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\n'
                       'int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(RmGrid), sizeof(RmMeshParams), offsetof(RmGrid, hi), offsetof(RmGrid, n), '
                       'offsetof(RmGrid, reserved), offsetof(RmMeshParams, normal_delta), offsetof(RmMeshParams, flags), offsetof(RmMeshParams, reserved)); return 0; }\n')
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [40, 24, abi.RmGrid.hi.offset, abi.RmGrid.n.offset, abi.RmGrid.reserved.offset, abi.RmMeshParams.normal_delta.offset,
                                     abi.RmMeshParams.flags.offset, abi.RmMeshParams.reserved.offset]


# ---- 7: the writers ------------------------------------------------------------------------------------------------------------

def read_obj(path):
    v, vn, f = [], [], []
    for line in Path(path).read_text().splitlines():
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            f.append([[int(i) if i else 0 for i in x.split("/")] for x in w[1:]])
    return np.array(v, F).reshape(-1, 3), np.array(vn, F).reshape(-1, 3), f


def read_ply(data: bytes):
    """A reader of what a PLY header declares (binary little-endian; float / uchar scalars, one uchar-counted uint list)."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = []
    for line in lines[2:]:
        w = line.split()
        if w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            elements[-1][2].append(w[1:])
    at, out = end, {}
    for name, count, props in elements:
        if name == "vertex":
            dt = np.dtype([(p[1], {"float": "<f4", "uchar": "u1"}[p[0]]) for p in props])
            out["vertex"] = np.frombuffer(data, dt, count, at)
            at += count * dt.itemsize
        else:
            assert props == [["list", "uchar", "uint", "vertex_indices"]]
            faces = []
            for _ in range(count):
                k = data[at]
                faces.append(struct.unpack_from("<%dI" % k, data, at + 1))
                at += 1 + 4 * k
            out["face"] = np.array(faces, np.uint32).reshape(-1, 3)
    assert at == len(data)
    return out


def small_mesh(normals, colours):
    pos, tri, cells = MR.surface_nets(LO, HI, N, analytic_fields()["sphere"])
    rng = np.random.default_rng(3)
    nrm = (pos / np.linalg.norm(pos, axis=1, keepdims=True)).astype(F) if normals else None
    col = rng.uniform(-0.2, 1.2, pos.shape).astype(F) if colours else None
    if colours:
        col[0] = (np.nan, np.inf, -np.inf)
    return M.Mesh(positions=pos, triangles=tri, cells=cells, normals=nrm, colours=col)


@pytest.mark.parametrize("normals, colours", [(False, False), (True, False), (True, True), (False, True)])
def test_obj_and_ply_read_back(tmp_path, normals, colours):
    m = small_mesh(normals, colours)
    M.write_obj(m, tmp_path / "m.obj")
    v, vn, f = read_obj(tmp_path / "m.obj")
    assert np.array_equal(v.view(np.uint32), m.positions.view(np.uint32))
    assert (np.array_equal(vn.view(np.uint32), m.normals.view(np.uint32))) if normals else len(vn) == 0
    assert len(f) == len(m.triangles)
    assert np.array_equal(np.array([[c[0] for c in face] for face in f]) - 1, m.triangles)  # 1-based
    assert all((len(c) == 3 and c[2] == c[0] and c[1] == 0) if normals else len(c) == 1 for face in f for c in face)
    M.write_ply(m, tmp_path / "m.ply")
    data = (tmp_path / "m.ply").read_bytes()
    assert data == M.encode_ply(m)
    ply = read_ply(data)
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + (["red", "green", "blue"] if colours else [])
    assert list(ply["vertex"].dtype.names) == names
    assert np.array_equal(np.stack([ply["vertex"][k] for k in "xyz"], -1).view(np.uint32), m.positions.view(np.uint32))
    if normals:
        assert np.array_equal(np.stack([ply["vertex"][k] for k in ("nx", "ny", "nz")], -1).view(np.uint32), m.normals.view(np.uint32))
    if colours:
        rgb = np.stack([ply["vertex"][k] for k in ("red", "green", "blue")], -1)
        assert rgb.dtype == np.uint8 and np.array_equal(rgb, M.colour_bytes(m.colours)) and tuple(rgb[0]) == (0, 255, 0)
        assert np.array_equal(M.colour_bytes(np.array([0.0, 1.0, 0.5, 0.25, -1.0, 2.0], F)), [0, 255, 128, 64, 0, 255])
    assert np.array_equal(ply["face"], m.triangles)
    empty = M.Mesh(positions=np.zeros((0, 3), F), triangles=np.zeros((0, 3), np.uint32))
    assert read_ply(M.encode_ply(empty))["vertex"].shape == (0,)


# ---- 8: the two hosts pack the same bytes ------------------------------------------------------------------------------------------

def test_node_packs_the_parameter_blocks_as_python_does():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    cases = [dict(grid=dict(lo=LO, hi=HI, n=N), params={}),
             dict(grid=dict(lo=(0, 0.1, -7), hi=(1, 0.3, 9.5), n=(1, 1024, 33)), params=dict(iso=0.0125, normals=False, colours=True, flags=abi.RM_RENDER_FAST)),
             dict(grid=dict(lo=(-1, -1, -1), hi=(1, 1, 1), n=(64, 64, 64)), params=dict(iso=-0.5, normalDelta=1e-3, flags=abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL))]
    script = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const out = { sizes: [r.addon.sizes().RmGrid, r.addon.sizes().RmMeshParams], defaults: r.meshParams(), cases: [], bad: [],
              fns: [typeof r.addon.sdfGrid, typeof r.addon.extractMesh, typeof r.addon.meshFromValues, typeof r.encodePly, typeof r.RenderJobContext.prototype.sdfGrid,
                    typeof r.RenderJobContext.prototype.extractMesh, typeof r.RenderJobContext.prototype.meshFromValues] };
for (const c of %s) {
  const b = r.addon.meshBlocks(r.meshGrid(c.grid.lo, c.grid.hi, c.grid.n), r.meshParams(c.params));
  out.cases.push([hex(b.grid), hex(b.params)]);
}
for (const f of [() => r.meshGrid([0, 0, 0], [1, 1, 1], [0, 1, 1]), () => r.meshGrid([0, 0, 0], [1, 1, 1], [1, 1025, 1]), () => r.meshGrid([0, 0, 0], [0, 1, 1], [1, 1, 1]),
                 () => r.meshGrid([0, 0, 0], [1, NaN, 1], [1, 1, 1]), () => r.meshGrid([0, 0, 0], [1, 1, 1], [1.5, 1, 1]), () => r.meshGrid([0, 0], [1, 1], [1, 1]),
                 () => r.meshGrid([0, 0, 0], [1, 1, 1], [1024, 1024, 255]),
                 () => r.meshParams({ iso: NaN }), () => r.meshParams({ normals: 2 }), () => r.meshParams({ colours: "yes" }), () => r.meshParams({ normalDelta: 0 }),
                 () => r.meshParams({ flags: 2 }), () => r.meshParams({ flags: 1.5 }), () => r.meshParams({ level: 1 })])
  try { f(); out.bad.push(false); } catch (e) { out.bad.push(true); }
console.log(JSON.stringify(out));
""" % (str(JS / "index.js"), json.dumps(cases))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["sizes"] == [40, 24] and all(out["bad"]) and out["fns"] == ["function"] * 7
    assert out["defaults"] == dict(iso=0.0, normals=1, normalDelta=1e-5, colours=0, flags=0)
    for c, (g, p) in zip(cases, out["cases"]):
        kw = {("normal_delta" if k == "normalDelta" else k): v for k, v in c["params"].items()}
        assert g == bytes(M.Grid(**c["grid"]).to_c()).hex() and p == bytes(M.mesh_params(**kw)).hex(), c


def test_node_encodes_the_ply_python_writes():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    for normals, colours in ((False, False), (True, True)):
        m = small_mesh(normals, colours)
        with tempfile.TemporaryDirectory() as tmp:
            for name in ("positions", "triangles", "normals", "colours"):
                a = getattr(m, name)
                if a is not None:
                    a.tofile(str(Path(tmp) / name))
            script = """
const r = require(%r), fs = require("fs"), d = %r;
const f32 = (n) => fs.existsSync(d + "/" + n) ? new Float32Array(new Uint8Array(fs.readFileSync(d + "/" + n)).buffer) : null;
const mesh = { positions: f32("positions"), normals: f32("normals"), colours: f32("colours"),
               triangles: new Uint32Array(new Uint8Array(fs.readFileSync(d + "/triangles")).buffer) };
fs.writeFileSync(d + "/out.ply", r.encodePly(mesh));
""" % (str(JS / "index.js"), tmp)
            subprocess.run(["node", "-e", script], check=True, timeout=60)
            assert (Path(tmp) / "out.ply").read_bytes() == M.encode_ply(m)
