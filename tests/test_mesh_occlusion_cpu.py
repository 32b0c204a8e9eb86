"""Ambient occlusion without a GPU: the ABI of rm_mesh_occlusion_default / _directions / rm_mesh_occlusion, the direction table, every refusal
that is made before the handles are looked at, the two hosts' packing of RmMeshOcclusion, the numpy restatement (tests/mesh_occlusion_ref.py) on
analytic fp32 distance fields, and the PLY writers' `quality` property."""
import ctypes as C
import json
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mesh_occlusion_ref as OR
from raymarching_engine_amd import abi, mesh as M, native

ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
ENTRY_POINTS = ("rm_mesh_occlusion_default", "rm_mesh_occlusion_directions", "rm_mesh_occlusion")
F = np.float32
DEFAULT_BYTES = np.array([0.25], "<f4").tobytes() + np.array([16, 4], "<i4").tobytes() + np.array([2.0 ** -10, 1.0], "<f4").tobytes() + bytes(12)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) {name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshOcclusion",) + ENTRY_POINTS)
    assert m.group(1).rstrip().endswith("(additions only)")
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(ENTRY_POINTS) <= exported


def test_defaults_and_struct_layout():
    lib = native.load_library()
    o = abi.RmMeshOcclusion(radius=3.0, directions=7, taps=3, normal_delta=1.0, strength=9.0, flags=5, reserved=(C.c_int32 * 2)(5, 6))
    lib.rm_mesh_occlusion_default(C.byref(o))
    lib.rm_mesh_occlusion_default(None)  # a no-op
    assert (o.radius, o.directions, o.taps, o.normal_delta, o.strength, o.flags, list(o.reserved)) == (0.25, 16, 4, 2.0 ** -10, 1.0, 0, [0, 0])
    assert bytes(o) == bytes(M.mesh_occlusion()) == DEFAULT_BYTES
    assert abi.MESH_OCCLUSION_DEFAULTS == dict(radius=0.25, directions=16, taps=4, normal_delta=2.0 ** -10, strength=1.0, flags=0)
    assert C.sizeof(abi.RmMeshOcclusion) == 32
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct layout from the header"
    names = ("radius", "directions", "taps", "normal_delta", "strength", "flags", "reserved")
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\nint main(void){ printf("%zu", sizeof(RmMeshOcclusion));\n'
                       + "".join(f'printf(" %zu", offsetof(RmMeshOcclusion, {n}));\n' for n in names) + "return 0; }\n")
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 4, 8, 12, 16, 20, 24]
    assert [getattr(abi.RmMeshOcclusion, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24]


# ---- the direction table -----------------------------------------------------------------------------------------------------------------------

def c_table(K):
    out = np.full((K, 4), np.nan, F)
    assert native.load_library().rm_mesh_occlusion_directions(K, native._fp(out)) == abi.RM_OK
    return out


def ulps(a, b):
    """The distance of two float32 arrays of one sign pattern, in units in the last place."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("K", OR.DIRECTIONS)
def test_the_direction_table(K):
    t = c_table(K)
    assert np.isfinite(t).all() and (t[:, 2] > 0).all()
    length = np.sqrt((t[:, :3].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 2.0 ** -22
    k = np.arange(K, dtype=np.float64)
    u, phi = (k + 0.5) / K, k * (np.pi * (3.0 - np.sqrt(5.0)))
    want = np.stack([np.sqrt(u) * np.cos(phi), np.sqrt(u) * np.sin(phi), np.sqrt(1.0 - u)], axis=1).astype(F)
    assert ulps(t[:, :3], want).max() <= 1
    assert np.array_equal(t[:, 3].view(np.uint32), (1.0 / t[:, 2].astype(np.float64)).astype(F).view(np.uint32))
    assert ulps(OR.directions(K)[:, :3], t[:, :3]).max() <= 1  # the restatement's own table: the same formula through numpy's cos and sin
    assert np.array_equal(OR.directions(K)[:, 2:].view(np.uint32), t[:, 2:].view(np.uint32))  # z and 1 / z have no libm in them


def test_the_direction_table_is_refused_for_other_counts_and_without_room():
    lib = native.load_library()
    last = lambda: lib.rm_last_error(None).decode()
    room = np.zeros((64, 4), F)
    for bad in (0, -1, 3, 5, 12, 65, 128, 1 << 30, -(1 << 31)):
        assert lib.rm_mesh_occlusion_directions(bad, native._fp(room)) == abi.RM_ERR_INVALID
        assert last() == "rm_mesh_occlusion_directions: directions must be 1, 2, 4, 8, 16, 32 or 64" and not room.any()
    assert lib.rm_mesh_occlusion_directions(16, None) == abi.RM_ERR_INVALID and last() == "rm_mesh_occlusion_directions: NULL argument"


# ---- the refusals made before the handles are looked at --------------------------------------------------------------------------------------

def c_block(**fields):
    reserved = fields.pop("reserved", (0, 0))
    return abi.RmMeshOcclusion(**{**abi.MESH_OCCLUSION_DEFAULTS, **fields}, reserved=(C.c_int32 * 2)(*reserved))


NAN, INF = float("nan"), float("inf")
# in the header's order: a block that fails several checks is refused with the first one's text
BAD_FIELDS = [
    ("radius", (0.0, -0.25, 2.0 ** -65, 2.0 ** 65, NAN, INF, -INF), "occlusion radius must be finite and in [2^-64, 2^64]"),
    ("directions", (0, -1, 3, 5, 12, 65, 128, 1 << 30), "occlusion directions must be 1, 2, 4, 8, 16, 32 or 64"),
    ("taps", (0, -1, 3, 5, 16, 1 << 30), "occlusion taps must be 1, 2, 4 or 8"),
    ("normal_delta", (0.0, -1e-3, NAN, INF), "occlusion normal_delta must be finite and > 0"),
    ("strength", (-0.125, 4.5, NAN, INF, -INF), "occlusion strength must be finite and in [0, 4]"),
    ("flags", (4, 8, -1, abi.RM_RENDER_FAST | 64, 1 << 20), "flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both"),
    ("reserved", ((1, 0), (0, -1), (3, 4)), "occlusion reserved must be 0"),
]


def test_every_invalid_field_is_refused_in_c_before_the_handles_and_in_order():
    """No mesh exists without a GPU: every call ends in RM_ERR_INVALID, and the text (rm_last_error(NULL)) tells which check spoke."""
    lib = native.load_library()
    last = lambda: lib.rm_last_error(None).decode()
    call, who, inv = lib.rm_mesh_occlusion, "rm_mesh_occlusion: ", abi.RM_ERR_INVALID
    out, ms = np.full(4, 7.0, F), (C.c_float * 2)(7.0, 7.0)
    for o in (native._fp(out), None):
        for at, (name, values, text) in enumerate(BAD_FIELDS):
            later = {n: v[0] for n, v, _ in BAD_FIELDS[at + 1:]}  # every later field bad as well: the earlier check speaks
            for bad in values:
                for rest in ({}, later):
                    assert call(None, None, C.byref(c_block(**{**rest, name: bad})), o, ms) == inv
                    assert last() == who + text, (name, bad, rest, last())
        # good blocks, and none (the defaults): the NULL handles are what is refused
        good = [None, c_block(), c_block(radius=2.0 ** -64), c_block(radius=2.0 ** 64), c_block(strength=0.0), c_block(strength=4.0), c_block(normal_delta=1e-30),
                c_block(flags=abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL)]
        good += [c_block(directions=k, taps=j) for k in OR.DIRECTIONS for j in OR.TAPS]
        for block in good:
            assert call(None, None, C.byref(block) if block is not None else None, o, ms) == inv and last() == who + "NULL argument"
    assert (out == 7.0).all() and list(ms) == [7.0, 7.0]  # nothing was written


PY_NAMES = ("radius", "directions", "taps", "normal_delta", "strength", "flags")


@pytest.mark.parametrize("name, bad", [(n, b) for n, values, _ in BAD_FIELDS[:-1] for b in values] +
                         [(n, b) for n in PY_NAMES for b in (None, "1", [1], True)] + [("directions", 16.0), ("taps", 4.0), ("flags", 0.0), ("radius", 1e39)])
def test_python_refuses_every_invalid_field(name, bad):
    with pytest.raises(ValueError, match="occlusion " + name):
        M.mesh_occlusion(**{name: bad})
    with pytest.raises(ValueError):
        native.Context._mesh_occlusion({name: bad})


def test_python_packs_what_it_is_given():
    assert isinstance(M.mesh_occlusion(), abi.RmMeshOcclusion)
    got = M.mesh_occlusion(radius=0.5, directions=64, taps=8, normal_delta=np.float32(0.125), strength=2, flags=abi.RM_RENDER_FAST)
    assert bytes(got) == np.array([0.5], "<f4").tobytes() + np.array([64, 8], "<i4").tobytes() + np.array([0.125, 2.0], "<f4").tobytes() + np.array([abi.RM_RENDER_FAST, 0, 0], "<i4").tobytes()
    to_c = native.Context._mesh_occlusion
    assert to_c(None) is None
    for given in (True, dict(), M.mesh_occlusion(), abi.RmMeshOcclusion(0.25, 16, 4, 2.0 ** -10, 1.0, 0)):
        assert bytes(to_c(given)) == DEFAULT_BYTES
    assert bytes(to_c(dict(taps=2, radius=1))) == bytes(M.mesh_occlusion(radius=1.0, taps=2))
    reserved = c_block(reserved=(0, 1))  # left for the library to refuse
    assert bytes(to_c(reserved)) == bytes(reserved)
    for bad in (False, 3, 0.25, "occlusion", [16], dict(tap=4), dict(taps=4, reserved=0), abi.RmMeshOcclusion(), abi.RmMeshSharp()):
        with pytest.raises(ValueError):
            to_c(bad)
    with pytest.raises(ValueError, match="unknown occlusion parameter tap"):
        M.mesh_occlusion(tap=4)
    import inspect

    sig = inspect.signature(native.Context.extract_mesh).parameters
    assert list(sig)[-1] == "occlusion" and sig["occlusion"].kind is inspect.Parameter.KEYWORD_ONLY and sig["occlusion"].default is None
    assert "occlusion" not in inspect.signature(native.Context.mesh_from_values).parameters  # no scene, no occlusion


def test_node_packs_the_occlusion_block_as_python_does():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    cases = [None, dict(), dict(radius=0.5), dict(directions=64, taps=8), dict(normalDelta=0.125, strength=2, flags=abi.RM_RENDER_FAST), dict(radius=2.0 ** -64, strength=0)]
    script = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const out = { size: r.addon.sizes().RmMeshOcclusion, defaults: r.MESH_OCCLUSION_DEFAULTS, made: r.meshOcclusion(), cases: [], bad: [],
              fns: [typeof r.meshOcclusion, typeof r.addon.meshOcclusionBlock], arity: r.RenderJobContext.prototype.extractMesh.length };
for (const c of %s) out.cases.push(hex(r.addon.meshOcclusionBlock(c === null ? null : r.meshOcclusion(c))));
for (const f of [() => r.meshOcclusion(true), () => r.meshOcclusion(16), () => r.meshOcclusion({ radius: 0 }), () => r.meshOcclusion({ radius: NaN }), () => r.meshOcclusion({ radius: 2 ** 65 }),
                 () => r.meshOcclusion({ directions: 3 }), () => r.meshOcclusion({ directions: "16" }), () => r.meshOcclusion({ directions: 128 }), () => r.meshOcclusion({ taps: 0 }),
                 () => r.meshOcclusion({ taps: 16 }), () => r.meshOcclusion({ taps: 4.5 }), () => r.meshOcclusion({ normalDelta: 0 }), () => r.meshOcclusion({ normalDelta: Infinity }),
                 () => r.meshOcclusion({ strength: -1 }), () => r.meshOcclusion({ strength: 4.5 }), () => r.meshOcclusion({ strength: null }), () => r.meshOcclusion({ flags: 4 }),
                 () => r.meshOcclusion({ flags: 0.5 }), () => r.meshOcclusion({ normal_delta: 1 }), () => r.meshOcclusion({ reserved: 0 }), () => r.addon.meshOcclusionBlock(7),
                 () => r.addon.meshOcclusionBlock()])
  try { f(); out.bad.push(false); } catch (e) { out.bad.push(true); }
console.log(JSON.stringify(out));
""" % (str(JS / "index.js"), json.dumps(cases))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["size"] == 32 and all(out["bad"]), out["bad"]
    assert out["fns"] == ["function"] * 2 and out["arity"] == 6  # the new parameter is appended behind the defaulted ones
    assert out["defaults"] == dict(radius=0.25, directions=16, taps=4, normalDelta=2.0 ** -10, strength=1, flags=0) == out["made"]
    py = dict(normalDelta="normal_delta")
    for c, got in zip(cases, out["cases"]):
        assert got == bytes(M.mesh_occlusion(**{py.get(k, k): v for k, v in (c or {}).items()})).hex(), c
    dts = (JS / "index.d.ts").read_text()
    assert "export function meshOcclusion(" in dts and "export interface MeshOcclusion " in dts and "occlusion: MeshOcclusion | true | null" in dts and "occlusion?: Float32Array" in dts


# ---- the restatement on analytic fp32 fields -----------------------------------------------------------------------------------------------------

def length(p):
    return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def sphere_sdf(p):
    return length(p) - F(1)


def sphere_normal(p):
    return p / length(p)[:, None]


def unit_directions(n, seed):
    g = np.random.default_rng(seed).standard_normal((n, 3)).astype(F)
    return g / length(g)[:, None]


def floor_and_box_sdf(p):
    """The plane z = 0 united with the unit box standing on it: [-0.5, 0.5]^2 x [0, 1]."""
    q = np.abs(p - np.array([0, 0, 0.5], F)) - F(0.5)
    outside = np.maximum(q, F(0))
    box = length(outside) + np.minimum(np.maximum(q[:, 0], np.maximum(q[:, 1], q[:, 2])), F(0))
    return np.minimum(p[:, 2], box)


def up(p):
    return np.tile(np.array([0, 0, 1], F), (len(p), 1))


def box_distance_on_the_floor(xy):
    return np.hypot(*np.maximum(np.abs(xy) - 0.5, 0.0).T)


@pytest.mark.parametrize("K, J", [(1, 1), (8, 1), (16, 4), (64, 4)])
def test_a_convex_surface_is_open(K, J):
    """500 points 1 % off a unit sphere: d is never below d0 + e, so every quantum is 0 and the result exactly 1."""
    p = (unit_directions(500, 1) * F(1.01)).astype(F)
    ao = OR.occlusion(p, sphere_sdf, sphere_normal, c_table(K), radius=0.25, taps=J)
    assert ao.dtype == F and ao.shape == (500,) and (ao == 1.0).all()


def test_a_floor_is_open_far_from_the_box_and_dark_at_its_foot():
    g = np.random.default_rng(2)
    xy = g.uniform(-2.0, 2.0, (4000, 2))
    dist = box_distance_on_the_floor(xy)
    far, near = xy[dist > 0.5], xy[(dist > 0) & (dist < 0.125)]
    assert len(far) > 1000 and len(near) > 100
    on_floor = lambda a: np.concatenate([a, np.zeros((len(a), 1))], axis=1).astype(F)
    table = c_table(16)
    ao_far = OR.occlusion(on_floor(far), floor_and_box_sdf, up, table, radius=0.25, taps=4)
    ao_near = OR.occlusion(on_floor(near), floor_and_box_sdf, up, table, radius=0.25, taps=4)
    print(f"far {ao_far.mean():.4f}; near: mean {ao_near.mean():.4f}, minimum {ao_near.min():.4f}")
    assert (ao_far == 1.0).all()  # no tap comes within reach of the box: d = e exactly, with d0 = 0
    assert ao_near.mean() < ao_far.mean() - 0.1  # (on these points the margin is 0.33; the mean depends on how the points spread over the 0.125)


def test_the_inside_of_a_sphere_is_evenly_shaded():
    p = unit_directions(500, 3)
    ao = OR.occlusion(p, lambda q: F(1) - length(q), lambda q: -sphere_normal(q), c_table(16), radius=0.25, taps=4)
    print(f"inside of a unit sphere: mean {ao.mean():.4f}, {ao.min():.4f} .. {ao.max():.4f}")
    assert abs(ao.mean() - 0.925) < 0.005 and ao.max() - ao.min() < 0.01  # the same at every point but for rounding


def test_strength_scales_and_clamps():
    p = unit_directions(64, 4)
    inside = dict(sdf=lambda q: F(1) - length(q), normal=lambda q: -sphere_normal(q), table=c_table(8), radius=0.25, taps=2)
    one, none, four = (OR.occlusion(p, strength=s, **inside) for s in (1.0, 0.0, 4.0))
    assert (none == 1.0).all() and (four < one).all() and (four >= 0).all()
    assert np.array_equal(four, (F(1) - F(4) * (F(1) - one)).astype(F))  # (1 - occ is exact here: occ is a multiple of 2^-20 below 1)
    assert len(OR.occlusion(np.zeros((0, 3), F), table=c_table(8), sdf=None, normal=None)) == 0


# ---- the writers -------------------------------------------------------------------------------------------------------------------------------------

def small_mesh(**more):
    g = np.random.default_rng(5)
    return M.Mesh(positions=g.standard_normal((5, 3)).astype(F), triangles=np.array([[0, 1, 2], [2, 3, 4]], np.uint32), **more)


def parse_ply(data):
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    props = [l.split()[1:] for l in lines if l.startswith("property") and "list" not in l]
    dtype = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    count = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    return lines, np.frombuffer(body[:count * dtype.itemsize], dtype), body[count * dtype.itemsize:]


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("colours", [False, True])
def test_encode_ply_writes_the_occlusion_as_quality_and_nothing_else_changes(normals, colours):
    g = np.random.default_rng(6)
    more = dict(normals=g.standard_normal((5, 3)).astype(F) if normals else None, colours=g.uniform(0, 1, (5, 3)).astype(F) if colours else None)
    plain = small_mesh(**more)
    assert plain.occlusion is None and small_mesh(occlusion=None, **more).occlusion is None
    lines, vertices, faces = parse_ply(M.encode_ply(plain))
    # today's bytes: the header and the layout of a mesh without an occlusion, spelt out
    want = ["ply", "format binary_little_endian 1.0", "comment hip_raymarch mesh", "element vertex 5", "property float x", "property float y", "property float z"]
    want += ["property float nx", "property float ny", "property float nz"] * normals + ["property uchar red", "property uchar green", "property uchar blue"] * colours
    want += ["element face 2", "property list uchar uint vertex_indices"]
    assert lines == want and len(M.encode_ply(plain)) == len("\n".join(want)) + 1 + len("end_header\n") + 5 * (12 + 12 * normals + 3 * colours) + 2 * 13
    assert M.encode_ply(small_mesh(occlusion=None, **more)) == M.encode_ply(plain)
    ao = np.array([0.0, 1.0, 0.25, np.float32(1 / 3), 0.999999], F)
    shaded_lines, shaded_vertices, shaded_faces = parse_ply(M.encode_ply(small_mesh(occlusion=ao, **more)))
    at = shaded_lines.index("property float quality")
    assert shaded_lines[:at] + shaded_lines[at + 1:] == lines and shaded_lines[at + 1] == "element face 2"  # behind the colours, the last vertex property
    assert np.array_equal(shaded_vertices["quality"].view(np.uint32), ao.view(np.uint32)) and shaded_faces == faces
    for name in vertices.dtype.names:
        assert np.array_equal(shaded_vertices[name], vertices[name])


def test_node_writes_the_same_ply_bytes():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    g = np.random.default_rng(7)
    ao = g.uniform(0, 1, 5).astype(F)
    meshes = [small_mesh(occlusion=ao), small_mesh(occlusion=ao, normals=g.standard_normal((5, 3)).astype(F), colours=g.uniform(0, 1, (5, 3)).astype(F)), small_mesh()]
    as_js = lambda m: {k: (None if v is None else [float(x) for x in np.asarray(v).ravel()]) for k, v in
                       dict(positions=m.positions, triangles=m.triangles, normals=m.normals, colours=m.colours, occlusion=m.occlusion).items()}
    script = """
const r = require(%r);
const f32 = (a) => a === null ? null : new Float32Array(a);
console.log(JSON.stringify(%s.map((m) => r.encodePly({ positions: f32(m.positions), triangles: new Uint32Array(m.triangles), normals: f32(m.normals), colours: f32(m.colours),
                                                        occlusion: f32(m.occlusion) }).toString("hex"))));
""" % (str(JS / "index.js"), json.dumps([as_js(m) for m in meshes]))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out == [M.encode_ply(m).hex() for m in meshes]


def test_shaded():
    g = np.random.default_rng(8)
    ao = np.array([0.0, 1.0, 0.25, 0.5, 0.75], F)
    colours = g.uniform(0, 1, (5, 3)).astype(F)
    coloured, grey = small_mesh(occlusion=ao, colours=colours), small_mesh(occlusion=ao)
    a, b = M.shaded(coloured), M.shaded(grey)
    assert a is not coloured and a.colours.dtype == F and np.array_equal(a.colours, colours * ao[:, None]) and np.array_equal(coloured.colours, colours)
    assert np.array_equal(b.colours, np.repeat(ao[:, None], 3, axis=1)) and grey.colours is None  # a copy: the mesh given is as it was
    for made, given in ((a, coloured), (b, grey)):
        assert made.positions is given.positions and made.triangles is given.triangles and made.occlusion is given.occlusion
    assert b"property uchar red" in M.encode_ply(b) and b"property float quality" in M.encode_ply(b)
    with pytest.raises(ValueError):
        M.shaded(small_mesh())
