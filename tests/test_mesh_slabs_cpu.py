"""Slabbed extraction without a GPU: the numpy restatement of the two-pass procedure (tests/mesh_slabs_ref.py) against mesh_ref.surface_nets
for every `layers`, the ABI of rm_mesh_extract_slabs / _sharp_slabs / rm_mesh_from_values_slabs, the refusals made before the handles are
looked at, in their order, the Python host's checks and the Node block."""
import ctypes as C
import inspect
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_ref as MR
import mesh_slabs_ref as WR
from raymarching_engine_amd import abi, mesh as M, native
from test_mesh_cpu import BAD_GRIDS, BAD_PARAMS, c_grid, c_params, special_field

ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
ENTRY_POINTS = ("rm_mesh_slabs_default", "rm_mesh_extract_slabs", "rm_mesh_extract_sharp_slabs", "rm_mesh_from_values_slabs")
GRIDS = [(5, 4, 7), (3, 3, 1), (2, 2, 2), (9, 6, 12)]
LO, HI = (-1.3, -1.2, -1.4), (1.25, 1.3, 1.35)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

def fields(n):
    """name -> values on the grid (LO, HI, n): special values, every cell active, and the two analytic shapes"""
    rng = np.random.default_rng(sum(n))
    shape = (n[2] + 1, n[1] + 1, n[0] + 1)
    p = MR.corner_positions(LO, HI, n).astype(np.float64)
    checker = (np.indices(shape).sum(axis=0) % 2) * 2 - 1  # neighbours differ in sign: every cell is active, every inner edge owns a quad
    return {"special": special_field(n, 11),
            "dense": ((rng.random(shape) + 0.25) * checker).astype(F),
            "random": rng.standard_normal(shape).astype(F),
            "sphere": (np.linalg.norm(p, axis=1) - 0.9).astype(F).reshape(shape),
            "torus": (np.hypot(np.hypot(p[:, 0], p[:, 2]) - 0.8, p[:, 1]) - 0.3).astype(F).reshape(shape)}


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("n", GRIDS)
def test_the_slabbed_restatement_is_surface_nets_for_every_layers(n):
    for name, values in fields(n).items():
        ref = MR.surface_nets(LO, HI, n, values)
        if name == "dense":
            assert len(ref[0]) == n[0] * n[1] * n[2]  # every cell is active
        for layers in range(1, n[2] + 2):
            stats = {}
            got = WR.surface_nets_slabs(LO, HI, n, values, 0.0, layers, stats)
            assert same(got, ref), (name, layers)
            assert stats["layers"] == min(layers, n[2]) and len(stats["totals"]) == -(-n[2] // stats["layers"])
            assert sum(t[0] for t in stats["totals"]) == len(ref[0]) and 2 * sum(t[1] for t in stats["totals"]) == len(ref[1])
        assert same(WR.surface_nets_slabs(LO, HI, n, values, 0.0, 0), ref)  # the default: one slab on grids this small


def test_empty_slabs_are_skipped_and_an_iso_away_from_the_field_gives_nothing():
    n = (9, 6, 12)
    values = fields(n)["sphere"]
    stats = {}
    got = WR.surface_nets_slabs(LO, HI, n, values, 0.0, 1, stats)
    assert same(got, MR.surface_nets(LO, HI, n, values)) and len(stats["skipped"]) >= 2 and stats["totals"][0] == (0, 0)  # the sphere ends inside the grid
    p, t, c = WR.surface_nets_slabs(LO, HI, n, values, 50.0, 2, stats)
    assert p.shape == (0, 3) and t.shape == (0, 3) and c.shape == (0,) and stats["skipped"] == list(range(6))


def test_the_layer_rule():
    assert WR.slab_layers((4, 4, 9), 3) == 3 and WR.slab_layers((4, 4, 9), 10) == 9 and WR.slab_layers((4, 4, 9), 0) == 9
    assert WR.slab_layers((1024, 1024, 1024), 0) == (1 << 26) // (1025 * 1025) - 2 == 61
    assert WR.slab_layers((1024, 1024, 1024), 253) == 253  # 255 * 1025^2 <= 2^28
    for layers in (254, 300, 5000):  # 300 is clamped to nothing below nz: the window itself is too large
        with pytest.raises(ValueError):
            WR.slab_layers((1024, 1024, 1024), layers)
    with pytest.raises(ValueError):
        WR.slab_layers((4, 4, 4), -1)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) {name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshSlabs",) + ENTRY_POINTS)
    assert m.group(1).rstrip().endswith("(additions only)")
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert set(ENTRY_POINTS) <= {line.split()[-1] for line in out.splitlines() if line.split()}
    assert "slabbed extraction" in header and "HALO" in header
    dts = (JS / "index.d.ts").read_text()
    assert "export interface MeshSlabs " in dts and "export function meshSlabs(" in dts and "slabs: MeshSlabs | number | true | null): Mesh;" in dts
    assert "opts: { slabs?: boolean } | null): MeshGrid;" in dts and "MESH_SLABS_DEFAULTS" in dts


def test_struct_size_and_defaults():
    assert C.sizeof(abi.RmMeshSlabs) == 8 and [n for n, _ in abi.RmMeshSlabs._fields_] == ["layers", "reserved"]
    assert abi.RmMeshSlabs.layers.offset == 0 and abi.RmMeshSlabs.reserved.offset == 4
    s = abi.RmMeshSlabs(layers=7, reserved=7)
    native.load_library().rm_mesh_slabs_default(C.byref(s))
    assert (s.layers, s.reserved) == (0, 0) and abi.MESH_SLABS_DEFAULTS == dict(layers=0)
    native.load_library().rm_mesh_slabs_default(None)
    made = M.mesh_slabs()
    assert bytes(made) == bytes(s) and bytes(M.mesh_slabs(layers=5)) == bytes(abi.RmMeshSlabs(layers=5))


def c_slabs(layers=0, reserved=0):
    return abi.RmMeshSlabs(layers=layers, reserved=reserved)


def c_sharp(**fields):
    s = abi.RmMeshSharp()
    native.load_library().rm_mesh_sharp_default(C.byref(s))
    for k, v in fields.items():
        setattr(s, k, v)
    return s


BIG = dict(lo=(-1, -1, -1), hi=(1, 1, 1), n=(1024, 1024, 1024))
BAD_SLABS = [(dict(layers=-1), "slabs layers"), (dict(reserved=1), "slabs reserved"), (dict(layers=-5, reserved=1), "slabs layers")]
BAD_SHARP = [(dict(refine=17), "sharp refine"), (dict(normal_delta=0.0), "sharp normal_delta"), (dict(threshold=1.0), "sharp threshold"), (dict(reserved=1), "sharp reserved")]


def test_refusals_speak_before_the_handles_and_in_the_stated_order():
    """No context exists without a GPU: every call ends in RM_ERR_INVALID, and the text tells which check spoke."""
    lib = native.load_library()
    out = C.c_void_p()
    last = lambda: lib.rm_last_error(None).decode()
    good, ok, sharp, slabs = c_grid(), c_params(), c_sharp(), c_slabs()
    plain = lambda g=good, p=ok, w=slabs: lib.rm_mesh_extract_slabs(None, None, C.byref(g) if g else None, C.byref(p) if p else None, C.byref(w) if w else None, C.byref(out))
    sharped = lambda g=good, p=ok, s=sharp, w=slabs: lib.rm_mesh_extract_sharp_slabs(None, None, C.byref(g) if g else None, C.byref(p) if p else None,
                                                                                  C.byref(s) if s else None, C.byref(w) if w else None, C.byref(out))
    valued = lambda g=good, iso=0.0, w=slabs: lib.rm_mesh_from_values_slabs(None, C.byref(g) if g else None, None, iso, C.byref(w) if w else None, C.byref(out))
    names = ((plain, "rm_mesh_extract_slabs"), (sharped, "rm_mesh_extract_sharp_slabs"), (valued, "rm_mesh_from_values_slabs"))
    # everything valid, NULL blocks included: the NULL handles are what is refused
    for call, who in names:
        assert call() == abi.RM_ERR_INVALID and last() == who + ": NULL argument"
        assert call(w=None) == abi.RM_ERR_INVALID and last() == who + ": NULL argument"
    assert plain(p=None) == abi.RM_ERR_INVALID and last() == "rm_mesh_extract_slabs: NULL argument"
    assert sharped(s=None) == abi.RM_ERR_INVALID and last() == "rm_mesh_extract_sharp_slabs: NULL argument"
    # 1. the grid: RmGrid's rule ...
    for bad in BAD_GRIDS + [None]:
        if bad is not None and bad.get("n") == (1024, 1024, 255):
            continue  # (more than 2^28 corners: what these entries are for)
        g = c_grid(**bad) if bad is not None else None
        for call, who in names:
            assert call(g=g, w=c_slabs(layers=-1)) == abi.RM_ERR_INVALID and re.match(rf"{who}: (grid|NULL grid)", last()), (who, bad, last())
    # ... without the bound on the corners: 1025^3 of them pass here, and rm_mesh_extract still refuses them
    big = c_grid(**BIG)
    for call, who in names:
        assert call(g=big) == abi.RM_ERR_INVALID and last() == who + ": NULL argument"
        assert call(g=c_grid(n=(1024, 1024, 255))) == abi.RM_ERR_INVALID and last() == who + ": NULL argument"
    assert lib.rm_mesh_extract(None, None, C.byref(big), C.byref(ok), C.byref(out)) == abi.RM_ERR_INVALID
    assert last() == "rm_mesh_extract: grid must have at most 2^28 corners"
    assert lib.rm_mesh_from_values(None, C.byref(big), None, 0.0, C.byref(out)) == abi.RM_ERR_INVALID and "at most 2^28 corners" in last()
    assert lib.rm_grid_axis(C.byref(big), 0, (C.c_float * 1025)()) == abi.RM_ERR_INVALID and "at most 2^28 corners" in last()
    # 2. params (iso for the values entry), ahead of sharp and slabs
    for fields, word in BAD_PARAMS:
        assert plain(p=c_params(**fields), w=c_slabs(layers=-1)) == abi.RM_ERR_INVALID and last().startswith("rm_mesh_extract_slabs: " + word), (fields, last())
        assert sharped(p=c_params(**fields), s=c_sharp(refine=17), w=c_slabs(layers=-1)) == abi.RM_ERR_INVALID
        assert last().startswith("rm_mesh_extract_sharp_slabs: " + word), (fields, last())
    for iso in (float("nan"), float("inf")):
        assert valued(iso=iso, w=c_slabs(layers=-1)) == abi.RM_ERR_INVALID and last() == "rm_mesh_from_values_slabs: iso must be finite"
    # 3. sharp, ahead of slabs
    for fields, word in BAD_SHARP:
        assert sharped(s=c_sharp(**fields), w=c_slabs(layers=-1)) == abi.RM_ERR_INVALID and last().startswith("rm_mesh_extract_sharp_slabs: " + word), (fields, last())
    # 4. slabs
    for fields, word in BAD_SLABS:
        for call, who in names:
            assert call(w=c_slabs(**fields)) == abi.RM_ERR_INVALID and last().startswith(f"{who}: {word}"), (who, fields, last())
    for call, who in names:
        assert call(g=big, w=c_slabs(layers=300)) == abi.RM_ERR_INVALID and last().startswith(who + ": slab window"), last()
        assert call(g=big, w=c_slabs(layers=254)) == abi.RM_ERR_INVALID and last().startswith(who + ": slab window"), last()
        for layers in (0, 1, 13, 253):  # admissible windows: then the handles
            assert call(g=big, w=c_slabs(layers=layers)) == abi.RM_ERR_INVALID and last() == who + ": NULL argument", layers
        assert call(w=c_slabs(layers=2 ** 31 - 1)) == abi.RM_ERR_INVALID and last() == who + ": NULL argument"  # above nz: nz
    assert out.value is None


# ---- the Python host ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [-1, 1.5, "3", True, None, 2 ** 31])
def test_python_refuses_bad_layers(bad):
    with pytest.raises(ValueError):
        M.mesh_slabs(layers=bad)


def test_the_slabs_argument_of_the_python_host():
    for fn in (native.Context.extract_mesh, native.Context.mesh_from_values):
        sig = inspect.signature(fn).parameters
        assert sig["slabs"].kind is inspect.Parameter.KEYWORD_ONLY and sig["slabs"].default is None
    small, big = M.Grid((0, 0, 0), (1, 1, 1), (2, 2, 2)), M.Grid((-1,) * 3, (1,) * 3, (1024,) * 3, slabs=True)
    block = native.Context._mesh_slabs
    assert block(None, small) is None
    assert bytes(block(True, small)) == bytes(abi.RmMeshSlabs()) and bytes(block(0, big)) == bytes(abi.RmMeshSlabs())
    for value in (4, np.int64(4), dict(layers=4), abi.RmMeshSlabs(layers=4)):
        assert bytes(block(value, small)) == bytes(abi.RmMeshSlabs(layers=4)), value
    assert block(abi.RmMeshSlabs(layers=1, reserved=3), small).reserved == 3  # left for the library to refuse
    for bad in (-1, dict(layers=-1), dict(rows=2), abi.RmMeshSlabs(layers=-2), "4", 2.0, False):
        with pytest.raises(ValueError):
            block(bad, small)
    with pytest.raises(ValueError, match="slabs"):
        block(None, big)  # a grid beyond the cap cannot go to the dense entries


def test_grid_with_slabs_lifts_the_corner_cap_and_nothing_else():
    with pytest.raises(ValueError, match="2\\^28"):
        M.Grid((-1,) * 3, (1,) * 3, (1024,) * 3)
    g = M.Grid((-1,) * 3, (1,) * 3, (1024,) * 3, slabs=True)
    assert g.slabs and g.corners == 1025 ** 3 and g.cells == 1 << 30 and g.shape == (1025,) * 3 and tuple(g.to_c().n) == (1024,) * 3
    plain = M.Grid((0, 0, 0), (1, 1, 1), (2, 3, 4))
    assert plain.slabs is False and list(inspect.signature(M.Grid.__init__).parameters) == ["self", "lo", "hi", "n", "slabs"]
    for bad in (dict(n=(0, 2, 2)), dict(n=(2, 1025, 2)), dict(lo=(float("nan"), 0, 0)), dict(lo=(1, 0, 0)), dict(n=(2.5, 2, 2))):
        with pytest.raises(ValueError):
            M.Grid(bad.get("lo", (0, 0, 0)), bad.get("hi", (1, 1, 1)), bad.get("n", (2, 2, 2)), slabs=True)
    lo, hi, n = (-2.5, 0.1, -1e-3), (2.5, 0.7, 1e3), (1024, 1000, 777)  # inexact cell sizes, 2^29.6 corners
    big = M.Grid(lo, hi, n, slabs=True)
    for a in range(3):
        got, ref = big.axis(a), MR.axis(lo[a], hi[a], n[a])
        assert got.shape == (n[a] + 1,) and got.tobytes() == ref.tobytes(), a
    small = M.Grid(LO, HI, (5, 4, 7), slabs=True)  # ... and below the cap it is the plain grid's axis
    assert all(small.axis(a).tobytes() == M.Grid(LO, HI, (5, 4, 7)).axis(a).tobytes() for a in range(3))


# ---- Node ---------------------------------------------------------------------------------------------------------------------------------------

def test_node_packs_the_slabs_block_as_python_does():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    script = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const out = { size: r.addon.sizes().RmMeshSlabs, defaults: r.meshSlabs(), same: r.MESH_SLABS_DEFAULTS, none: hex(r.addon.meshSlabsBlock(null)), cases: [], bad: [], calls: [],
              fns: [typeof r.addon.extractMeshSlabs, typeof r.addon.meshFromValuesSlabs], grids: [] };
for (const layers of [0, 1, 13, 1024]) out.cases.push(hex(r.addon.meshSlabsBlock(r.meshSlabs({ layers }))));
for (const bad of [{ layers: -1 }, { layers: 1.5 }, { layers: "3" }, { rows: 2 }, 7]) { try { r.meshSlabs(bad); out.bad.push(false); } catch (e) { out.bad.push(true); } }
try { r.meshGrid([-1, -1, -1], [1, 1, 1], [1024, 1024, 1024]); out.grids.push(false); } catch (e) { out.grids.push(true); }
const big = r.meshGrid([-1, -1, -1], [1, 1, 1], [1024, 1024, 1024], { slabs: true });
out.grids.push(big.slabs === true, !("slabs" in r.meshGrid([0, 0, 0], [1, 1, 1], [2, 2, 2])));
r.addon.extractMeshSlabs = (...a) => { out.calls.push(["extractMeshSlabs", a.length, a[3], a[11]]); return {}; };
r.addon.meshFromValuesSlabs = (...a) => { out.calls.push(["meshFromValuesSlabs", a.length, a[4], a[9]]); return {}; };
r.addon.extractMesh = (...a) => { out.calls.push(["extractMesh", a.length]); return {}; };
const ctx = Object.create(r.RenderJobContext.prototype);
ctx.ctx = "ctx"; ctx.sceneHandle = () => "scene";
const g = r.meshGrid([0, 0, 0], [1, 1, 1], [2, 2, 2]), v = new Float32Array(27);
ctx.extractMesh(null, g); ctx.extractMesh(null, g, null, null, null, false, null, null, null, false, null);
ctx.extractMesh(null, g, null, null, null, false, null, null, null, false, true); ctx.extractMesh(null, big, null, true, true, true, null, null, true, true, 4);
ctx.extractMesh(null, g, null, null, null, false, null, null, null, false, { layers: 2 });
ctx.meshFromValues(g, v, 0, null, false, null, null, false, 3);
try { ctx.extractMesh(null, big); out.grids.push(false); } catch (e) { out.grids.push(true); }
out.arity = [r.RenderJobContext.prototype.extractMesh.length, r.RenderJobContext.prototype.meshFromValues.length];
console.log(JSON.stringify(out));
""" % str(JS / "index.js")
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["size"] == 8 and out["defaults"] == out["same"] == dict(layers=0) and out["fns"] == ["function", "function"]
    assert out["none"] == bytes(abi.RmMeshSlabs()).hex()
    assert out["cases"] == [bytes(M.mesh_slabs(layers=k)).hex() for k in (0, 1, 13, 1024)]
    assert out["bad"] == [True] * 5 and out["grids"] == [True, True, True, True] and out["arity"] == [6, 2]
    assert out["calls"] == [["extractMesh", 4], ["extractMesh", 4], ["extractMeshSlabs", 12, dict(layers=0), False], ["extractMeshSlabs", 12, dict(layers=4), True],
                            ["extractMeshSlabs", 12, dict(layers=2), False], ["meshFromValuesSlabs", 10, dict(layers=3), False]]
