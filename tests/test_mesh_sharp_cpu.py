"""Sharp vertices without a GPU: the ABI of rm_mesh_extract_sharp, every refusal that is made before the handles are looked at, the two
hosts' packing of RmMeshSharp, and the numpy restatement (tests/mesh_sharp_ref.py) on an analytic box: its accuracy against the float64
surface and its invariants."""
import ctypes as C
import json
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mesh_ref as MR
import mesh_sharp_ref as SR
from raymarching_engine_amd import abi, mesh as M, native
from test_mesh_cpu import BAD_GRIDS, BAD_PARAMS, c_grid, c_params

ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
ENTRY_POINTS = ("rm_mesh_sharp_default", "rm_mesh_extract_sharp")

# the off-grid axis-aligned box of the accuracy condition, on [-1, 1]^3
BOX_CENTRE, BOX_HALF = (0.031, -0.017, 0.023), (0.52, 0.41, 0.63)
BOX_LO, BOX_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
BOX_CELLS = (16, 24)


def box_sdf(points, dtype):
    """The signed distance of the box, every operation in `dtype`."""
    p = np.asarray(points, dtype)
    q = np.abs(p - np.asarray(BOX_CENTRE, dtype)) - np.asarray(BOX_HALF, dtype)
    outside = np.sqrt((np.maximum(q, dtype(0)) ** 2).sum(-1, dtype=dtype))
    return (outside + np.minimum(q.max(-1), dtype(0))).astype(dtype)


def box_sdf32(points):
    return box_sdf(points, F)


def box_normal32(points, delta):
    """fp32 forward differences, not normalised: (sdf(p + delta e_k) - sdf(p)) / delta."""
    p = np.asarray(points, F)
    d0 = box_sdf32(p)
    out = np.empty(p.shape, F)
    for k in range(3):
        q = p.copy()
        q[:, k] = q[:, k] + F(delta)
        out[:, k] = (box_sdf32(q) - d0) / F(delta)
    return out


def zero_normal(points, delta):
    return np.zeros(np.asarray(points).shape, F)


def box_case(n):
    """(cells per axis, surface-nets mesh, corner values, axes) of the box on n^3 cells: computed once per size."""
    if n not in box_case.cache:
        nn = (n, n, n)
        values = box_sdf32(MR.corner_positions(BOX_LO, BOX_HI, nn))
        box_case.cache[n] = (nn, MR.surface_nets(BOX_LO, BOX_HI, nn, values), values, MR.axes(BOX_LO, BOX_HI, nn))
    return box_case.cache[n]


box_case.cache = {}


def worst_distance_in_cells(positions, n):
    """max |float64 analytic distance| over the vertices, in units of the cell size h = 2 / n."""
    return float(np.abs(box_sdf(np.asarray(positions, np.float64), np.float64)).max() / (2.0 / n))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) {name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshSharp",) + ENTRY_POINTS)
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(ENTRY_POINTS) <= exported


def test_defaults_and_struct_layout():
    lib = native.load_library()
    s = abi.RmMeshSharp(refine=3, normal_delta=1.0, threshold=0.5, reserved=9)
    lib.rm_mesh_sharp_default(C.byref(s))
    lib.rm_mesh_sharp_default(None)  # a no-op
    assert (s.refine, s.normal_delta, s.threshold, s.reserved) == (6, 2.0 ** -10, float(F(0.1)), 0)
    assert bytes(s) == bytes(M.mesh_sharp()) and abi.MESH_SHARP_DEFAULTS == dict(refine=6, normal_delta=2.0 ** -10, threshold=0.1)
    assert abi.MESH_DEFAULTS == dict(iso=0.0, normals=1, normal_delta=1e-5, colours=0, flags=0)  # as it was
    assert C.sizeof(abi.RmMeshSharp) == 16
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct layout from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\n'
                       'int main(void){ printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(RmMeshSharp), offsetof(RmMeshSharp, refine), offsetof(RmMeshSharp, normal_delta), '
                       'offsetof(RmMeshSharp, threshold), offsetof(RmMeshSharp, reserved), sizeof(RmMeshParams)); return 0; }\n')
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 0, 4, 8, 12, 24]
    assert [abi.RmMeshSharp.refine.offset, abi.RmMeshSharp.normal_delta.offset, abi.RmMeshSharp.threshold.offset, abi.RmMeshSharp.reserved.offset] == [0, 4, 8, 12]


def test_node_packs_the_sharp_block_as_python_does():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    cases = [{}, dict(refine=0), dict(refine=16, normalDelta=1e-5, threshold=0.0), dict(threshold=0.9), dict(normalDelta=0.125, refine=3)]
    script = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const out = { size: r.addon.sizes().RmMeshSharp, defaults: r.meshSharp(), same: r.MESH_SHARP_DEFAULTS, none: hex(r.addon.meshSharpBlock(null)), cases: [], bad: [],
              params: r.meshParams(), fns: [typeof r.meshSharp, typeof r.addon.meshSharpBlock, typeof r.RenderJobContext.prototype.extractMesh] };
for (const c of %s) out.cases.push(hex(r.addon.meshSharpBlock(r.meshSharp(c))));
for (const f of [() => r.meshSharp({ refine: -1 }), () => r.meshSharp({ refine: 17 }), () => r.meshSharp({ refine: 1.5 }), () => r.meshSharp({ refine: "6" }),
                 () => r.meshSharp({ normalDelta: 0 }), () => r.meshSharp({ normalDelta: -1 }), () => r.meshSharp({ normalDelta: NaN }), () => r.meshSharp({ normalDelta: Infinity }),
                 () => r.meshSharp({ normalDelta: 1e-60 }), () => r.meshSharp({ threshold: -0.1 }), () => r.meshSharp({ threshold: 1 }), () => r.meshSharp({ threshold: NaN }),
                 () => r.meshSharp({ threshold: 0.99999999999 }), () => r.meshSharp({ reserved: 0 }), () => r.meshSharp({ normal_delta: 1e-3 }), () => r.meshSharp(3)])
  try { f(); out.bad.push(false); } catch (e) { out.bad.push(true); }
console.log(JSON.stringify(out));
""" % (str(JS / "index.js"), json.dumps(cases))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["size"] == 16 and all(out["bad"]) and out["fns"] == ["function"] * 3
    assert out["defaults"] == out["same"] == dict(refine=6, normalDelta=2.0 ** -10, threshold=0.1)
    assert out["params"] == dict(iso=0.0, normals=1, normalDelta=1e-5, colours=0, flags=0)  # meshParams is as it was
    assert out["none"] == bytes(M.mesh_sharp()).hex()
    for c, got in zip(cases, out["cases"]):
        kw = {("normal_delta" if k == "normalDelta" else k): v for k, v in c.items()}
        assert got == bytes(M.mesh_sharp(**kw)).hex(), c


# ---- the refusals made before the handles are looked at ------------------------------------------------------------------------------

def c_sharp(**fields):
    s = abi.RmMeshSharp()
    native.load_library().rm_mesh_sharp_default(C.byref(s))
    for k, v in fields.items():
        setattr(s, k, v)
    return s


BAD_SHARP = [(dict(refine=-1), "refine"), (dict(refine=17), "refine"), (dict(refine=1 << 20), "refine"), (dict(normal_delta=0.0), "normal_delta"),
             (dict(normal_delta=-1e-3), "normal_delta"), (dict(normal_delta=float("nan")), "normal_delta"), (dict(normal_delta=float("inf")), "normal_delta"),
             (dict(threshold=-0.125), "threshold"), (dict(threshold=1.0), "threshold"), (dict(threshold=2.0), "threshold"), (dict(threshold=float("nan")), "threshold"),
             (dict(threshold=float("inf")), "threshold"), (dict(reserved=1), "reserved"), (dict(reserved=-1), "reserved")]


def test_every_refusal_speaks_before_the_handles_and_in_order():
    """No context exists without a GPU: every call ends in RM_ERR_INVALID, and the text (rm_last_error(NULL)) tells which check spoke."""
    lib = native.load_library()
    out = C.c_void_p()
    who = "rm_mesh_extract_sharp"
    last = lambda: lib.rm_last_error(None).decode()
    call = lambda g, p, s: lib.rm_mesh_extract_sharp(None, None, g, p, s, C.byref(out))
    good, ok, fine = c_grid(), c_params(), c_sharp()
    # everything valid, NULL params and NULL sharp included (the defaults): the NULL handles are what is refused
    for p in (C.byref(ok), None):
        for s in (C.byref(fine), None):
            assert call(C.byref(good), p, s) == abi.RM_ERR_INVALID and last() == who + ": NULL argument"
    assert lib.rm_mesh_extract_sharp(None, None, C.byref(good), None, None, None) == abi.RM_ERR_INVALID and last() == who + ": NULL argument"
    for fields in (dict(refine=0), dict(refine=16), dict(threshold=0.0), dict(threshold=float(np.nextafter(F(1), F(0)))), dict(normal_delta=1e-30)):
        assert call(C.byref(good), C.byref(ok), C.byref(c_sharp(**fields))) == abi.RM_ERR_INVALID and last() == who + ": NULL argument", fields
    # 1: what rm_mesh_extract refuses, first -- even beside a bad sharp block
    wrong = c_sharp(refine=99, reserved=3)
    for bad in BAD_GRIDS + [None]:
        g = C.byref(c_grid(**bad)) if bad is not None else None
        for s in (C.byref(fine), C.byref(wrong), None):
            assert call(g, C.byref(ok), s) == abi.RM_ERR_INVALID and re.match(rf"{who}: (grid|NULL grid)", last()), (bad, last())
    for fields, word in BAD_PARAMS:
        for s in (C.byref(fine), C.byref(wrong), None):
            assert call(C.byref(good), C.byref(c_params(**fields)), s) == abi.RM_ERR_INVALID and last().startswith(f"{who}: {word}"), (fields, last())
    # 2: the sharp block, at that same point
    for fields, word in BAD_SHARP:
        for p in (C.byref(ok), None):
            assert call(C.byref(good), p, C.byref(c_sharp(**fields))) == abi.RM_ERR_INVALID and last().startswith(f"{who}: sharp {word}"), (fields, last())
    # rm_mesh_extract itself is as it was
    assert lib.rm_mesh_extract(None, None, C.byref(good), C.byref(ok), C.byref(out)) == abi.RM_ERR_INVALID and last() == "rm_mesh_extract: NULL argument"


@pytest.mark.parametrize("bad", [dict(refine=-1), dict(refine=17), dict(refine=1.0), dict(refine=True), dict(refine="6"), dict(normal_delta=0.0), dict(normal_delta=-1e-3),
                                 dict(normal_delta=float("nan")), dict(normal_delta=float("inf")), dict(normal_delta=1e-60), dict(normal_delta="1"), dict(threshold=-0.125),
                                 dict(threshold=1.0), dict(threshold=0.99999999999), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=None),
                                 dict(reserved=0), dict(normalDelta=1e-3), dict(iso=0.0)])
def test_python_refuses_bad_sharp_parameters(bad):
    with pytest.raises(ValueError):
        M.mesh_sharp(**bad)


def test_python_packs_what_it_is_given():
    s = M.mesh_sharp(refine=0, normal_delta=1e-5, threshold=0.9)
    assert (s.refine, s.normal_delta, s.threshold, s.reserved) == (0, float(F(1e-5)), float(F(0.9)), 0)
    assert bytes(M.mesh_sharp(refine=np.int64(16), threshold=np.float32(0.0))) == bytes(abi.RmMeshSharp(16, 2.0 ** -10, 0.0, 0))
    assert bytes(M.mesh_params()) == bytes(c_params())  # mesh_params is as it was


# ---- the restatement on the analytic box ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", BOX_CELLS)
def test_restatement_puts_the_vertices_of_a_box_on_its_surface(n):
    """Worst |d| against the float64 analytic box, in cells.  Measured with this file's fp32 box and forward differences: surface nets 0.517
    (16^3) and 0.519 (24^3); sharp, the defaults, 3.0e-7 and 4.5e-7.  The bar h / 256 is a condition, not a measurement: it leaves room for another unit's square root
    and the order of operations of a table evaluator, and stays more than 100 times below what surface nets can reach (its vertex is a mean
    of crossings: half a cell off at a corner)."""
    nn, (nets, tri, cells), values, axes = box_case(n)
    plain = worst_distance_in_cells(nets, n)
    sharp = SR.sharp_positions(cells, values, axes, box_sdf32, box_normal32, nets=nets)
    got = worst_distance_in_cells(sharp, n)
    print(f"box {n}^3: {len(nets)} vertices; worst |d| / h: surface nets {plain:.4g}, sharp {got:.4g}")
    assert plain > 0.4  # the condition on the input: surface nets bevels this box
    assert got <= 1.0 / 256.0
    assert sharp.dtype == F and sharp.shape == nets.shape
    assert MR.inside_cell_boxes(BOX_LO, BOX_HI, nn, sharp, cells)


@pytest.mark.parametrize("n", BOX_CELLS)
def test_without_bisection_the_box_is_missed(n):
    """refine = 0: linear crossings only.  Along a grid edge near an edge of the box the distance is not linear, so the planes are misplaced and
    the vertices stay off the surface -- 0.119 h and 0.116 h measured.  That the defaults pass the bar above is therefore the bisection rounds' doing."""
    nn, (nets, tri, cells), values, axes = box_case(n)
    got = worst_distance_in_cells(SR.sharp_positions(cells, values, axes, box_sdf32, box_normal32, refine=0, nets=nets), n)
    print(f"box {n}^3, refine 0: worst |d| / h {got:.4g}")
    assert not got <= 1.0 / 16.0


# ---- invariants of the restatement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(refine=0), dict(refine=16), dict(threshold=0.0), dict(threshold=0.9), dict(normal_delta=1e-5)], ids=str)
def test_every_vertex_stays_in_its_cell(kw):
    nn, (nets, tri, cells), values, axes = box_case(16)
    pos = SR.sharp_positions(cells, values, axes, box_sdf32, box_normal32, nets=nets, **kw)
    assert np.isfinite(pos).all() and MR.inside_cell_boxes(BOX_LO, BOX_HI, nn, pos, cells)
    # ... also with normals that send the minimiser far away: the clamp holds it
    wild = lambda p, d: (np.asarray(p, F) * F(1e3) + F(1)).astype(F)
    pos = SR.sharp_positions(cells, values, axes, box_sdf32, wild, nets=nets, **kw)
    assert np.isfinite(pos).all() and MR.inside_cell_boxes(BOX_LO, BOX_HI, nn, pos, cells)


def test_zero_normals_give_the_mass_points():
    nn, (nets, tri, cells), values, axes = box_case(16)
    pos, mass, live = SR.sharp_positions(cells, values, axes, box_sdf32, zero_normal, nets=nets, details=True)
    assert live.any(0).all() and np.array_equal(pos.view(np.uint32), mass.view(np.uint32))
    nan = lambda p, d: np.full(np.asarray(p).shape, np.nan, F)
    assert np.array_equal(SR.sharp_positions(cells, values, axes, box_sdf32, nan, nets=nets).view(np.uint32), mass.view(np.uint32))
    # and they differ from the QEF's: the normals are used
    assert not np.array_equal(SR.sharp_positions(cells, values, axes, box_sdf32, box_normal32, nets=nets), mass)


@pytest.mark.parametrize("n", BOX_CELLS)
def test_refine_0_and_zero_normals_give_surface_nets_bit_for_bit(n):
    nn, (nets, tri, cells), values, axes = box_case(n)

    def never(points):
        raise AssertionError("refine = 0 evaluates no distance")

    pos = SR.sharp_positions(cells, values, axes, never, zero_normal, refine=0)
    assert np.array_equal(pos.view(np.uint32), nets.view(np.uint32))
    v = np.random.default_rng(5).standard_normal((8, 9, 10)).astype(F)  # and on a field of noise, at another level
    lo, hi, nn = (-1.0, 0.0, 0.5), (1.0, 3.0, 0.75), (9, 8, 7)
    nets, tri, cells = MR.surface_nets(lo, hi, nn, v, 0.125)
    pos = SR.sharp_positions(cells, v, MR.axes(lo, hi, nn), never, zero_normal, iso=0.125, refine=0)
    assert len(nets) > 0 and np.array_equal(pos.view(np.uint32), nets.view(np.uint32))
