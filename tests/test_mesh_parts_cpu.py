"""Components and islands without a GPU: the ABI of rm_mesh_components / rm_mesh_components_download / rm_mesh_filter, every refusal that is
made before the handles are looked at, the two hosts' packing of RmMeshKeep, and the numpy restatement (tests/mesh_parts_ref.py) on the meshes
the GPU tests use.  The numbers asserted on the restatement are conditions on those inputs: a changed input cannot quietly empty a test."""
import ctypes as C
import json
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mesh_parts_ref as PR
import mesh_ref as MR
from raymarching_engine_amd import abi, mesh as M, native

ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
ENTRY_POINTS = ("rm_mesh_keep_default", "rm_mesh_components", "rm_mesh_components_download", "rm_mesh_filter")


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) {name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshKeep", "RM_MESH_PART_LABELS") + ENTRY_POINTS)
    assert m.group(1).rstrip().endswith("(additions only)")
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(ENTRY_POINTS) <= exported
    assert (abi.RM_MESH_PART_LABELS, abi.RM_MESH_PART_SIZES) == (0, 1)


def test_defaults_and_struct_layout():
    lib = native.load_library()
    k = abi.RmMeshKeep(min_triangles=7, largest=3, reserved=(C.c_int32 * 2)(5, 6))
    lib.rm_mesh_keep_default(C.byref(k))
    lib.rm_mesh_keep_default(None)  # a no-op
    assert (k.min_triangles, k.largest, k.reserved[0], k.reserved[1]) == (1, 0, 0, 0)
    assert bytes(k) == bytes(M.mesh_keep()) and abi.MESH_KEEP_DEFAULTS == dict(min_triangles=1, largest=0)
    assert C.sizeof(abi.RmMeshKeep) == 16
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct layout from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "k.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\n'
                       'int main(void){ printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(RmMeshKeep), offsetof(RmMeshKeep, min_triangles), offsetof(RmMeshKeep, largest), '
                       'offsetof(RmMeshKeep, reserved), sizeof(RmMeshParams), sizeof(RmMeshSharp), RM_MESH_PART_LABELS, RM_MESH_PART_SIZES); return 0; }\n')
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "k")], check=True)
        out = subprocess.run([str(Path(tmp) / "k")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 0, 4, 8, 24, 16, 0, 1]
    assert [abi.RmMeshKeep.min_triangles.offset, abi.RmMeshKeep.largest.offset, abi.RmMeshKeep.reserved.offset] == [0, 4, 8]


# ---- the refusals made before the handles are looked at --------------------------------------------------------------------------------------

def c_keep(**fields):
    k = abi.RmMeshKeep()
    native.load_library().rm_mesh_keep_default(C.byref(k))
    for name, v in fields.items():
        if name == "reserved":
            k.reserved[0], k.reserved[1] = v
        else:
            setattr(k, name, v)
    return k


BAD_KEEP = [(dict(min_triangles=-1), "min_triangles"), (dict(min_triangles=-(1 << 31)), "min_triangles"), (dict(largest=-1), "largest"), (dict(largest=-7), "largest"),
            (dict(reserved=(1, 0)), "reserved"), (dict(reserved=(0, -1)), "reserved"),
            # the order: min_triangles speaks before largest, largest before reserved
            (dict(min_triangles=-1, largest=-1, reserved=(1, 1)), "min_triangles"), (dict(largest=-1, reserved=(1, 1)), "largest")]


def test_every_refusal_speaks_before_the_handles_and_in_order():
    """No mesh exists without a GPU: every call ends in RM_ERR_INVALID, and the text (rm_last_error(NULL)) tells which check spoke."""
    lib = native.load_library()
    out = C.c_void_p()
    last = lambda: lib.rm_last_error(None).decode()
    inv = abi.RM_ERR_INVALID
    for fields, word in BAD_KEEP:
        for o in (C.byref(out), None):
            assert lib.rm_mesh_filter(None, C.byref(c_keep(**fields)), o) == inv and last().startswith(f"rm_mesh_filter: keep {word}"), (fields, last())
    # a good keep and a NULL keep (the defaults): the NULL handles are what is refused
    for fields in (dict(), dict(min_triangles=0), dict(min_triangles=(1 << 31) - 1), dict(largest=1), dict(largest=(1 << 31) - 1), dict(min_triangles=12, largest=5)):
        assert lib.rm_mesh_filter(None, C.byref(c_keep(**fields)), C.byref(out)) == inv and last() == "rm_mesh_filter: NULL argument", fields
    assert lib.rm_mesh_filter(None, None, C.byref(out)) == inv and last() == "rm_mesh_filter: NULL argument"
    assert lib.rm_mesh_filter(None, None, None) == inv and last() == "rm_mesh_filter: NULL argument"
    count = C.c_ulonglong(77)
    assert lib.rm_mesh_components(None, C.byref(count)) == inv and last() == "rm_mesh_components: NULL argument" and count.value == 77
    assert lib.rm_mesh_components(None, None) == inv and last() == "rm_mesh_components: NULL argument"
    buf = np.zeros(4, np.uint32)
    for what in (abi.RM_MESH_PART_LABELS, abi.RM_MESH_PART_SIZES, -1, 2):
        assert lib.rm_mesh_components_download(None, what, buf.ctypes.data_as(C.c_void_p), 16) == inv and last() == "rm_mesh_components_download: NULL argument"
    # the mesh entries beside them are as they were
    assert lib.rm_mesh_download(None, 0, None, 0) == inv and last() == "rm_mesh_download: NULL mesh"


@pytest.mark.parametrize("bad", [dict(min_triangles=-1), dict(largest=-1), dict(min_triangles=1.0), dict(largest=2.5), dict(min_triangles=True), dict(largest=False),
                                 dict(min_triangles="1"), dict(largest=None), dict(min_triangles=1 << 31), dict(largest=1 << 40), dict(reserved=0), dict(minTriangles=1),
                                 dict(iso=0.0)])
def test_python_refuses_bad_keep_parameters(bad):
    with pytest.raises(ValueError):
        M.mesh_keep(**bad)


def test_python_packs_what_it_is_given():
    k = M.mesh_keep(min_triangles=12, largest=5)
    assert (k.min_triangles, k.largest, k.reserved[0], k.reserved[1]) == (12, 5, 0, 0)
    assert bytes(k) == np.array([12, 5, 0, 0], "<i4").tobytes()
    assert bytes(M.mesh_keep(min_triangles=np.int64(0), largest=np.uint8(3))) == np.array([0, 3, 0, 0], "<i4").tobytes()
    assert bytes(M.mesh_keep(largest=(1 << 31) - 1)) == np.array([1, (1 << 31) - 1, 0, 0], "<i4").tobytes()
    # the host's own conversion of `keep`: True, a dict and a struct say the same thing; anything else is refused
    to_c = native.Context._mesh_keep
    assert bytes(to_c(True)) == bytes(M.mesh_keep()) == bytes(to_c({})) == bytes(to_c(abi.RmMeshKeep(1, 0)))
    assert bytes(to_c(dict(largest=2))) == bytes(to_c(abi.RmMeshKeep(1, 2))) == np.array([1, 2, 0, 0], "<i4").tobytes()
    for bad in (False, 1, "largest", [1, 0], abi.RmMeshKeep(-1, 0), dict(biggest=1)):
        with pytest.raises(ValueError):
            to_c(bad)
    # the mesh of the Python host: the two new fields lie behind `timings` and default to None
    m = M.Mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    assert m.labels is None and m.component_sizes is None
    names = [f for f in M.Mesh.__dataclass_fields__]
    assert names[names.index("timings") + 1:] == ["labels", "component_sizes"]


def test_node_packs_the_keep_block_as_python_does():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    cases = [{}, dict(minTriangles=0), dict(minTriangles=12, largest=5), dict(largest=1), dict(largest=1000000000, minTriangles=1000000000)]
    script = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const out = { size: r.addon.sizes().RmMeshKeep, defaults: r.meshKeep(), same: r.MESH_KEEP_DEFAULTS, none: hex(r.addon.meshKeepBlock(null)), cases: [], bad: [],
              sharp: r.meshSharp(), params: r.meshParams(),
              fns: [typeof r.meshKeep, typeof r.addon.meshKeepBlock, typeof r.RenderJobContext.prototype.extractMesh, typeof r.RenderJobContext.prototype.meshFromValues],
              arity: [r.RenderJobContext.prototype.extractMesh.length, r.RenderJobContext.prototype.meshFromValues.length] };
for (const c of %s) out.cases.push(hex(r.addon.meshKeepBlock(r.meshKeep(c))));
for (const f of [() => r.meshKeep({ minTriangles: -1 }), () => r.meshKeep({ largest: -1 }), () => r.meshKeep({ minTriangles: 1.5 }), () => r.meshKeep({ largest: "1" }),
                 () => r.meshKeep({ largest: true }), () => r.meshKeep({ minTriangles: NaN }), () => r.meshKeep({ largest: Infinity }), () => r.meshKeep({ largest: null }),
                 () => r.meshKeep({ reserved: 0 }), () => r.meshKeep({ min_triangles: 1 }), () => r.meshKeep(3), () => r.meshKeep({ largest: 2 ** 31 })])
  try { f(); out.bad.push(false); } catch (e) { out.bad.push(true); }
console.log(JSON.stringify(out));
""" % (str(JS / "index.js"), json.dumps(cases))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["size"] == 16 and all(out["bad"]) and out["fns"] == ["function"] * 4
    assert out["arity"] == [6, 2]  # (scene, grid, params, sharp, keep, components) and (grid, values, iso = 0, ...): the new ones are appended
    assert out["defaults"] == out["same"] == dict(minTriangles=1, largest=0)
    assert out["sharp"] == dict(refine=6, normalDelta=2.0 ** -10, threshold=0.1)  # meshSharp and meshParams are as they were
    assert out["params"] == dict(iso=0.0, normals=1, normalDelta=1e-5, colours=0, flags=0)
    assert out["none"] == bytes(M.mesh_keep()).hex()
    for c, got in zip(cases, out["cases"]):
        kw = {("min_triangles" if k == "minTriangles" else k): v for k, v in c.items()}
        assert got == bytes(M.mesh_keep(**kw)).hex(), c


# ---- the restatement on the meshes the GPU tests use ---------------------------------------------------------------------------------------

def cached(name, make):
    if name not in cached.store:
        lo, hi, n, values, iso = make()
        pos, tri, cells = MR.surface_nets(lo, hi, n, values, iso)
        labels, sizes = PR.components(len(pos), tri)
        cached.store[name] = dict(positions=pos, triangles=tri, cells=cells, labels=labels, sizes=sizes)
    return cached.store[name]


cached.store = {}
MESHES = {"two balls": lambda: PR.two_balls_field() + (0.0,), "snake": lambda: PR.snake_field() + (0.0,), "noise 1.5": lambda: PR.noise_field() + (1.5,),
          "noise 0.25": lambda: PR.noise_field() + (0.25,)}


def check_partition(m):
    """labels are a partition numbered by smallest vertex index; sizes sum to V and T; no triangle spans two components."""
    labels, sizes, tri = m["labels"], m["sizes"], m["triangles"]
    v, t, c = len(m["positions"]), len(tri), len(sizes)
    assert labels.dtype == np.uint32 and labels.shape == (v,) and sizes.dtype == np.uint32 and sizes.shape == (c, 2)
    assert int(sizes[:, 0].sum()) == v and int(sizes[:, 1].sum()) == t and (sizes[:, 0] >= 1).all()
    assert np.array_equal(np.unique(labels), np.arange(c))
    firsts = np.array([np.flatnonzero(labels == k)[0] for k in range(min(c, 64))])
    assert (np.diff(firsts) > 0).all()  # component index ascends with the smallest vertex index
    if t:
        assert (labels[tri[:, 0]] == labels[tri[:, 1]]).all() and (labels[tri[:, 1]] == labels[tri[:, 2]]).all()
    referenced = np.zeros(v, bool)
    referenced[tri.reshape(-1)] = True
    assert np.array_equal(sizes[labels, 1] == 0, ~referenced)  # a component without triangles is one unreferenced vertex
    assert (sizes[sizes[:, 1] == 0, 0] == 1).all()


def test_restatement_two_balls():
    m = cached("two balls", MESHES["two balls"])
    check_partition(m)
    assert len(m["sizes"]) == 2 and (m["sizes"][:, 1] > 100).all()
    # the same partition from a search that knows nothing of minima: flood from a vertex over the vertex adjacency
    tri = m["triangles"].astype(np.int64)
    reached, frontier = {0}, [0]
    nbr = {}
    for a, b, c in tri:
        for x, y in ((a, b), (b, c), (c, a)):
            nbr.setdefault(x, set()).add(y)
            nbr.setdefault(y, set()).add(x)
    while frontier:
        nxt = [y for x in frontier for y in nbr.get(x, ()) if y not in reached]
        reached.update(nxt)
        frontier = list(set(nxt))
    assert np.array_equal(np.flatnonzero(m["labels"] == 0), np.array(sorted(reached)))


def test_restatement_snake_is_long():
    m = cached("snake", MESHES["snake"])
    check_partition(m)
    assert (len(m["positions"]), len(m["triangles"])) == (1008, 2008)
    assert len(m["sizes"]) == 2 and m["sizes"][:, 0].tolist() == [504, 504]
    least, sweeps = PR.least_index(len(m["positions"]), m["triangles"], jump=False)
    print("snake: plain neighbour-minimum propagation took", sweeps, "sweeps")
    assert sweeps > 64  # more rounds than the device's cap: hooking roots, not passing minima along, is what makes it converge
    jumped, fewer = PR.least_index(len(m["positions"]), m["triangles"])
    assert np.array_equal(least, jumped) and fewer < sweeps


def test_restatement_noise():
    coarse, fine = cached("noise 1.5", MESHES["noise 1.5"]), cached("noise 0.25", MESHES["noise 0.25"])
    for m in (coarse, fine):
        check_partition(m)
    tri = coarse["sizes"][:, 1]
    print("noise 1.5:", len(coarse["positions"]), len(coarse["triangles"]), len(tri), "median", int(np.median(tri)), "largest", sorted(tri.tolist())[-4:][::-1])
    print("noise 0.25:", len(fine["positions"]), len(fine["triangles"]), len(fine["sizes"]))
    assert len(tri) > 1000
    passing = np.sort(tri[tri > 0])
    assert (np.diff(passing) == 0).any()  # at least two components of equal triangle count
    assert (tri == 12).any() and (tri < 12).any() and (tri > 13).any()  # the keep cases at 12 and 13 cut through the population
    assert len(fine["positions"]) > 65536 and len(fine["sizes"]) > 1
    assert (fine["sizes"][:, 1] == 0).any()  # unreferenced boundary vertices: components of one vertex and no triangle


@pytest.mark.parametrize("name", list(MESHES))
def test_keep_rule_and_filtered_arrays(name):
    m = cached(name, MESHES[name])
    sizes, labels = m["sizes"], m["labels"]
    tri_count = sizes[:, 1].astype(np.int64)
    for rule in PR.KEEP_CASES:
        mask = PR.keep_mask(sizes, **rule)
        lo, k = rule.get("min_triangles", 1), rule.get("largest", 0)
        passing = tri_count >= lo
        assert not (mask & ~passing).any()
        if k == 0:
            assert np.array_equal(mask, passing)
        else:
            assert int(mask.sum()) == min(k, int(passing.sum()))
            if mask.any() and (passing & ~mask).any():
                # nothing left out beats anything kept: more triangles, or as many and a lower index
                worst_kept = max((-int(tri_count[c]), c) for c in np.flatnonzero(mask))
                best_left = min((-int(tri_count[c]), c) for c in np.flatnonzero(passing & ~mask))
                assert worst_kept < best_left
        f = PR.filter_arrays(mask, labels, m["positions"], m["triangles"], m["cells"])
        assert f["positions"].dtype == np.float32 and f["triangles"].dtype == np.uint32 and f["cells"].dtype == np.uint32
        assert len(f["positions"]) == int(sizes[mask, 0].sum()) == len(f["cells"]) and len(f["triangles"]) == int(sizes[mask, 1].sum())
        assert f["normals"] is None and f["colours"] is None
        if len(f["triangles"]):
            # a kept triangle's corners are the source's, by position bits
            kept = mask[labels[m["triangles"][:, 0]]]
            assert np.array_equal(f["positions"][f["triangles"]].view(np.uint32), m["positions"][m["triangles"][kept]].view(np.uint32))
        assert (np.diff(f["cells"].astype(np.int64)) > 0).all()  # the original relative order: cells ascend
        # filtering twice equals filtering once
        labels2, sizes2 = PR.components(len(f["positions"]), f["triangles"])
        again = PR.filter_arrays(PR.keep_mask(sizes2, **rule), labels2, f["positions"], f["triangles"], f["cells"])
        for key in ("positions", "triangles", "cells"):
            assert again[key].tobytes() == f[key].tobytes(), (rule, key)
    assert not PR.keep_mask(sizes, min_triangles=1 << 30).any()  # the empty selection
    assert np.array_equal(PR.keep_mask(sizes), tri_count >= 1)  # the defaults drop exactly the unreferenced vertices


def test_largest_across_a_tie_takes_the_lower_index():
    sizes = np.array([[3, 4], [9, 12], [1, 0], [8, 12], [7, 12], [30, 40], [2, 1]], np.uint32)
    assert np.flatnonzero(PR.keep_mask(sizes, largest=1)).tolist() == [5]
    assert np.flatnonzero(PR.keep_mask(sizes, largest=2)).tolist() == [1, 5]
    assert np.flatnonzero(PR.keep_mask(sizes, largest=3)).tolist() == [1, 3, 5]
    assert np.flatnonzero(PR.keep_mask(sizes, largest=5)).tolist() == [0, 1, 3, 4, 5]
    assert np.flatnonzero(PR.keep_mask(sizes, min_triangles=13, largest=5)).tolist() == [5]
    assert np.flatnonzero(PR.keep_mask(sizes, min_triangles=0, largest=7)).tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert np.flatnonzero(PR.keep_mask(sizes, min_triangles=0)).tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert np.flatnonzero(PR.keep_mask(sizes, min_triangles=12)).tolist() == [1, 3, 4, 5]
    assert not PR.keep_mask(np.zeros((0, 2), np.uint32), largest=3).any()
