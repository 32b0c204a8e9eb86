"""Both hosts run every stage of the mesh pipeline at once on the GPU: the Node host's longest argument lists (thirteen, and fourteen in slabs)
against Context.extract_mesh.  Every array is compared byte for byte, every report field by field (milliseconds apart), and the Node result's
keys in their order.  A block handed to the wrong stage, or a stage left out, cannot pass."""
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_deviation_ref as DR
import mesh_measure_ref as QR
import mesh_project_ref as PR
from raymarching_engine_amd import mesh as M, native, scene as S

pytestmark = pytest.mark.gpu
JS = Path(__file__).resolve().parents[1] / "raymarching-engine_amd" / "js"
# a sphere and a box apart: two components, and hard edges
LO, HI, N, CLUSTERS = (-1.0, -1.0, -1.0), (1.6, 1.0, 1.0), (20, 16, 16), (10, 8, 8)
SPHERE, BOX = ((0.0, 0.0, 0.0), 0.6), ((1.2, 0.0, 0.0), (0.25, 0.25, 0.25))
KEYS = ["positions", "normals", "colours", "triangles", "cells", "labels", "componentSizes", "projection", "residual", "occlusion", "deviation",
        "triangleDeviation", "timings", "measures"]
ARRAYS = dict(positions="positions", normals="normals", triangles="triangles", cells="cells", labels="labels", componentSizes="component_sizes", residual="residual",
              occlusion="occlusion", triangleDeviation="triangle_deviation")


def snake(report: dict) -> dict:
    return {re.sub(r"[A-Z]", lambda m: "_" + m.group(0).lower(), k): v for k, v in report.items()}


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def node(tmp_path_factory):
    """the Node host's two results: without slabs, and in slabs of five layers"""
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    d = tmp_path_factory.mktemp("hosts")
    script = f"""
const r = require({str(JS / "index.js")!r}), fs = require("fs"), d = {str(d)!r};
const ctx = new r.RenderJobContext(0), sc = new r.CsgScene().sphere({list(SPHERE[0])}, {SPHERE[1]}).union().box({list(BOX[0])}, {list(BOX[1])});
const g = r.meshGrid({list(LO)}, {list(HI)}, {list(N)}), clusters = r.meshGrid({list(LO)}, {list(HI)}, {list(CLUSTERS)});
const flat = (k, v) => v instanceof BigUint64Array ? Array.from(v, String) : ArrayBuffer.isView(v) ? undefined : v;
for (const [name, slabs] of [["whole", null], ["slabbed", 5]]) {{
  const m = ctx.extractMesh(sc, g, null, true, {{ largest: 1 }}, true, {{ grid: clusters }}, true, {{ directions: 4, taps: 2 }}, true, slabs, true, {{ order: 2 }});
  for (const k of {json.dumps(list(ARRAYS))}) fs.writeFileSync(d + "/" + name + "_" + k, Buffer.from(m[k].buffer, m[k].byteOffset, m[k].byteLength));
  fs.writeFileSync(d + "/" + name + ".json", JSON.stringify({{ keys: Object.keys(m), colours: m.colours, report: m }}, flat));
}}
ctx.close();
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return d


@pytest.mark.parametrize("name, slabs", [("whole", None), ("slabbed", 5)])
def test_every_stage_at_once_gives_both_hosts_the_same_mesh(ctx, node, name, slabs):
    scene = ctx.create_scene(S.CsgScene().sphere(*SPHERE).union().box(*BOX))
    try:
        want = ctx.extract_mesh(scene, M.Grid(LO, HI, N), sharp=True, simplify=M.Grid(LO, HI, CLUSTERS), quadric=True, keep=dict(largest=1), components=True, project=True,
                                occlusion=dict(directions=4, taps=2), measures=True, deviation=dict(order=2), slabs=slabs)
    finally:
        scene.destroy()
    got = json.loads((node / (name + ".json")).read_text())
    assert got["keys"] == KEYS and got["colours"] is None and want.colours is None
    assert want.vertices > 0 and len(want.triangles) > 0 and len(want.component_sizes) == 1  # (the sphere: the box was filtered out)
    for js, py in ARRAYS.items():
        assert (node / (name + "_" + js)).read_bytes() == getattr(want, py).tobytes(), js
    report = got["report"]
    assert len(report["timings"]) == 4 and set(want.timings) == {"sampling", "meshing", "attributes", "projection", "occlusion", "deviation", "measures"}
    for mine, theirs, fields, same in ((report["projection"], want.projection, PR.FIELDS, PR.same), (report["deviation"], want.deviation, DR.FIELDS, DR.same)):
        assert set(snake(mine)) == set(fields) | {"milliseconds"} and same(snake(mine), theirs) == [], (mine, theirs)  # (a JSON number gives every double and float back)
    measures = snake(report["measures"])
    edges = np.array([int(x) for x in measures["component_edges"]], np.uint64).reshape(-1, 4)
    assert edges.tobytes() == want.measures["component_edges"].tobytes() and len(measures.pop("milliseconds")) == 2
    assert set(measures) == set(want.measures) and QR.same(measures, want.measures) == [], (measures, want.measures)
    assert want.measures["vertices"] == want.vertices and want.projection["vertices"] == want.vertices and want.deviation["triangles"] == len(want.triangles)
