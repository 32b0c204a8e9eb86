"""The half-precision G-buffer (RM_GBUFFER_F16, ABI 9) without a GPU: the C ABI, the code object, the accumulation rule
on the CPU oracle's samples, and the hosts' validation.

LoadRenderJobContext.tsx:81-119 allocates normal + DoF radius and albedo + depth as RGBA16F; raymarcher.frag:347-351
adds a sample's contribution to what the attachment holds, so on a hardware GL every sample's sum is rounded to half:
    h = (h.astype(np.float32) + v).astype(np.float16)      (per sample, per component)
fold_half below is that rule; the GPU tests hold the kernels to it bit for bit (test_gpu_gbuffer_half.py)."""
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import golden_cases as GC
from oracle import oracle as O
from raymarching_engine_amd import abi, job as J, native, scene as S

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/llvm/bin")
NEW_ENTRY_POINTS = ("rm_fb_create_fmt", "rm_fb_create_striped_fmt", "rm_fb_wrap_fmt", "rm_fb_gbuffer", "rm_fb_download_raw", "rm_fb_upload_raw")


def fold_half(planes):
    """The RGBA16F accumulation of per-sample fp32 contributions `planes` (each [rows, W, 4]): the stored half sum after each."""
    h = np.zeros(planes[0].shape, np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        for v in planes:
            h = (h.astype(np.float32) + v).astype(np.float16)
    return h


def test_abi_version_and_entry_points():
    lib = native.load_library()
    assert abi.RM_ABI_VERSION == 9 == lib.rm_abi_version()
    assert (abi.RM_GBUFFER_F32, abi.RM_GBUFFER_F16) == (0, 1)
    for name in NEW_ENTRY_POINTS:
        assert name in native.EXPORTS
        assert hasattr(lib, name)
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    assert re.search(r"#define RM_ABI_VERSION 9 /\* 9: ", header)
    assert "RM_GBUFFER_F32 = 0, RM_GBUFFER_F16 = 1" in header
    for name in NEW_ENTRY_POINTS:
        assert f"RM_API int {name}(" in header


def _code_objects(lib_path: Path):
    """The gfx950 code objects of the library's offload bundles (.hip_fatbin: __CLANG_OFFLOAD_BUNDLE__ headers, each listing
    (offset, size, triple) entries relative to the bundle)."""
    objcopy = LLVM / "llvm-objcopy"
    blob = subprocess.run([str(objcopy), "--dump-section", ".hip_fatbin=/dev/stdout", str(lib_path), "/dev/null"], capture_output=True, check=True).stdout
    magic, out, i = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (i := blob.find(magic, i)) >= 0:
        (n,) = struct.unpack_from("<Q", blob, i + 24)
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(blob[i + off:i + off + size])
        i += len(magic)
    return out


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists() or not (LLVM / "llvm-objcopy").exists(), reason="ROCm's llvm-objdump is missing")
def test_code_object_rounds_to_nearest_even_and_keeps_half_denormals(tmp_path):
    """No kernel narrows with v_cvt_pkrtz_f16_f32 (round toward zero: wrong for RGBA16F), the half G-buffer's kernels do narrow
    (v_cvt_pk_f16_f32 / v_cvt_f16_f32, which round by the MODE register: to nearest even), and every kernel descriptor keeps
    f16 / f64 denormals (float_denorm_mode_16_64 = 3: flushing would change small normal components)."""
    objs = _code_objects(native.LIB_PATH)
    assert objs, "no gfx950 code object in the library"
    kernels = narrowing = 0
    for k, co in enumerate(objs):
        path = tmp_path / f"co{k}.o"
        path.write_bytes(co)
        dis = subprocess.run([str(LLVM / "llvm-objdump"), "-D", str(path)], capture_output=True, text=True, check=True).stdout
        assert "v_cvt_pkrtz_f16_f32" not in dis
        n = len(re.findall(r"^\s*\.amdhsa_kernel ", dis, re.M))
        assert n == len(re.findall(r"^\s*\.amdhsa_float_denorm_mode_16_64 3\s*$", dis, re.M))
        kernels += n
        narrowing += len(re.findall(r"\bv_cvt_(?:pk_)?f16_f32", dis))
    assert kernels > 0 and narrowing > 0


def _dof_scene_samples(n, width=32, height=32, seed_pairs=None):
    """n single samples (each into a fresh oracle.Frame) of a small strict scene with depth of field and sky: a sphere on a floor
    (the plane y = -1, whose normal is +y exactly)."""
    sc = S.CsgScene().sphere((0.0, 0.0, 0.0), 1.0).union().plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0))
    schema = J.make_schema(sc, width, height, counts=(16,), render_mode="full", position=(0.0, 0.0, -3.0), lights=GC.LIGHT,
                           dof_amount=0.1, dof_distance=2.0)
    pairs = seed_pairs if seed_pairs is not None else GC.halton_pairs(n)
    frames = []
    for p in pairs[:n]:
        f = O.Frame(width, height)
        O.render(sc, J.uniforms_from_schema(schema, p), f)
        frames.append(f)
    return frames


def test_fold_rule_on_the_oracle_saturates_overflows_and_shows():
    """The rule folded over the oracle's per-sample planes: the summed normal of a pixel stops at 2048 (2048 + 1 rounds back to
    2048 in half) while the fp32 sum keeps growing; and a sky pixel's summed depth (clamped to 1e8, raymarcher.frag:337) overflows
    half's 65504 to +inf."""
    J.reset_halton()
    n = 2100
    frames = _dof_scene_samples(n, 16, 16)
    nd = [f.normal_dof for f in frames]
    ad = [f.albedo_depth for f in frames]
    hn, ha = fold_half(nd), fold_half(ad)
    f32n = np.sum(np.stack(nd).astype(np.float64), axis=0)
    # saturation: a pixel whose normal.y is in (0, 1] in every sample (the sum passes 2048) sits at 2048 in half
    ny = np.stack(nd)[..., 1]
    sat = np.all((ny > 0.0) & (ny <= 1.0), axis=0) & (f32n[..., 1] > 2050.0)
    assert sat.any(), "the scene has no pixel whose normal.y sum passes 2048"
    assert np.all(hn[..., 1][sat] == np.float16(2048.0))
    # the fp32 planes keep counting: their sum is past 2048 where the half one stopped
    acc = np.zeros_like(nd[0])
    for v in nd:
        acc = acc + v
    assert np.all(acc[..., 1][sat] > 2050.0)
    # sky: the depth of an escaped ray (clamped to 1e8) summed past half's 65504 is +inf, where fp32 holds a finite sum
    depth = np.stack(ad)[..., 3]
    sky = np.all(np.stack(nd)[..., 1] == 0.0, axis=0) & np.all(np.isfinite(depth), axis=0) & (np.sum(depth.astype(np.float64), axis=0) > 65520.0)
    assert sky.any()
    assert np.all(np.isposinf(ha[..., 3][sky]))
    assert np.all(np.isfinite(acc[..., 1]))
    d32 = np.zeros_like(ad[0])
    for v in ad:
        d32 = d32 + v
    assert np.all(np.isfinite(d32[..., 3][sky]))


def test_fold_rule_changes_the_present_of_a_dof_frame():
    """oracle.present of the widened half planes against the fp32 ones of the same 64 samples of a DoF scene: some pixel differs
    (the format is observable in the canvas), and the colour plane is the same in both."""
    J.reset_halton()
    n = 64
    frames = _dof_scene_samples(n)
    color = np.zeros_like(frames[0].color)
    nd32 = np.zeros_like(frames[0].normal_dof)
    for f in frames:  # additive blend: colour and the fp32 G-buffer are plain sums
        color = color + f.color
        nd32 = nd32 + f.normal_dof
    nd16 = fold_half([f.normal_dof for f in frames]).astype(np.float32)
    assert (nd32[..., 3] > 0).any() and (nd16[..., 3] > 0).any()  # the blur is on
    assert not np.array_equal(nd16, nd32)
    a, b = O.present(color, nd32, n), O.present(color, nd16, n)
    assert (a != b).any(), "the half DoF radius changes no byte of the canvas"


def test_hosts_refuse_an_unknown_format_before_device_work():
    with pytest.raises(ValueError):
        J.RenderJobContext(gbuffer="f64", native_context=object())
    with pytest.raises(ValueError):
        native.gbuffer_code("half")
    assert native.gbuffer_code("f32") == abi.RM_GBUFFER_F32 and native.gbuffer_code("f16") == abi.RM_GBUFFER_F16
    assert J.RenderJobContext(native_context=object()).gbuffer == "f32"


def test_job_context_asks_for_its_format():
    """Every framebuffer a context with gbuffer="f16" makes -- whole frame, row window, stripes -- is asked of the native context in
    that format; the default context asks as it always has (no argument: stand-in contexts predate it)."""
    calls = []

    class FakeFb:
        row_count = 8
        def clear(self): pass
        def destroy(self): pass

    class FakeNative:
        def create_framebuffer(self, *a, **kw):
            calls.append(("plain", a, kw))
            return FakeFb()
        def create_striped_framebuffer(self, *a, **kw):
            calls.append(("striped", a, kw))
            return FakeFb()

    for fmt in ("f32", "f16"):
        del calls[:]
        J.RenderJobContext(native_context=FakeNative(), gbuffer=fmt).fbo_create(16, 8, 0)
        J.RenderJobContext(native_context=FakeNative(), gbuffer=fmt, rows=(0, 4)).fbo_create(16, 8, 0)
        J.RenderJobContext(native_context=FakeNative(), gbuffer=fmt, stripes=(3, 1)).fbo_create(16, 8, 0)
        assert [c[0] for c in calls] == ["plain", "plain", "striped"]
        assert all(c[2] == ({} if fmt == "f32" else {"gbuffer": "f16"}) for c in calls)


@pytest.mark.skipif(shutil.which("node") is None or not (ROOT / "raymarching-engine_amd" / "js" / "rm_napi.node").exists(), reason="node or the addon is missing")
def test_js_contexts_pass_the_format_to_the_addon():
    """new RenderJobContext({ gbuffer: "f16" }) / ShardedRenderJobContext({ gbuffer: "f16" }) create their framebuffers with
    RM_GBUFFER_F16 (the addon's calls recorded); an unknown format is a RangeError before any device work."""
    js = ROOT / "raymarching-engine_amd" / "js" / "index.js"
    script = f"""
const rm = require({str(js)!r});
const a = rm.addon, got = [];
a.ctxCreate = () => ({{}}); a.setSamplesInFlight = () => {{}};
a.fbCreate = (...args) => {{ got.push(["fbCreate", args.slice(1)]); return {{}}; }};
a.fbCreateStriped = (...args) => {{ got.push(["fbCreateStriped", args.slice(1)]); return {{}}; }};
new rm.RenderJobContext().fboCreate(16, 8, 0);
new rm.RenderJobContext({{ gbuffer: "f16" }}).fboCreate(16, 8, 0);
new rm.RenderJobContext(0, rm.RM.RENDER_FAST).fboCreate(16, 8, 0);
new rm.ShardedRenderJobContext({{ devices: [0, 0], gbuffer: "f16" }}).fboCreate(16, 8, 0);
let bad = "";
try {{ new rm.RenderJobContext({{ gbuffer: "f64" }}); }} catch (e) {{ bad = e.name; }}
process.stdout.write(JSON.stringify({{ got, bad, fast: new rm.RenderJobContext(0, rm.RM.RENDER_FAST).flags }}));
"""
    import json

    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["bad"] == "RangeError" and out["fast"] == abi.RM_RENDER_FAST
    assert out["got"] == [["fbCreate", [16, 8, 0, 8, 0]], ["fbCreate", [16, 8, 0, 8, 1]], ["fbCreate", [16, 8, 0, 8, 0]],
                          ["fbCreateStriped", [16, 8, 8, 2, 0, 1]], ["fbCreateStriped", [16, 8, 8, 2, 1, 1]]]
