// index.js -- JavaScript host of the render-job API on top of the N-API addon.
//
// Mirrors client/src/renderer/RenderJobExecutor.tsx:77-341 of the reference:
// `doRenderJob(schema, context)` resolves to a generator factory; the generator
// yields every `sampleYieldInterval` samples after calling `present`, and
// returns {success:true} or {success:false, why} -- errors are values.  The
// gl.* block of the reference (:181-326) is one native call per sample.
// The RenderJobSchema is the reference's (RenderJobSchema.tsx:17-86) plus
// `sdfScene`, a scene built with the composition API below (a HIP kernel
// cannot consume GLSL text; the composer emits both back ends).
// Types: index.d.ts.  (The container has Node 12 / N-API 8 and no tsc, so the
// host is JavaScript with hand-written typings.)
"use strict";
// Process environment the device path depends on (read by the HIP / HSA runtime when it starts, i.e. when the addon
// first touches the GPU): dmabuf IPC.  Set unless the user has set it (native.py does the same).
if (process.env.HSA_ENABLE_IPC_MODE_LEGACY === undefined) process.env.HSA_ENABLE_IPC_MODE_LEGACY = "0";
const addon = require("./rm_napi.node");

const RM = {
  MAX_BOUNCES: 10, MAX_LIGHTS: 10,
  SCENE_TABLE: 0, SCENE_MANDELBULB: 1, SCENE_SPHERE_GRID: 2, SCENE_SPHERE_LATTICE: 3, SCENE_MENGER: 4, SCENE_KIFS_TREE: 5, SCENE_KIFS_BOX: 6,
  PRIM_SPHERE: 0, PRIM_BOX: 1, PRIM_REPEAT: 2, PRIM_FOLD: 3, PRIM_KIND: 4, PRIM_TORUS: 5, PRIM_CYLINDER: 6, PRIM_PLANE: 7,
  OP_UNION: 0, OP_SMOOTH_UNION: 1, OP_SUBTRACT: 2, OP_INTERSECT: 3, OP_SMOOTH_SUBTRACT: 4, OP_SMOOTH_INTERSECT: 5,
  RENDER_STRICT: 0, RENDER_FAST: 1, RENDER_COLOR_ONLY: 2, RENDER_MEGAKERNEL: 4, RENDER_WAVEFRONT: 16, RENDER_NO_OVERLAP: 32, RENDER_NO_FAR_JUMP: 64, RENDER_NO_CULL: 128,
  GBUFFER_F32: 0, GBUFFER_F16: 1, FB_MOMENTS: 0x100, PLANE_MOMENTS: 3, DENOISE_NONE: 0, DENOISE_ATROUS: 1, DENOISE_VARIANCE: 2,
};
// G-buffer formats of a context's framebuffers (include/hip_raymarch.h RM_GBUFFER_*): "f32", the default (the goldens' software GL
// stack), or "f16", the reference's RGBA16F normal + DoF radius and albedo + depth planes (LoadRenderJobContext.tsx:81-119)
const GBUFFER = { f32: RM.GBUFFER_F32, f16: RM.GBUFFER_F16 };
function gbufferCode(name) {
  if (!Object.prototype.hasOwnProperty.call(GBUFFER, name)) throw new RangeError(`gbuffer must be "f32" or "f16", not ${JSON.stringify(name)}`);
  return GBUFFER[name];
}

// ---- struct layouts (include/hip_raymarch.h; all fields are 4 bytes) ----------------
const U_FIELDS = [
  ["blendWithPreviousFactor", 1, "f"], ["randNoise", 2, "f"], ["position", 3, "f"], ["rotation", 16, "f"], ["dofAmount", 1, "f"],
  ["dofFocalPlaneDistance", 1, "f"], ["cameraMode", 1, "i"], ["fov", 1, "f"], ["reflections", 1, "f"], ["raymarchingSteps", 1, "f"],
  ["indirectLightingRaymarchingSteps", 1, "f"], ["aspect", 1, "f"], ["fogDensity", 1, "f"], ["exposure", 1, "f"],
  ["raymarchingStepCountsArray", 10, "f"], ["blendMode", 1, "i"], ["renderMode", 1, "i"], ["lightPositions", 30, "f"],
  ["lightColors", 30, "f"], ["lightSizes", 10, "f"], ["lightCount", 1, "i"], ["showDofFocalPlane", 1, "i"],
];
const U_OFFSET = {};
let uSize = 0;
for (const [name, n] of U_FIELDS) { U_OFFSET[name] = uSize; uSize += 4 * n; }
if (uSize !== addon.sizes().RmUniforms) throw new Error("RmUniforms layout mismatch: " + uSize + " != " + addon.sizes().RmUniforms);

function packUniforms(values) {
  const buf = new ArrayBuffer(uSize);
  const f = new Float32Array(buf), i = new Int32Array(buf);
  for (const [name, n, t] of U_FIELDS) {
    const v = values[name];
    if (v === undefined) continue;
    const at = U_OFFSET[name] / 4, arr = n === 1 && !Array.isArray(v) ? [v] : v;
    for (let k = 0; k < arr.length && k < n; k++) (t === "f" ? f : i)[at + k] = arr[k];
  }
  return buf;
}

// ---- scene composition --------------------------------------------------------------
const DEFAULT_MATERIAL = {  // Validate.tsx:18-51
  diffuse: [0.6, 0.6, 0.6], diffuse_cutoff: 35, specular: [0.6, 0.6, 0.6], specular_cutoff: 35, roughness: 0.2, subsurface: 11111115,
  subsurface_color: [1, 1, 1], ior: 100, sky_color: [0.7, 0.8, 1.0], sky_floor: 0.2, sky_scale: 2, sky_radius: 36, sky_axis: 1,
};
const glf = (x) => { const s = String(Math.fround(x)); return /[.e]/.test(s) ? s : s + ".0"; };
const glv = (v) => `vec3(${glf(v[0])}, ${glf(v[1])}, ${glf(v[2])})`;

class Scene {
  constructor(kind, params, material) { this.kind = kind; this.params = params || []; this.material = Object.assign({}, DEFAULT_MATERIAL, material || {}); this.prims = []; this.surfaces = []; }
  // RmSceneDesc bytes: kind, nprims, prims pointer (8, filled natively), params[16], material (22 x 4), nsurfaces, reserved, surfaces pointer (8, filled natively)
  desc() {
    const buf = new ArrayBuffer(addon.sizes().RmSceneDesc);
    const f = new Float32Array(buf), i = new Int32Array(buf);
    i[0] = this.kind; i[1] = this.prims.length;
    for (let k = 0; k < this.params.length; k++) f[4 + k] = this.params[k];
    const m = this.material, at = 20;
    f.set([...m.diffuse, m.diffuse_cutoff, ...m.specular, m.specular_cutoff, m.roughness, m.subsurface, ...m.subsurface_color, m.ior,
           ...m.sky_color, m.sky_floor, m.sky_scale, m.sky_radius], at);
    i[at + 20] = m.sky_axis;
    i[at + 22] = this.surfaces.length;
    let prims = null;
    if (this.prims.length) {
      prims = new ArrayBuffer(32 * this.prims.length);
      const pf = new Float32Array(prims), pi = new Int32Array(prims);
      this.prims.forEach((p, n) => { pi[8 * n] = p.prim | (p.op << 8) | ((p.surface || 0) << 16); pf[8 * n + 1] = p.k; pf.set(p.center, 8 * n + 2); pf.set(p.size, 8 * n + 5); });
    }
    let surfaces = null;
    if (this.surfaces.length) {  // RmSurface rows: diffuse[3], roughness, specular[3], subsurface, subsurface_color[3], ior
      surfaces = new ArrayBuffer(48 * this.surfaces.length);
      const sf = new Float32Array(surfaces);
      this.surfaces.forEach((u, n) => sf.set([...u.diffuse, u.roughness, ...u.specular, u.subsurface, ...u.subsurface_color, u.ior], 12 * n));
    }
    return { desc: buf, prims, surfaces };
  }
  key() { const d = this.desc(); return Buffer.from(d.desc).toString("hex") + (d.prims ? Buffer.from(d.prims).toString("hex") : "") + (d.surfaces ? Buffer.from(d.surfaces).toString("hex") : ""); }
}

class CsgScene extends Scene {
  constructor(material) { super(RM.SCENE_TABLE, [], material); this._op = RM.OP_UNION; this._k = 0; }
  union() { this._op = RM.OP_UNION; this._k = 0; return this; }
  smoothUnion(k) { this._op = RM.OP_SMOOTH_UNION; this._k = k; return this; }
  subtract() { this._op = RM.OP_SUBTRACT; this._k = 0; return this; }
  intersect() { this._op = RM.OP_INTERSECT; this._k = 0; return this; }
  // ABI 8: the smooth forms of the other two operators (h = clamp(0.5 - 0.5 (d +- di) / k, 0, 1); mix(d, -+di, h) + k h (1 - h)) ...
  smoothSubtract(k) { this._op = RM.OP_SMOOTH_SUBTRACT; this._k = k; return this; }
  smoothIntersect(k) { this._op = RM.OP_SMOOTH_INTERSECT; this._k = k; return this; }
  // `surface` (optional): material values of this shape's own -- {diffuse, specular, roughness, subsurface, subsurface_color, ior}, missing
  // ones from the reference defaults (Validate.tsx:18-51); the material functions then depend on the position (materialGlsl)
  _surface(surface) {
    if (!surface) return 0;
    const u = { diffuse: [0.6, 0.6, 0.6], specular: [0.6, 0.6, 0.6], roughness: 0.2, subsurface: 11111115, subsurface_color: [1, 1, 1], ior: 100, ...surface };
    const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
    let k = this.surfaces.findIndex((v) => same(v, u));
    if (k < 0) { if (this.surfaces.length >= 15) throw new RangeError("a scene has at most 15 surfaces"); this.surfaces.push(u); k = this.surfaces.length - 1; }
    return k + 1;
  }
  sphere(center, radius, surface) { this.prims.push({ prim: RM.PRIM_SPHERE, op: this._op, k: this._k, center, size: [radius, 0, 0], surface: this._surface(surface) }); return this; }
  box(center, half, surface) { this.prims.push({ prim: RM.PRIM_BOX, op: this._op, k: this._k, center, size: half, surface: this._surface(surface) }); return this; }
  // ... and three more shapes about `center`, axis y: a ring, a capped cylinder, a half space (unit normal); their GLSL text is the
  // Python composer's (scene.py CsgScene: rmTorus, rmCylinder, rmPlane): glsl() here throws
  torus(center, majorRadius, minorRadius, surface) { this.prims.push({ prim: RM.PRIM_TORUS, op: this._op, k: this._k, center, size: [majorRadius, minorRadius, 0], surface: this._surface(surface) }); return this; }
  cylinder(center, radius, halfHeight, surface) { this.prims.push({ prim: RM.PRIM_CYLINDER, op: this._op, k: this._k, center, size: [radius, halfHeight, 0], surface: this._surface(surface) }); return this; }
  plane(point, normal, surface) { this.prims.push({ prim: RM.PRIM_PLANE, op: this._op, k: this._k, center: point, size: normal, surface: this._surface(surface) }); return this; }
  // a shape whose distance term is another scene kind's own estimator at p - center (RM_PRIM_KIND, include/hip_raymarch.h): a Mandelbulb
  // (or a kind 3 lattice), folded like a sphere or a box -- new CsgScene().shape(new Mandelbulb()).intersect().box(...) is a Mandelbulb cut
  // by a box.  One kind with one parameter set per table (they travel in the scene's parameter block).  The GLSL text of such a table
  // is the Python composer's (scene.py CsgScene.shape); glsl() here throws.
  shape(scene, center = [0, 0, 0], surface) {
    if (scene.kind !== RM.SCENE_MANDELBULB && scene.kind !== 3) throw new TypeError("shape(): the kinds a table row can evaluate are the Mandelbulb and the sphere lattice");
    if (this._kind !== undefined && (this._kind !== scene.kind || JSON.stringify(this.params) !== JSON.stringify(scene.params))) throw new TypeError("shape(): a table evaluates ONE kind with one set of parameters");
    this._kind = scene.kind; this.params = scene.params.slice();
    this.prims.push({ prim: RM.PRIM_KIND, op: this._op, k: this._k, center, size: [scene.kind, 0, 0], surface: this._surface(surface) });
    return this;
  }
  // domain operators (include/hip_raymarch.h): they transform the point the FOLLOWING primitives are evaluated at
  repeat(period) { this.prims.push({ prim: RM.PRIM_REPEAT, op: 0, k: 0, center: [0, 0, 0], size: period }); return this; }
  fold(scale, offset, angles = [0, 0, 0]) { this.prims.push({ prim: RM.PRIM_FOLD, op: 0, k: scale, center: offset, size: angles }); return this; }
  glsl() {  // the reference's scene contract: float sdf(vec3); helpers sdfSphere/sdBox come from raymarcher.frag:74,108
    const lines = [];
    if (this.prims.some((n) => n.prim === RM.PRIM_KIND)) throw new Error("glsl(): a table with kind rows gets its text from the Python composer (scene.py CsgScene.shape)");
    if (this.prims.some((n) => n.prim > RM.PRIM_KIND || n.op > RM.OP_INTERSECT)) throw new Error("glsl(): a table with ABI 8's shapes or smooth operators gets its text from the Python composer (scene.py CsgScene)");
    const isShape = (n) => n.prim === RM.PRIM_SPHERE || n.prim === RM.PRIM_BOX;
    const shapes = this.prims.filter(isShape), domain = shapes.length !== this.prims.length;
    if (shapes.slice(1).some((p) => p.op === RM.OP_SMOOTH_UNION))
      lines.push("float rmSmoothUnion(float d1, float d2, float k) { float h = clamp(0.5 + 0.5 * (d2 - d1) / k, 0.0, 1.0); return mix(d2, d1, h) - k * h * (1.0 - h); }");
    if (this.prims.some((n) => n.prim === RM.PRIM_FOLD))
      lines.push("vec3 rmFold(vec3 q, float scale, vec3 off, vec3 ang) { q = q / scale; q = abs(q) - off; float c; float s; float nx; float ny;" +
        " c = cos(ang.x); s = sin(ang.x); nx = q.x * c + q.y * -s; ny = q.x * s + q.y * c; q.x = nx; q.y = ny;" +
        " c = cos(ang.y); s = sin(ang.y); nx = q.y * c + q.z * -s; ny = q.y * s + q.z * c; q.y = nx; q.z = ny;" +
        " c = cos(ang.z); s = sin(ang.z); nx = q.x * c + q.z * -s; ny = q.x * s + q.z * c; q.x = nx; q.z = ny; return q; }");
    lines.push("float sdf(vec3 p) {");
    const q = domain ? "q" : "p";
    if (domain) lines.push("  vec3 q = p; float factor = 1.0; float d;");
    let first = true;
    this.prims.forEach((n) => {
      if (n.prim === RM.PRIM_REPEAT) { lines.push(`  q = mod(q + 0.5 * ${glv(n.size)}, ${glv(n.size)}) - 0.5 * ${glv(n.size)};`); return; }
      if (n.prim === RM.PRIM_FOLD) { lines.push(`  q = rmFold(q, ${glf(n.k)}, ${glv(n.center)}, ${glv(n.size)}); factor = factor * ${glf(n.k)};`); return; }
      let e = n.prim === RM.PRIM_SPHERE ? `sdfSphere(${q}, ${glv(n.center)}, ${glf(n.size[0])})` : `sdBox(${q} - ${glv(n.center)}, ${glv(n.size)})`;
      if (domain) e = `(${e} * factor)`;
      if (first) { lines.push(domain ? `  d = ${e};` : `  float d = ${e};`); first = false; }
      else if (n.op === RM.OP_UNION) lines.push(`  d = min(d, ${e});`);
      else if (n.op === RM.OP_SMOOTH_UNION) lines.push(`  d = rmSmoothUnion(d, ${e}, ${glf(n.k)});`);
      else if (n.op === RM.OP_SUBTRACT) lines.push(`  d = max(d, -${e});`);
      else lines.push(`  d = max(d, ${e});`);
    });
    lines.push("  return d;", "}");
    if (this.prims.some((n) => n.surface)) lines.push(this.materialGlsl());
    return lines.join("\n");
  }
  // The seven material functions of a scene whose shapes name surfaces (scene.py material_glsl, statement for statement): at
  // `position` the values of the shape row whose distance term there is the smallest (the earliest on a tie; a NaN never wins).
  materialGlsl() {
    const isShape = (n) => n.prim === RM.PRIM_SPHERE || n.prim === RM.PRIM_BOX;
    const domain = this.prims.filter(isShape).length !== this.prims.length, q = domain ? "q" : "p", m = this.material;
    const all = [{ diffuse: m.diffuse, specular: m.specular, roughness: m.roughness, subsurface: m.subsurface, subsurface_color: m.subsurface_color, ior: m.ior }, ...this.surfaces];
    const n = all.length, lines = ["int rmSurfaceIndex(vec3 p) {"];
    if (domain) lines.push("  vec3 q = p; float factor = 1.0;");
    lines.push("  float best = 0.0; float di; int surface = 0;");
    let first = true;
    this.prims.forEach((node) => {
      if (node.prim === RM.PRIM_REPEAT) { lines.push(`  q = mod(q + 0.5 * ${glv(node.size)}, ${glv(node.size)}) - 0.5 * ${glv(node.size)};`); return; }
      if (node.prim === RM.PRIM_FOLD) { lines.push(`  q = rmFold(q, ${glf(node.k)}, ${glv(node.center)}, ${glv(node.size)}); factor = factor * ${glf(node.k)};`); return; }
      let e = node.prim === RM.PRIM_SPHERE ? `sdfSphere(${q}, ${glv(node.center)}, ${glf(node.size[0])})` : `sdBox(${q} - ${glv(node.center)}, ${glv(node.size)})`;
      if (domain) e = `(${e} * factor)`;
      if (first) { lines.push(`  best = ${e}; surface = ${node.surface || 0};`); first = false; }
      else lines.push(`  di = ${e}; if (di < best) { best = di; surface = ${node.surface || 0}; }`);
    });
    lines.push("  return surface;", "}");
    const table = (name, typ, vals) => `const ${typ} ${name}[${n}] = ${typ}[${n}](${vals.join(", ")});`;
    lines.push(table("rmDiffuse", "vec3", all.map((u) => glv(u.diffuse))), table("rmSpecular", "vec3", all.map((u) => glv(u.specular))),
      table("rmSubsurfaceColor", "vec3", all.map((u) => glv(u.subsurface_color))), table("rmRoughness", "float", all.map((u) => glf(u.roughness))),
      table("rmSubsurface", "float", all.map((u) => glf(u.subsurface))), table("rmIor", "float", all.map((u) => glf(u.ior))),
      `vec3 sceneDiffuseColor(vec3 position) { if (length(position) > ${glf(m.diffuse_cutoff)}) return vec3(0.0); return rmDiffuse[rmSurfaceIndex(position)]; }`,
      `vec3 sceneSpecularColor(vec3 position) { if (length(position) > ${glf(m.specular_cutoff)}) return vec3(0.0); return rmSpecular[rmSurfaceIndex(position)]; }`,
      "float sceneSpecularRoughness(vec3 position) { return rmRoughness[rmSurfaceIndex(position)]; }",
      "float sceneSubsurfaceScattering(vec3 position) { return rmSubsurface[rmSurfaceIndex(position)]; }",
      "vec3 sceneSubsurfaceScatteringColor(vec3 position) { return rmSubsurfaceColor[rmSurfaceIndex(position)]; }",
      "float sceneIOR(vec3 position) { return rmIor[rmSurfaceIndex(position)]; }",
      `vec3 sceneEmission(vec3 position) { float d = max(normalize(position).${"xyz"[m.sky_axis]}, ${glf(m.sky_floor)}); vec3 brightColor = ${glv(m.sky_color)} * d * 1.0;` +
      ` return (length(position) > ${glf(m.sky_radius)}) ? (brightColor * ${glf(m.sky_scale)}) : vec3(0.0); }`);
    return lines.join("\n");
  }
}
const singleSphere = (center = [0, 0, 0], radius = 1, material) => new CsgScene(material).sphere(center, radius);
class Mandelbulb extends Scene {
  constructor(power = 8, iterations = 8, bailout = 2, material) { super(RM.SCENE_MANDELBULB, [power, iterations, bailout], material); }
}

// ---- host side of the job -------------------------------------------------------------
function* halton(b) {  // util/Halton.tsx:1-19, value for value
  for (let i = 1; ; i++) { let num = 0, den = 1; for (let k = i; k > 0; k = Math.floor(k / b)) { num = num * b + (k % b); den *= b; } yield num / den; }
}
let halton2 = halton(2), halton3 = halton(3);  // module-level like RenderJobExecutor.tsx:70-71: continues across jobs
const resetHalton = () => { halton2 = halton(2); halton3 = halton(3); };

function uniformsFromSchema(schema, randNoise) {  // RenderJobExecutor.tsx:212-297
  const cam = schema.camera, r = schema.render, counts = schema.reflectionIterationCounts;
  if (counts.length > RM.MAX_BOUNCES || schema.lights.length > RM.MAX_LIGHTS) throw new Error("at most 10 bounces / 10 lights");
  const mode = cam.mode.type;
  const pos = [], col = [], size = [];
  for (const l of schema.lights) { pos.push(...(l.type === "point" ? l.position : l.direction)); col.push(...l.color); size.push(l.type === "point" ? l.size : 0); }
  return packUniforms({
    blendWithPreviousFactor: r.blendWithPreviousFrameFactor, randNoise, position: cam.position, rotation: Array.from(cam.rotation),
    dofAmount: schema.dof.amount, dofFocalPlaneDistance: schema.dof.distance,
    cameraMode: ["perspective", "orthographic", "panoramic"].indexOf(mode),
    fov: mode === "perspective" ? cam.mode.fov : mode === "orthographic" ? cam.mode.size : 1,
    reflections: counts.length, raymarchingSteps: counts[0], indirectLightingRaymarchingSteps: counts.length > 1 ? counts[1] : counts[0],
    aspect: r.width / r.height, fogDensity: schema.fogDensity, exposure: r.exposure / r.samplesPerPixel,
    raymarchingStepCountsArray: counts, blendMode: r.blendMode === "additive" ? 1 : 0, renderMode: r.renderMode === "preview" ? 1 : 0,
    lightPositions: pos, lightColors: col, lightSizes: size, lightCount: schema.lights.length, showDofFocalPlane: schema.dof.showFocusedArea ? 1 : 0,
  });
}

// :167-180.  The reference passes (x1, y1, x2, y2) to gl.scissor(x, y, width, height): identical to the intended tile
// for subdivisions <= 2, over-covering from 3 on.  Default: the intent; render.referenceScissor = true: the reference's rectangle.
function tileRect(schema, xp, yp) {
  const r = schema.render, n = r.subdivisions;
  const x1 = Math.floor((r.width / n) * xp), y1 = Math.floor((r.height / n) * yp);
  const x2 = Math.ceil((r.width / n) * (xp + 1)), y2 = Math.ceil((r.height / n) * (yp + 1));
  if (r.referenceScissor) return new Int32Array([x1, y1, Math.min(x2, r.width - x1), Math.min(y2, r.height - y1)]);
  return new Int32Array([x1, y1, x2 - x1, y2 - y1]);
}

// A scene cache keeps this many entries (a Map iterates in insertion order: the first key is the least recently used).  The
// reference's programCache grows with every edit of the shader text, for a page's lifetime; a long-running host that animates scene
// parameters would otherwise keep a device table per distinct scene (the culling grids of long CSG tables -- 31.5 MB per 64 rows --
// are bounded by the library itself, by bytes: rm_ctx_cull_stats).  A scene a job still renders is pinned (doRenderJob: jobs yield
// between samples) and is never the one that goes.
const SCENE_CACHE_ENTRIES = 64;
function evictScenes(map, destroy, pins, keep) {  // `keep`: the key being handed out (with 64 pinned scenes it is the only unpinned one)
  let spare = map.size - SCENE_CACHE_ENTRIES;
  for (const k of Array.from(map.keys())) {
    if (spare <= 0) break;
    if ((pins && pins.get(k) > 0) || k === keep) continue;
    const v = map.get(k); map.delete(k); destroy(v); spare--;
  }
}
const scenePins = {  // mixed into both contexts, for hosts that hold handles themselves (doRenderJob does not pin: see there): pinScene(scene) -> [key, handle or error value]; unpinScene(key)
  pinScene(scene) { const hit = this.getScene(scene), key = scene.key(); this.pins.set(key, (this.pins.get(key) || 0) + 1); return [key, hit]; },
  unpinScene(key) { const n = (this.pins.get(key) || 0) - 1; if (n > 0) this.pins.set(key, n); else { this.pins.delete(key); this.evict(); } },
};

class RenderJobContext {  // RenderJobContext + loadRenderJobContext (LoadRenderJobContext.tsx:162-287)
  // new RenderJobContext(device?, flags?) or new RenderJobContext({ device, flags, gbuffer, moments })
  // moments: every framebuffer also keeps the luminance moments plane (RM_FB_MOMENTS) the variance-guided denoiser reads
  constructor(device = 0, flags = RM.RENDER_STRICT) {
    let gbuffer = "f32", moments = false;
    if (device !== null && typeof device === "object") ({ device = 0, flags = RM.RENDER_STRICT, gbuffer = "f32", moments = false } = device);
    this.gbuffer = gbuffer; this.gbufferCode = gbufferCode(gbuffer);  // (before any device work)
    this.moments = !!moments;
    this.ctx = addon.ctxCreate(device); this.flags = flags; this.scenes = new Map(); this.pins = new Map(); this.live = new Map(); this.purgatory = [];
  }
  evict(keep) { evictScenes(this.scenes, (s) => { if (!(s && s.infoLog)) addon.sceneDestroy(s); }, this.pins, keep); }
  getScene(scene) {  // programCache.getProgram: results AND errors are cached (ShaderCache.tsx:91-119); bounded, least recently used out first
    const key = scene.key();
    if (!this.scenes.has(key)) {
      try { const d = scene.desc(); this.scenes.set(key, addon.sceneCreate(this.ctx, d.desc, d.prims, d.surfaces)); }
      catch (e) { this.scenes.set(key, { type: "fragment", infoLog: String(e.message) }); }
      this.evict(key);
    } else { const hit = this.scenes.get(key); this.scenes.delete(key); this.scenes.set(key, hit); }
    return this.scenes.get(key);
  }
  fboCreate(w, h, frameid) {  // :186-223
    const key = `${w}x${h}#${frameid}`;
    if (this.live.has(key)) return this.live.get(key);
    const i = this.purgatory.findIndex((e) => e.w === w && e.h === h);
    let fb;
    if (i >= 0) { const e = this.purgatory.splice(i, 1)[0]; if (e.frameid !== frameid) addon.fbClear(e.fb); fb = e.fb; }
    else fb = addon.fbCreate(this.ctx, w, h, 0, h, this.gbufferCode | (this.moments ? RM.FB_MOMENTS : 0));
    const info = { fb, width: w, height: h, frameid, download: (plane = 0) => { const out = new Float32Array(w * h * 4); addon.fbDownload(this.ctx, fb, plane, out); return out; },
                   // the present pass (display.frag) on the GPU: RGBA8, row 0 = bottom
                   // opts.denoise (true or the parameters of denoiseParams): the denoised colour through the same pass (rm_present_denoised);
                   // "variance" or { mode: "variance", ... } (denoiseVarianceParams): the variance-guided filter's (rm_present_denoised_variance)
                   // opts.despeckle (true or the parameters of despeckleParams): the firefly filter ahead of either (rm_present_filtered);
                   // without it the calls are the ones above
                   // opts.display (the parameters of displayParams -- gain, tone "clip" / "reinhard" / "aces", white --, or "auto" /
                   // { auto: true or statsExposure's parameters, tone, white }: the gain from stats of the same chain): the display
                   // transform behind the blur (rm_present_display); without it the calls are the ones above
                   present: (samples, opts = {}) => {
                     const out = new Uint8Array(w * h * 4);
                     const d = opts.denoise;
                     if (opts.display !== undefined && opts.display !== null) {
                       addon.presentDisplay(this.ctx, fb, samples, filters(opts), info.displayBlock(samples, opts), out);
                       return out;
                     }
                     if (opts.despeckle !== undefined && opts.despeckle !== null && opts.despeckle !== false) {
                       addon.presentFiltered(this.ctx, fb, samples, filters(opts), out);
                       return out;
                     }
                     if (d === undefined || d === null || d === false) addon.present(this.ctx, fb, samples, out);
                     else if (isVarianceMode(d)) addon.presentDenoisedVariance(this.ctx, fb, samples, denoiseVarianceParams(d), out);
                     else addon.presentDenoised(this.ctx, fb, samples, denoiseParams(d && d.mode === "atrous" ? withoutMode(d) : d), out);
                     return out; },
                   // the RmDisplay of opts.display: displayParams', or with "auto" the gain rm_stats_exposure gives for the same chain's statistics
                   displayBlock: (samples, opts = {}) => {
                     const disp = opts.display;
                     if (!displayIsAuto(disp)) return displayParams(disp);
                     const { auto = true, ...rest } = disp === "auto" ? {} : disp;
                     if ("gain" in rest) throw new TypeError("display: give either a gain or auto");
                     const p = displayParams(rest);
                     p.gain = statsExposure(info.stats(samples, opts), auto === true ? undefined : auto);
                     return p; },
                   // the blurred, exposed frame as floats (rm_present_linear): (e.r, e.g, e.b, 1), row 0 = bottom; opts as present takes them
                   linear: (samples, opts = {}) => { const out = new Float32Array(w * h * 4);
                     addon.presentLinear(this.ctx, fb, samples, filters(opts), info.displayBlock(samples, opts), out); return out; },
                   // the luminance statistics (rm_frame_stats) of the colour plane, or with opts.despeckle / opts.denoise of the chain's result
                   stats: (samples, opts = {}) => { const raw = new ArrayBuffer(addon.sizes().RmFrameStats);
                     const on = (v) => !(v === undefined || v === null || v === false);
                     addon.frameStats(this.ctx, fb, samples, on(opts.despeckle) || on(opts.denoise) ? filters(opts) : null, raw); return unpackStats(raw); },
                   // the colour plane after the chain despeckle -> denoise (rm_filter): opts = { despeckle, denoise } as present takes them
                   filter: (samples, opts = {}) => { const out = new Float32Array(w * h * 4); addon.filter(this.ctx, fb, samples, filters(opts), out); return out; },
                   // the colour plane after the variance-guided filter (rm_denoise_variance; needs { moments: true }): as denoise
                   denoiseVariance: (samples, params) => { const out = new Float32Array(w * h * 4); addon.denoiseVariance(this.ctx, fb, samples, denoiseVarianceParams(params), out); return out; },
                   // the colour plane after the G-buffer-guided a-trous filter (rm_denoise): Float32Array, colour-plane units, row 0 = bottom
                   denoise: (samples, params) => { const out = new Float32Array(w * h * 4); addon.denoise(this.ctx, fb, samples, denoiseParams(params), out); return out; },
                   // canvas.toDataURL("image/png"), index.tsx:470-476
                   toDataURL: (samples, opts = {}) => "data:image/png;base64," + encodePng(info.present(samples, opts), w, h).toString("base64") };
    this.live.set(key, info);
    return info;
  }
  fboDelete(w, h, frameid) {  // :227-248: parked in a <= 3 entry purgatory
    const key = `${w}x${h}#${frameid}`, info = this.live.get(key);
    if (!info) return;
    this.live.delete(key);
    this.purgatory.push({ w, h, frameid, fb: info.fb });
    while (this.purgatory.length > 3) addon.fbDestroy(this.purgatory.shift().fb);
  }
  // ---- mesh extraction (include/hip_raymarch.h "mesh extraction"); scene: a composer object, through the scene cache ----
  sceneHandle(scene) { const h = this.getScene(scene); if (h && h.infoLog) throw new Error("scene: " + h.infoLog); return h; }
  // the scene's distance at every corner of grid (meshGrid): Float32Array, x fastest -- rm_probe's RM_PROBE_SDF at the corners, bit for bit
  sdfGrid(scene, grid, flags = 0) {
    const out = new Float32Array((grid.n[0] + 1) * (grid.n[1] + 1) * (grid.n[2] + 1));
    addon.sdfGrid(this.ctx, this.sceneHandle(scene), grid, flags, out);
    return out;
  }
  // the level set opts.iso as { positions, normals | null, colours | null, triangles, cells, timings } (opts: meshParams'), through a pipeline on
  // the GPU whose stages are all opt-in -- undefined / null = the stage is off, true = its defaults, else its block's options -- in this order:
  // extract: rm_mesh_extract; with sharp (meshSharp's) rm_mesh_extract_sharp, the same triangles with each vertex at its cell's QEF minimiser
  //   (hard edges and corners stay sharp); with slabs (true, a number of cell layers or meshSlabs') rm_mesh_extract_slabs / _sharp_slabs, the same
  //   mesh byte for byte, made from one window of z layers at a time -- which also takes a meshGrid(lo, hi, n, { slabs: true }) beyond 2^28 corners
  // simplify (meshSimplify's { grid, keepDuplicates }; no `true`): the vertices of every cell of that grid of clusters merged into one
  //   (rm_mesh_simplify); the result's cells index the cluster grid.  With quadric (meshQuadric's; with simplify only) rm_mesh_simplify_quadric, the
  //   same mesh with every cluster's vertex at the minimiser of its plane quadrics
  // keep (meshKeep's): the connected components filtered before anything is copied (rm_mesh_filter; the defaults drop the unreferenced vertices)
  // project (meshProject's): the vertices moved onto the scene's level set by Newton steps (rm_mesh_project); every later stage sees the projected
  //   mesh.  iso, where not given, is the extraction's; reach, where not given, is meshProjectReach of the grid the mesh lies on (the cluster grid
  //   with simplify, else the sampling grid).  Adds projection (RmMeshProjection's fields in camel case, and milliseconds: the rounds and the
  //   normals) and residual (Float32Array(V): the distance minus iso at the new vertices); timings stays the producing mesh's
  // measures (truthy): the mesh is measured before anything is copied (rm_mesh_measure).  Adds measures: RmMeshMeasures' fields in camel case --
  //   the counts as Numbers (all below 2^53: V, T < 2^32 and E <= 3 T), closed as a boolean, lo / hi as arrays --, componentEdges:
  //   BigUint64Array(4 C) of (edges, boundary, irregular, unbalanced) per component as the raw uint64 rows, and milliseconds: [topology, geometry]
  // components (truthy): adds labels (Uint32Array(V)) and componentSizes (Uint32Array(2 C): vertices, triangles per component) (rm_mesh_components)
  // occlusion (meshOcclusion's): adds occlusion (Float32Array(V), 1 = open), baked from the scene's distance field (rm_mesh_occlusion); its
  //   milliseconds are timings[3], which is there only with it
  // deviation (meshDeviation's): how far the triangles lie off the scene's level set at order * order fixed samples each (rm_mesh_deviation).  iso,
  //   where not given, is the extraction's.  Adds deviation (RmMeshDeviationReport's fields in camel case, and milliseconds) and triangleDeviation
  //   (Float32Array(T): each triangle's largest |distance - iso| over its samples)
  // refine (meshRefine's): behind project and before measures, components, occlusion and deviation, the edges whose midpoint lies further than
  //   `tolerance` off the scene's level set are split, for `rounds` rounds (rm_mesh_refine); every round's mesh is projected with the project block, or
  //   with its defaults (iso and reach filled as above) where none is given.  iso, where not given, is the extraction's; tolerance, where not given,
  //   is meshRefineTolerance of the grid the mesh lies on (a default, not a bar).  The criterion looks at edge midpoints only: deviation remains the
  //   judge.  Adds refinement (RmMeshRefinement's fields in camel case, the per-round counts as arrays of eight, and milliseconds).  Only with refine
  //   is the addon's extractMeshRefined called, which takes all fifteen arguments
  extractMesh(scene, grid, opts, sharp, keep, components, simplify = null, quadric = null, occlusion = null, measures = false, slabs = null, project = null, deviation = null, refine = null) {
    const o = meshOptions(grid, opts, { sharp, keep, components, simplify, quadric, occlusion, measures, slabs, project, deviation, refine });
    const stages = [o.sharp, o.keep, o.components, o.simplify, o.quadric, o.occlusion, o.measures, o.project, o.deviation], h = this.sceneHandle(scene);
    if (o.refine !== null) return addon.extractMeshRefined(this.ctx, h, grid, o.refine, o.slabs, o.params, ...stages);
    if (o.slabs !== null) return addon.extractMeshSlabs(...meshArguments([this.ctx, h, grid, o.slabs, o.params, ...stages], 12));
    return addon.extractMesh(...meshArguments([this.ctx, h, grid, o.params, ...stages], 4, 5));
  }
  // the mesher alone on the caller's field: values Float32Array of the grid's corners, x fastest (rm_mesh_from_values; with slabs
  // rm_mesh_from_values_slabs); keep, components, simplify, quadric, measures, slabs: as in extractMesh
  meshFromValues(grid, values, iso = 0, keep, components, simplify, quadric, measures, slabs) {
    if (!(values instanceof Float32Array)) throw new TypeError("meshFromValues: values must be a Float32Array");
    if (!finite(iso)) throw new RangeError("mesh: iso must be a finite number");
    const o = meshOptions(grid, undefined, { keep, components, simplify, quadric, measures, slabs });
    const stages = [o.keep, o.components, o.simplify, o.quadric, o.measures];
    if (o.slabs !== null) return addon.meshFromValuesSlabs(...meshArguments([this.ctx, grid, values, iso, o.slabs, ...stages], 10));
    return addon.meshFromValues(...meshArguments([this.ctx, grid, values, iso, ...stages], 4, 4));
  }
  close() { for (const e of this.purgatory) addon.fbDestroy(e.fb); for (const v of this.live.values()) addon.fbDestroy(v.fb);
            for (const s of this.scenes.values()) if (!(s && s.infoLog)) addon.sceneDestroy(s); addon.ctxDestroy(this.ctx); }
}

// A frame sharded over several GPUs by THIS process -- the reference's host is one thread with one render loop
// (index.tsx:120), and so is a Node host: one native context per GPU, each holding one part of the frame's 8-row stripes
// (rm_fb_create_striped: pixel coordinates stay global, so the assembled frame has the single-GPU bits).  doRenderJob
// hands every batch of samples to each context in turn -- the launches are asynchronous, so the GPUs render
// concurrently -- and `present(samples)` of the framebuffer set is rm_present_sharded: every GPU tone-maps (or, with
// depth of field, packs) its rows, peer copies over xGMI bring them to the first GPU, which puts them in image order and
// runs the blur.  Same interface as RenderJobContext, so the reference's `present` callback does not change.
// (The tile loop of the reference, RenderJobExecutor.tsx:148-182, is the precedent for cutting a job's frame.)
const STRIPE_ROWS = 8;
class ShardedRenderJobContext {
  // new ShardedRenderJobContext(devices?, flags?, samplesInFlight?) or new ShardedRenderJobContext({ devices, flags, samplesInFlight, gbuffer })
  constructor(devices = [0], flags = RM.RENDER_STRICT, samplesInFlight = 3) {
    let gbuffer = "f32", moments = false;
    if (devices !== null && typeof devices === "object" && !Array.isArray(devices))
      ({ devices = [0], flags = RM.RENDER_STRICT, samplesInFlight = 3, gbuffer = "f32", moments = false } = devices);
    this.gbuffer = gbuffer; this.gbufferCode = gbufferCode(gbuffer);
    if (moments)
      throw new RangeError("ShardedRenderJobContext: moments needs framebuffers holding the whole frame (the denoiser reads rows other GPUs hold)");
    if (!Array.isArray(devices) || devices.length < 1) throw new TypeError("ShardedRenderJobContext(devices: number[], flags?)");
    this.devices = devices.slice(); this.flags = flags;
    this.ctxs = devices.map((d) => addon.ctxCreate(d));
    for (const c of this.ctxs) addon.setSamplesInFlight(c, samplesInFlight);
    this.ctx = this.ctxs[0];
    this.scenes = new Map(); this.pins = new Map(); this.live = new Map(); this.purgatory = [];
  }
  evict(keep) { evictScenes(this.scenes, (s) => { if (s.handles) for (const h of s.handles) addon.sceneDestroy(h); }, this.pins, keep); }
  getScene(scene) {  // one handle per context; a failure (on any of them) is cached like a failed compile
    const key = scene.key();
    if (!this.scenes.has(key)) {
      const made = [];
      try { const d = scene.desc(); for (const c of this.ctxs) made.push(addon.sceneCreate(c, d.desc, d.prims, d.surfaces)); this.scenes.set(key, { handles: made }); }
      catch (e) { for (const h of made) addon.sceneDestroy(h); this.scenes.set(key, { type: "fragment", infoLog: String(e.message) }); }
      this.evict(key);
    } else { const hit = this.scenes.get(key); this.scenes.delete(key); this.scenes.set(key, hit); }
    return this.scenes.get(key);
  }
  fboCreate(w, h, frameid) {
    const key = `${w}x${h}#${frameid}`;
    if (this.live.has(key)) return this.live.get(key);
    const i = this.purgatory.findIndex((e) => e.w === w && e.h === h);
    let fbs;
    if (i >= 0) { const e = this.purgatory.splice(i, 1)[0]; if (e.frameid !== frameid) for (const fb of e.fbs) addon.fbClear(fb); fbs = e.fbs; }
    else {
      fbs = [];
      try { this.ctxs.forEach((c, p) => fbs.push(addon.fbCreateStriped(c, w, h, STRIPE_ROWS, this.ctxs.length, p, this.gbufferCode))); }
      catch (e) { for (const fb of fbs) addon.fbDestroy(fb); throw e; }
    }
    const info = { fbs, width: w, height: h, frameid, sharded: true, dof: false,
                   rows: () => fbs.map((fb) => addon.fbRows(fb)),
                   // the canvas of the assembled frame (display.frag, with its blur when the job has depth of field): RGBA8, row 0 = bottom
                   present: (samples, dof = info.dof, opts = {}) => {
                     if (opts.denoise !== undefined || (dof !== null && typeof dof === "object"))
                       throw new Error("present: denoising a sharded frame is not supported (the filter reads rows other GPUs hold)");
                     if (opts.despeckle !== undefined)
                       throw new Error("present: the firefly filter on a sharded frame is not supported (it reads rows other GPUs hold)");
                     if (opts.display !== undefined)
                       throw new Error("present: the display transform on a sharded frame is not supported yet (the sharded presents keep the reference's transform)");
                     const out = new Uint8Array(w * h * 4); addon.presentSharded(this.ctxs, fbs, samples, !!dof, out); return out; },
                   // the same in two halves (rm_present_sharded_start / _finish): startPresent snapshots and sends and returns at once, so a
                   // `present` callback that calls it lets doRenderJob hand out the next samples while the frame travels; finishPresent
                   // (at the next callback, or whenever the canvas is wanted) returns the canvas of THAT present.  One at a time.
                   startPresent: (samples, dof = info.dof) => { addon.presentShardedStart(this.ctxs, fbs, samples, !!dof); info.pendingPresent = true; },
                   finishPresent: () => {
                     // the pending present lives on the contexts, not on this framebuffer set: only the set that started it may finish it
                     // (another set's canvas may be smaller; the library checks the buffer's size as well)
                     if (!info.pendingPresent) throw new Error("finishPresent: this framebuffer set has no present pending (startPresent was called on another set, or not at all)");
                     const out = new Uint8Array(w * h * 4); addon.presentShardedFinish(this.ctxs, out); info.pendingPresent = false; return out; },
                   pendingPresent: false,
                   toDataURL: (samples) => "data:image/png;base64," + encodePng(info.present(samples), w, h).toString("base64") };
    this.live.set(key, info);
    return info;
  }
  fboDelete(w, h, frameid) {
    const key = `${w}x${h}#${frameid}`, info = this.live.get(key);
    if (!info) return;
    this.live.delete(key);
    this.purgatory.push({ w, h, frameid, fbs: info.fbs });
    while (this.purgatory.length > 3) for (const fb of this.purgatory.shift().fbs) addon.fbDestroy(fb);
  }
  close() {
    for (const e of this.purgatory) for (const fb of e.fbs) addon.fbDestroy(fb);
    for (const v of this.live.values()) for (const fb of v.fbs) addon.fbDestroy(fb);
    for (const s of this.scenes.values()) if (s.handles) for (const h of s.handles) addon.sceneDestroy(h);
    for (const c of this.ctxs) addon.ctxDestroy(c);
  }
}

Object.assign(RenderJobContext.prototype, scenePins);
Object.assign(ShardedRenderJobContext.prototype, scenePins);

async function doRenderJob(schema, context) {  // RenderJobExecutor.tsx:77
  const fail = (why) => function* () { return { success: false, why }; };
  const r = schema.render;
  let framebuffers;
  try { framebuffers = context.fboCreate(r.width, r.height, r.frameid); }
  catch (e) { return fail({ type: "general", infoLog: "Failed to load framebuffers. " + e.message }); }
  if (!schema.sdfScene) return fail({ type: "fragment", infoLog: "no sdfScene: the HIP back end takes a composed scene, not GLSL text" });
  const compiled = context.getScene(schema.sdfScene);
  if (compiled && compiled.infoLog !== undefined) return fail(compiled);
  let samples = 0;
  // a sharded context: the same calls on every GPU's context, each with its part of the stripes (the tile is clipped to them)
  const ctxs = framebuffers.sharded ? context.ctxs : [context.ctx];
  const fbs = framebuffers.sharded ? framebuffers.fbs : [framebuffers.fb];
  if (framebuffers.sharded) framebuffers.dof = schema.dof.amount !== 0;  // what a present gathers (rm_present_sharded)
  // (a sharded set's present is ordered on the contexts' streams behind the samples: no host-side wait before it, so that a
  // callback using startPresent overlaps the travelling frame with the next samples; the single context waits as it always did)
  const syncAll = () => { if (!framebuffers.sharded) for (const c of ctxs) addon.sync(c); };
  const syncEnd = () => { for (const c of ctxs) addon.sync(c); };
  return function* (present) {
    // The job yields between samples, and other jobs may bring in more scenes than the cache holds meanwhile.  No pin is held across a
    // yield (round 6: a JS generator that is started and then dropped without .return() never runs its `finally`, so a pin taken for
    // its lifetime would keep the scene un-evictable for the life of the context): the scene is looked up again -- and, had it been
    // evicted, made again -- in front of every batch of native calls, with nothing in between that could suspend the job.
    for (let yp = 0; yp < r.subdivisions; yp++) for (let xp = 0; xp < r.subdivisions; xp++) {
      const tile = tileRect(schema, xp, yp);
      for (let left = r.samplesPerPixel; left > 0;) {
        if (samples % r.sampleYieldInterval === 0) { syncAll(); present(schema, context, framebuffers, samples); yield; }
        // the samples up to the next yield differ in randNoise only (:219-222): one native call for all of them
        const k = Math.min(left, r.sampleYieldInterval - samples % r.sampleYieldInterval);
        const noise = new Float32Array(2 * k);
        for (let i = 0; i < k; i++) { noise[2 * i] = halton2.next().value; noise[2 * i + 1] = halton3.next().value; }
        const u = uniformsFromSchema(schema, [noise[0], noise[1]]);
        const scene = context.getScene(schema.sdfScene);
        if (scene && scene.infoLog !== undefined) { context.fboDelete(r.width, r.height, r.frameid); return { success: false, why: scene }; }
        const scenes = framebuffers.sharded ? scene.handles : [scene];
        for (let g = 0; g < ctxs.length; g++) {
          if (k === 1) addon.renderSample(ctxs[g], scenes[g], fbs[g], u, tile, context.flags);
          else addon.renderSamples(ctxs[g], scenes[g], fbs[g], u, noise, tile, context.flags);
        }
        samples += k; left -= k;
      }
    }
    context.fboDelete(r.width, r.height, r.frameid);
    syncEnd();  // the job's last word: an asynchronous failure becomes this call's exception (the caller's {success: false})
    present(schema, context, framebuffers, samples);
    return { success: true };
  };
}

// ---- parameters of the frame filters (include/hip_raymarch.h RmDenoise, RmDenoiseVariance, RmDespeckle and their rm_*_default) ----
const DENOISE_DEFAULTS = { iterations: 5, sigma_color: 2.5, sigma_normal: 2.0, sigma_depth: 0.2 };
const DENOISE_VARIANCE_DEFAULTS = { iterations: 3, sigma_luminance: 4.0, sigma_normal: 1.0, sigma_depth: 0.2 };
const DESPECKLE_DEFAULTS = { radius: 2, rank: 1, gain: 3.0, floor: 0.1, repair: 1 };
// One table per block for filterParams: the prefix of its messages, the forms that mean "the defaults" as the refusal of any other
// form names them, the defaults, the `mode` an object may name, the fields a boolean may set, and the library's own checks in the
// library's order as field: [holds, text].
const finite = (v) => typeof v === "number" && Number.isFinite(v);
const POSITIVE = [(v) => finite(v) && v > 0, "must be finite and > 0"];
const integerIn = (lo, hi, shown = hi) => [(v) => Number.isInteger(v) && v >= lo && v <= hi, "must be an integer in " + lo + ".." + shown];
const FILTER_BLOCKS = {
  atrous: { label: "denoise", forms: "true", defaults: DENOISE_DEFAULTS,
            checks: { iterations: integerIn(0, 8), sigma_color: POSITIVE, sigma_normal: POSITIVE, sigma_depth: POSITIVE } },
  variance: { label: "denoise", forms: "\"variance\"", defaults: DENOISE_VARIANCE_DEFAULTS, mode: "variance",
              checks: { iterations: integerIn(0, 8), sigma_luminance: POSITIVE, sigma_normal: POSITIVE, sigma_depth: POSITIVE } },
  despeckle: { label: "despeckle", forms: "true", defaults: DESPECKLE_DEFAULTS, flags: ["repair"],
               checks: { radius: [(v) => v === 1 || v === 2, "must be 1 or 2"], rank: integerIn(0, 3), gain: [(v) => finite(v) && v >= 1, "must be finite and >= 1"],
                         floor: [(v) => finite(v) && v >= 0, "must be finite and >= 0"], repair: [Number.isInteger, "must be an integer (0 = off)"] } },
};
// true / undefined / null / the block's mode = the defaults, or an object with some of the defaults' fields (and the block's mode);
// checked as the library checks them
function filterParams({ label, forms, defaults, mode, flags = [], checks }, params) {
  const p = { ...defaults };
  if (params !== undefined && params !== null && params !== true && !(mode !== undefined && params === mode)) {
    if (typeof params !== "object") throw new TypeError(label + ": expected " + forms + " or an object of parameters");
    for (const [k, v] of Object.entries(params)) {
      if (mode !== undefined && k === "mode") { if (v !== mode) throw new TypeError(label + ": mode " + v + " is not the " + mode + "-guided filter"); continue; }
      if (!(k in defaults)) throw new TypeError(label + ": unknown parameter " + k);
      p[k] = flags.includes(k) && typeof v === "boolean" ? Number(v) : v;
    }
  }
  for (const [k, [holds, text]] of Object.entries(checks)) if (!holds(p[k])) throw new RangeError(label + ": " + k + " " + text);
  return p;
}
function denoiseParams(params) { return filterParams(FILTER_BLOCKS.atrous, params); }
function denoiseVarianceParams(params) { return filterParams(FILTER_BLOCKS.variance, params); }
function despeckleParams(params) { return filterParams(FILTER_BLOCKS.despeckle, params); }
function isVarianceMode(d) { return d === "variance" || (d !== null && typeof d === "object" && d.mode === "variance"); }
function withoutMode(d) { const { mode, ...rest } = d; return rest; }
// the addon's RmFilters of { despeckle, denoise }: a stage that is undefined / null / false is off
function filters(opts = {}) {
  const off = (v) => v === undefined || v === null || v === false;
  const f = { despeckle: off(opts.despeckle) ? null : despeckleParams(opts.despeckle), denoise: RM.DENOISE_NONE, atrous: null, variance: null };
  const d = opts.denoise;
  if (!off(d)) {
    if (isVarianceMode(d)) { f.denoise = RM.DENOISE_VARIANCE; f.variance = denoiseVarianceParams(d); }
    else { f.denoise = RM.DENOISE_ATROUS; f.atrous = denoiseParams(d && d.mode === "atrous" ? withoutMode(d) : d); }
  }
  return f;
}

// ---- the display transform and the frame statistics (include/hip_raymarch.h RmDisplay, RmFrameStats, RmAutoExposure) ----
const TONES = { clip: 0, reinhard: 1, aces: 2 };
const DISPLAY_DEFAULTS = { gain: 1.0, tone: "clip", white: 4.0 };
const AUTO_EXPOSURE_DEFAULTS = { key: 0.18, low: 0.10, high: 0.95, min_gain: 2 ** -10, max_gain: 2 ** 10 };
const STATS_BINS = 512;
// undefined / null / true = the defaults (gain 1, the hard clip), or an object with some of gain, tone ("clip" | "reinhard" | "aces"), white;
// checked as the library checks them (white for "reinhard" alone); returns { gain, tone: the RM_TONE_* number, white }
function displayParams(params) {
  const p = { ...DISPLAY_DEFAULTS };
  if (params !== undefined && params !== null && params !== true) {
    if (typeof params !== "object") throw new TypeError("display: expected \"auto\" or an object of parameters");
    for (const [k, v] of Object.entries(params)) {
      if (!(k in DISPLAY_DEFAULTS)) throw new TypeError("display: unknown parameter " + k);
      p[k] = v;
    }
  }
  if (!POSITIVE[0](p.gain)) throw new RangeError("display: gain " + POSITIVE[1]);
  if (!(typeof p.tone === "string" && Object.prototype.hasOwnProperty.call(TONES, p.tone))) throw new RangeError("display: tone must be \"clip\", \"reinhard\" or \"aces\"");
  if (p.tone === "reinhard" && !POSITIVE[0](p.white)) throw new RangeError("display: white " + POSITIVE[1]);
  return { gain: p.gain, tone: TONES[p.tone], white: finite(p.white) ? p.white : DISPLAY_DEFAULTS.white };
}
function displayIsAuto(d) { return d === "auto" || (d !== null && typeof d === "object" && "auto" in d); }
// the RmFrameStats the addon filled, as { pixels, below, above, nonFinite, min, max, hist: Float64Array(512) } (counts stay below 2^53)
function unpackStats(raw) {
  const v = new DataView(raw);
  const u64 = (at) => Number(v.getBigUint64(at, true));
  const hist = new Float64Array(STATS_BINS);
  for (let b = 0; b < STATS_BINS; b++) hist[b] = u64(40 + 8 * b);
  return { pixels: u64(0), below: u64(8), above: u64(16), nonFinite: u64(24), min: v.getFloat32(32, true), max: v.getFloat32(36, true), hist };
}
function packStats(stats) {
  if (stats === null || typeof stats !== "object" || !stats.hist || stats.hist.length !== STATS_BINS) throw new TypeError("stats: expected what fb.stats returns");
  const raw = new ArrayBuffer(addon.sizes().RmFrameStats), v = new DataView(raw);
  [stats.pixels, stats.below, stats.above, stats.nonFinite].forEach((n, i) => v.setBigUint64(8 * i, BigInt(n), true));
  v.setFloat32(32, stats.min, true); v.setFloat32(36, stats.max, true);
  for (let b = 0; b < STATS_BINS; b++) v.setBigUint64(40 + 8 * b, BigInt(stats.hist[b]), true);
  return raw;
}
// rm_stats_exposure: the gain that brings the log-average luminance between two percentiles to `key`; opts: some of AUTO_EXPOSURE_DEFAULTS' fields
function statsExposure(stats, opts) {
  const p = { ...AUTO_EXPOSURE_DEFAULTS };
  if (opts !== undefined && opts !== null && opts !== true) {
    if (typeof opts !== "object") throw new TypeError("auto exposure: expected an object of parameters");
    for (const [k, v] of Object.entries(opts)) {
      if (!(k in AUTO_EXPOSURE_DEFAULTS)) throw new TypeError("auto exposure: unknown parameter " + k);
      if (!finite(v)) throw new RangeError("auto exposure: " + k + " must be a finite number");
      p[k] = v;
    }
  }
  return addon.statsExposure(packStats(stats), p);
}
// rm_stats_percentile: the upper edge of the bin that holds the ceil(q N)-th smallest binned pixel
function statsPercentile(stats, q) {
  if (!(typeof q === "number" && q >= 0 && q <= 1)) throw new RangeError("statsPercentile: q must be in [0, 1]");
  return addon.statsPercentile(packStats(stats), q);
}

// ---- mesh extraction: the grid, the parameters and the PLY writer (include/hip_raymarch.h RmGrid, RmMeshParams) ----
const MESH_DEFAULTS = { iso: 0.0, normals: 1, normalDelta: 1e-5, colours: 0, flags: 0 };
// { lo, hi, n }: n = CELLS per axis between the corners lo and hi; checked as the library checks an RmGrid.  opts.slabs: true lifts the bound of
// 2^28 corners and nothing else ({ lo, hi, n, slabs: true }): a grid for extractMesh / meshFromValues with slabs
function meshGrid(lo, hi, n, opts) {
  const slabs = !!(opts && opts.slabs);
  const three = (a) => Array.isArray(a) && a.length === 3 && a.every((v) => typeof v === "number");
  if (!three(lo) || !three(hi) || !three(n)) throw new TypeError("grid: lo, hi and n take three numbers each");
  if (!n.every((v) => Number.isInteger(v) && v >= 1 && v <= 1024)) throw new RangeError("grid: n must be integers in 1..1024 cells per axis");
  for (let a = 0; a < 3; a++) {
    const l = Math.fround(lo[a]), h = Math.fround(hi[a]), step = Math.fround(Math.fround(h - l) / n[a]);
    if (!finite(l) || !finite(h) || !finite(step) || !(step > 0)) throw new RangeError("grid: lo, hi and the cell size (hi - lo) / n must be finite, the cell size > 0");
  }
  if (!slabs && (n[0] + 1) * (n[1] + 1) * (n[2] + 1) > 2 ** 28) throw new RangeError("grid: at most 2^28 corners");
  return slabs ? { lo: lo.slice(), hi: hi.slice(), n: n.slice(), slabs: true } : { lo: lo.slice(), hi: hi.slice(), n: n.slice() };
}
// ---- the parameter blocks of the mesh calls (include/hip_raymarch.h RmMeshParams, RmMeshSharp, ... RmMeshDeviation) ----
// Every block but simplify: undefined / null = the defaults, or an object with some of the defaults' fields; checked as the library checks it.
// params: iso, normals, normalDelta, colours, flags (RM.RENDER_FAST, RM.RENDER_NO_CULL); returns { iso, normals: 0 | 1, normalDelta, colours: 0 | 1, flags }
// sharp (extractMesh): refine, normalDelta, threshold
const MESH_SHARP_DEFAULTS = { refine: 6, normalDelta: 2 ** -10, threshold: 0.1 };
// keep (extractMesh / meshFromValues): minTriangles (a component passes with at least that many triangles) and largest (0 = every passing
// component, k > 0 = only the k with the most triangles, the lower component index first among equals); integers in 0..1e9, what the addon's
// integer fields hold
const MESH_KEEP_DEFAULTS = { minTriangles: 1, largest: 0 };
// slabs (extractMesh / meshFromValues): layers (the cell layers per slab, 0 = chosen by the library; above the grid's nz it means nz); an integer
// in 0..1e9
const MESH_SLABS_DEFAULTS = { layers: 0 };
// quadric (extractMesh / meshFromValues): threshold (eigenvalues at or below threshold * the largest are dropped from a cluster's solve, in [0, 1))
const MESH_QUADRIC_DEFAULTS = { threshold: 0.1 };
// occlusion (extractMesh): radius (the first tap's distance, in [2^-64, 2^64]), directions (1, 2, 4, ... 64), taps (1, 2, 4, 8), normalDelta (> 0),
// strength (in [0, 4]) and flags (RM.RENDER_FAST, RM.RENDER_NO_CULL)
const MESH_OCCLUSION_DEFAULTS = { radius: 0.25, directions: 16, taps: 4, normalDelta: 2 ** -10, strength: 1, flags: 0 };
// project (rm_mesh_project): iso (the level to project onto), rounds (1..16), relax (in (0, 1]), tolerance (>= 0), reach (>= 0; 0 = no limit),
// normalDelta (> 0) and flags
const MESH_PROJECT_DEFAULTS = { iso: 0, rounds: 4, relax: 1, tolerance: 0, reach: 0, normalDelta: 2 ** -10, flags: 0 };
// deviation (rm_mesh_deviation): iso (the level the mesh stands for), order (n = 1, 2, 4 or 8: n * n samples per triangle), tolerance (>= 0: a
// triangle whose largest |distance - iso| exceeds it counts as over) and flags
const MESH_DEVIATION_DEFAULTS = { iso: 0, order: 4, tolerance: 0, flags: 0 };
// refine (rm_mesh_refine): iso (the level the mesh stands for), tolerance (>= 0: an edge is split iff its midpoint's |distance - iso| exceeds it),
// minEdge (>= 0: ... and its length exceeds it), rounds (1..8), maxTriangles (a round that would give more is not applied; 0 = the kernels' own
// limit) and flags
const MESH_REFINE_DEFAULTS = { iso: 0, tolerance: 0, minEdge: 0, rounds: 1, maxTriangles: 0, flags: 0 };
// The checks' predicates as [holds(value, block), text]; `32`: the value must also hold as the float32 the addon stores.
const toFlag = (v) => v === true || v === 1 ? 1 : v === false || v === 0 ? 0 : -1;
const finite32 = (text) => [(v) => finite(v) && finite(Math.fround(v)), text];
const within32 = (holds, interval) => [(v) => finite(v) && holds(Math.fround(v)), "must be finite and in " + interval];
const POSITIVE32 = [(v) => POSITIVE[0](v) && POSITIVE[0](Math.fround(v)), POSITIVE[1]];
const NOT_NEGATIVE32 = [(v) => finite(v) && finite(Math.fround(v)) && v >= 0, "must be finite and >= 0"];
const BELOW_ONE32 = within32((f) => f >= 0 && f < 1, "[0, 1)");
const COUNT = integerIn(0, 1e9, "1e9");
const oneOf = (set, text) => [(v) => set.includes(v), text];
const RENDER_FLAGS = [(v) => Number.isInteger(v) && (v & ~(RM.RENDER_FAST | RM.RENDER_NO_CULL)) === 0, "must be 0, RM.RENDER_FAST, RM.RENDER_NO_CULL or both"];
// One row per block for meshBlock: the label its messages carry, the defaults, the fields true / false may set (0 | 1 in the result), and the
// library's own checks in the library's order as [what the message names, [holds, text]].
const MESH_BLOCKS = {
  params: { label: "", defaults: MESH_DEFAULTS, flags: ["normals", "colours"],
            checks: [["iso", finite32("must be a finite number")], ["normals and colours", [(v, p) => p.normals >= 0 && p.colours >= 0, "must be true or false"]],
                     ["normalDelta", [(v, p) => !p.normals || POSITIVE[0](v), POSITIVE[1]]], ["flags", RENDER_FLAGS]] },
  sharp: { label: "sharp", defaults: MESH_SHARP_DEFAULTS, checks: [["refine", integerIn(0, 16)], ["normalDelta", POSITIVE32], ["threshold", BELOW_ONE32]] },
  keep: { label: "keep", defaults: MESH_KEEP_DEFAULTS, checks: [["minTriangles", COUNT], ["largest", COUNT]] },
  slabs: { label: "slabs", defaults: MESH_SLABS_DEFAULTS, checks: [["layers", COUNT]] },
  quadric: { label: "quadric", defaults: MESH_QUADRIC_DEFAULTS, checks: [["threshold", BELOW_ONE32]] },
  occlusion: { label: "occlusion", defaults: MESH_OCCLUSION_DEFAULTS,
               checks: [["radius", within32((f) => f >= 2 ** -64 && f <= 2 ** 64, "[2^-64, 2^64]")], ["directions", oneOf([1, 2, 4, 8, 16, 32, 64], "must be one of 1, 2, 4, 8, 16, 32, 64")],
                        ["taps", oneOf([1, 2, 4, 8], "must be one of 1, 2, 4, 8")], ["normalDelta", POSITIVE32], ["strength", within32((f) => f >= 0 && f <= 4, "[0, 4]")],
                        ["flags", RENDER_FLAGS]] },
  project: { label: "project", defaults: MESH_PROJECT_DEFAULTS,
             checks: [["iso", finite32("must be finite")], ["rounds", integerIn(1, 16)], ["relax", within32((f) => f > 0 && f <= 1, "(0, 1]")], ["tolerance", NOT_NEGATIVE32],
                      ["reach", NOT_NEGATIVE32], ["normalDelta", POSITIVE32], ["flags", RENDER_FLAGS]] },
  deviation: { label: "deviation", defaults: MESH_DEVIATION_DEFAULTS,
               checks: [["iso", finite32("must be finite")], ["order", oneOf([1, 2, 4, 8], "must be 1, 2, 4 or 8")], ["tolerance", NOT_NEGATIVE32], ["flags", RENDER_FLAGS]] },
  refine: { label: "refine", defaults: MESH_REFINE_DEFAULTS,
            checks: [["iso", finite32("must be finite")], ["tolerance", NOT_NEGATIVE32], ["minEdge", NOT_NEGATIVE32], ["rounds", integerIn(1, 8)],
                     ["maxTriangles", integerIn(0, Number.MAX_SAFE_INTEGER, "2^53 - 1")], ["flags", RENDER_FLAGS]] },
};
function meshBlock({ label, defaults, flags = [], checks }, opts) {
  const of = label && label + " ", p = { ...defaults };
  if (opts !== undefined && opts !== null) {
    if (typeof opts !== "object") throw new TypeError("mesh: expected an object of " + of + "parameters");
    for (const [k, v] of Object.entries(opts)) {
      if (!(k in defaults)) throw new TypeError("mesh: unknown " + of + "parameter " + k);
      p[k] = v;
    }
  }
  for (const k of flags) p[k] = toFlag(p[k]);
  for (const [k, [holds, text]] of checks) if (!holds(p[k], p)) throw new RangeError("mesh: " + of + k + " " + text);
  return p;
}
function meshParams(opts) { return meshBlock(MESH_BLOCKS.params, opts); }
function meshSharp(opts) { return meshBlock(MESH_BLOCKS.sharp, opts); }
function meshKeep(opts) { return meshBlock(MESH_BLOCKS.keep, opts); }
function meshSlabs(opts) { return meshBlock(MESH_BLOCKS.slabs, opts); }
function meshQuadric(opts) { return meshBlock(MESH_BLOCKS.quadric, opts); }
function meshOcclusion(opts) { return meshBlock(MESH_BLOCKS.occlusion, opts); }
function meshProject(opts) { return meshBlock(MESH_BLOCKS.project, opts); }
function meshDeviation(opts) { return meshBlock(MESH_BLOCKS.deviation, opts); }
function meshRefine(opts) { return meshBlock(MESH_BLOCKS.refine, opts); }

// the simplify block of extractMesh / meshFromValues (include/hip_raymarch.h RmMeshSimplify and the RmGrid of clusters): an object with grid (a
// meshGrid: one output vertex per occupied cell; it need not be related to the sampling grid) and, optionally, keepDuplicates (keep the triangles
// that repeat an earlier one); checked as the library checks them; returns { grid, keepDuplicates: 0 | 1 }
const MESH_SIMPLIFY_DEFAULTS = { keepDuplicates: 0 };
function meshSimplify(opts) {
  if (opts === undefined || opts === null || typeof opts !== "object") throw new TypeError("mesh: expected an object of simplify parameters");
  for (const k of Object.keys(opts))
    if (k !== "grid" && !(k in MESH_SIMPLIFY_DEFAULTS)) throw new TypeError("mesh: unknown simplify parameter " + k);
  const g = opts.grid;
  if (g === undefined || g === null || typeof g !== "object") throw new TypeError("mesh: simplify needs a grid { lo, hi, n }");
  const flag = toFlag("keepDuplicates" in opts ? opts.keepDuplicates : MESH_SIMPLIFY_DEFAULTS.keepDuplicates);
  if (flag < 0) throw new RangeError("mesh: simplify keepDuplicates must be true or false");
  return { grid: meshGrid(g.lo, g.hi, g.n), keepDuplicates: flag };
}

// the reach extractMesh(..., project) takes when none is given: half the smallest cell side of the grid, 0.5f * min h[a] with h in fp32 by RmGrid's rule
function meshProjectReach(grid) {
  let least = Infinity;
  for (let a = 0; a < 3; a++) least = Math.min(least, Math.fround(Math.fround(Math.fround(grid.hi[a]) - Math.fround(grid.lo[a])) / Math.fround(grid.n[a])));
  return Math.fround(0.5 * least);
}

// the tolerance extractMesh(..., refine) takes when none is given: 1/64 of the smallest cell side of the grid, 2^-6 * min h[a] with h in fp32 by RmGrid's
// rule -- the sagitta of a one-cell edge on a surface whose radius of curvature is 8 cells.  A default, not a bar
function meshRefineTolerance(grid) {
  let least = Infinity;
  for (let a = 0; a < 3; a++) least = Math.min(least, Math.fround(Math.fround(Math.fround(grid.hi[a]) - Math.fround(grid.lo[a])) / Math.fround(grid.n[a])));
  return Math.fround(2 ** -6 * least);
}

// Every option of extractMesh / meshFromValues as the addon takes it, each normalised once: a block that is undefined / null is null, true is the
// block's defaults, slabs as a number is { layers }; project and deviation take true as {} and get the extraction's iso (project also the reach
// of the grid the mesh lies on) where theirs is not given; components and measures are booleans.  When several options are wrong, the first in
// this order speaks.
function meshOptions(grid, opts, given) {
  const absent = (v) => v === undefined || v === null;
  const block = (make, v) => absent(v) ? null : make(v === true ? undefined : v);
  const scenePass = (make, label, v, filled) => {
    if (absent(v)) return null;
    const asked = v === true ? {} : v;
    if (typeof asked !== "object") throw new TypeError("mesh: expected true or an object of " + label + " parameters");
    return make({ ...filled(), ...asked });
  };
  const o = { components: !!given.components, measures: !!given.measures };
  o.quadric = block(meshQuadric, given.quadric);
  if (o.quadric !== null && absent(given.simplify)) throw new TypeError("mesh: quadric places the vertices of a simplification: give simplify as well");
  o.params = meshParams(opts);
  o.simplify = absent(given.simplify) ? null : meshSimplify(given.simplify);
  o.deviation = scenePass(meshDeviation, "deviation", given.deviation, () => ({ iso: o.params.iso }));
  o.project = scenePass(meshProject, "project", given.project, () => ({ iso: o.params.iso, reach: meshProjectReach(o.simplify !== null ? o.simplify.grid : grid) }));
  o.occlusion = block(meshOcclusion, given.occlusion);
  o.sharp = block(meshSharp, given.sharp);
  o.keep = block(meshKeep, given.keep);
  o.slabs = block(meshSlabs, typeof given.slabs === "number" ? { layers: given.slabs } : given.slabs);
  if (o.slabs === null && grid && grid.slabs) throw new TypeError("mesh: a grid made with slabs: true is extracted in slabs: give slabs as well");
  // refine: its block, and with it the projection inside its rounds -- the caller's project block, or the defaults filled as that one is
  const lies = o.simplify !== null ? o.simplify.grid : grid;
  const refine = scenePass(meshRefine, "refine", given.refine, () => ({ iso: o.params.iso, tolerance: meshRefineTolerance(lies) }));
  o.refine = refine === null ? null : { ...refine, project: o.project !== null ? o.project : meshProject({ iso: o.params.iso, reach: meshProjectReach(lies) }) };
  return o;
}
// The addon's argument list of a mesh call, cut as the addon's optional arguments allow: the trailing entries that are null or false are
// dropped, never below the `fixed` leading ones; the components flag (behind `keepAt`) travels with its keep block.
function meshArguments(args, fixed, keepAt) {
  let n = args.length;
  while (n > fixed && (args[n - 1] === null || args[n - 1] === false)) n--;
  return args.slice(0, n === keepAt + 1 ? n + 1 : n);
}

// binary little-endian PLY of { positions, triangles, normals?, colours?, occlusion? }: x y z, then nx ny nz, then uchar red green blue
// (floor(clamp(c, 0, 1) * 255 + 0.5), NaN as 0), then float quality (the occlusion); faces as a uchar count and uint indices -- the bytes the
// Python host writes
// Binary STL of { positions, triangles }: 80 header bytes (`hip_raymarch mesh`, zero padded), uint32 T, then per triangle the facet normal, p0, p1,
// p2 as little-endian float32 and a uint16 0.  The normal in double from the float32 coordinates, every operation rounded on its own: e1 = p1 - p0,
// e2 = p2 - p0, c = e1 x e2, len = sqrt((cx cx + cy cy) + cz cz), c / len rounded to float32; (0, 0, 0) where len is not > 0 or not finite -- the
// bytes the Python host's mesh.encode_stl writes
function encodeStl(mesh) {
  const p = mesh.positions, t = mesh.triangles, T = t.length / 3;
  const out = Buffer.alloc(84 + 50 * T);
  out.write("hip_raymarch mesh", 0, "ascii");
  out.writeUInt32LE(T, 80);
  let at = 84;
  for (let i = 0; i < T; i++) {
    const a = 3 * t[3 * i], b = 3 * t[3 * i + 1], c = 3 * t[3 * i + 2];
    if (a + 2 >= p.length || b + 2 >= p.length || c + 2 >= p.length) throw new RangeError("encodeStl: a triangle names a vertex beyond the positions");
    const e1x = p[b] - p[a], e1y = p[b + 1] - p[a + 1], e1z = p[b + 2] - p[a + 2];
    const e2x = p[c] - p[a], e2y = p[c + 1] - p[a + 1], e2z = p[c + 2] - p[a + 2];
    const cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const len = Math.sqrt((cx * cx + cy * cy) + cz * cz), good = len > 0 && Number.isFinite(len);
    out.writeFloatLE(good ? cx / len : 0, at); out.writeFloatLE(good ? cy / len : 0, at + 4); out.writeFloatLE(good ? cz / len : 0, at + 8);
    at += 12;
    for (const v of [a, b, c]) for (let k = 0; k < 3; k++, at += 4) out.writeFloatLE(p[v + k], at);
    at += 2;  // (the attribute count: 0)
  }
  return out;
}

function encodePly(mesh) {
  const V = mesh.positions.length / 3, T = mesh.triangles.length / 3, nrm = mesh.normals || null, col = mesh.colours || null, occ = mesh.occlusion || null;
  const header = ["ply", "format binary_little_endian 1.0", "comment hip_raymarch mesh", "element vertex " + V, "property float x", "property float y", "property float z"];
  if (nrm) header.push("property float nx", "property float ny", "property float nz");
  if (col) header.push("property uchar red", "property uchar green", "property uchar blue");
  if (occ) header.push("property float quality");
  header.push("element face " + T, "property list uchar uint vertex_indices", "end_header");
  const head = Buffer.from(header.join("\n") + "\n", "ascii"), stride = 12 + (nrm ? 12 : 0) + (col ? 3 : 0) + (occ ? 4 : 0);
  const out = Buffer.alloc(head.length + V * stride + T * 13);
  head.copy(out, 0);
  let at = head.length;
  const byte = (c) => { const x = Number.isNaN(c) ? 0 : Math.min(Math.max(c, 0), 1); return Math.floor(x * 255 + 0.5); };
  for (let v = 0; v < V; v++) {
    for (let k = 0; k < 3; k++) { out.writeFloatLE(mesh.positions[3 * v + k], at); at += 4; }
    if (nrm) for (let k = 0; k < 3; k++) { out.writeFloatLE(nrm[3 * v + k], at); at += 4; }
    if (col) for (let k = 0; k < 3; k++) out[at++] = byte(col[3 * v + k]);
    if (occ) { out.writeFloatLE(occ[v], at); at += 4; }
  }
  for (let t = 0; t < T; t++) {
    out[at++] = 3;
    for (let k = 0; k < 3; k++) { out.writeUInt32LE(mesh.triangles[3 * t + k], at); at += 4; }
  }
  return out;
}

// ---- PNG capture (index.tsx:470-476 canvas.toDataURL): RGBA8, filter 0, rows flipped to top-down ----
const zlib = require("zlib");
const CRC_TABLE = (() => { const t = new Uint32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = c & 1 ? 0xedb88320 ^ (c >>> 1) : c >>> 1; t[n] = c >>> 0; } return t; })();
function crc32(buf) { let c = 0xffffffff; for (let i = 0; i < buf.length; i++) c = CRC_TABLE[(c ^ buf[i]) & 0xff] ^ (c >>> 8); return (c ^ 0xffffffff) >>> 0; }
function pngChunk(tag, data) {
  const out = Buffer.alloc(12 + data.length);
  out.writeUInt32BE(data.length, 0); out.write(tag, 4, "ascii"); data.copy(out, 8);
  out.writeUInt32BE(crc32(out.slice(4, 8 + data.length)), 8 + data.length);
  return out;
}
function encodePng(rgba, width, height, bottomUp = true) {
  if (rgba.length !== width * height * 4) throw new RangeError("encodePng: rgba must hold width * height * 4 bytes");
  const raw = Buffer.alloc(height * (1 + width * 4));
  for (let y = 0; y < height; y++) {
    const src = (bottomUp ? height - 1 - y : y) * width * 4;
    raw[y * (1 + width * 4)] = 0;
    Buffer.from(rgba.buffer, rgba.byteOffset + src, width * 4).copy(raw, y * (1 + width * 4) + 1);
  }
  const ihdr = Buffer.alloc(13);
  ihdr.writeUInt32BE(width, 0); ihdr.writeUInt32BE(height, 4); ihdr[8] = 8; ihdr[9] = 6;
  return Buffer.concat([Buffer.from([0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a]), pngChunk("IHDR", ihdr), pngChunk("IDAT", zlib.deflateSync(raw)), pngChunk("IEND", Buffer.alloc(0))]);
}

module.exports = { RM, addon, encodePng, Scene, CsgScene, Mandelbulb, singleSphere, DEFAULT_MATERIAL, halton, resetHalton, uniformsFromSchema, packUniforms,
                   tileRect, RenderJobContext, ShardedRenderJobContext, doRenderJob, U_OFFSET, DENOISE_DEFAULTS, denoiseParams,
                   DENOISE_VARIANCE_DEFAULTS, denoiseVarianceParams, DESPECKLE_DEFAULTS, despeckleParams, DISPLAY_DEFAULTS, AUTO_EXPOSURE_DEFAULTS,
                   displayParams, statsExposure, statsPercentile, MESH_DEFAULTS, meshGrid, meshParams, MESH_SHARP_DEFAULTS, meshSharp, MESH_KEEP_DEFAULTS, meshKeep, MESH_SLABS_DEFAULTS, meshSlabs,
                   MESH_SIMPLIFY_DEFAULTS, meshSimplify, MESH_QUADRIC_DEFAULTS, meshQuadric, MESH_OCCLUSION_DEFAULTS, meshOcclusion, MESH_PROJECT_DEFAULTS, meshProject, meshProjectReach, MESH_DEVIATION_DEFAULTS, meshDeviation, MESH_REFINE_DEFAULTS, meshRefine, meshRefineTolerance, encodePly, encodeStl };
