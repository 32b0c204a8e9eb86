// Typings of the JS host (index.js).  The job description is the reference's
// RenderJobSchema (client/src/renderer/RenderJobSchema.tsx:17-86) plus `sdfScene`.
export type Vec3 = [number, number, number];
export type UniformData = { type: "f" | "i" | "ui"; count: 1 | 2 | 3 | 4; data: number[] };
export type RenderJobLight =
  | { type: "point"; position: Vec3; color: Vec3; size: number }
  | { type: "sun"; direction: Vec3; color: Vec3 };
export interface Material {
  diffuse: Vec3; diffuse_cutoff: number; specular: Vec3; specular_cutoff: number; roughness: number; subsurface: number;
  subsurface_color: Vec3; ior: number; sky_color: Vec3; sky_floor: number; sky_scale: number; sky_radius: number; sky_axis: 0 | 1 | 2;
}
/** material values a shape of a composed scene can have of its own (RmSurface); missing ones = the reference defaults */
export interface Surface { diffuse?: Vec3; specular?: Vec3; roughness?: number; subsurface?: number; subsurface_color?: Vec3; ior?: number; }
export class Scene { kind: number; params: number[]; material: Material; key(): string; }
export class CsgScene extends Scene {
  constructor(material?: Partial<Material>);
  union(): this; smoothUnion(k: number): this; subtract(): this; intersect(): this; smoothSubtract(k: number): this; smoothIntersect(k: number): this;
  /** ABI 8: a ring, a capped cylinder (axis y) and a half space (unit normal) about `center` / through `point` */
  torus(center: Vec3, majorRadius: number, minorRadius: number, surface?: Surface): this; cylinder(center: Vec3, radius: number, halfHeight: number, surface?: Surface): this;
  plane(point: Vec3, normal: Vec3, surface?: Surface): this;
  /** `surface`: the material functions then depend on the position -- at a point, the values of the nearest shape */
  sphere(center: Vec3, radius: number, surface?: Surface): this; box(center: Vec3, halfExtents: Vec3, surface?: Surface): this;
  /** domain operators: transform the point the FOLLOWING primitives are evaluated at (sphere-grid.glsl's repeat; one level of tree.glsl's fold) */
  repeat(period: Vec3): this; fold(scale: number, offset: Vec3, angles?: Vec3): this;
  /** a shape whose distance term is another scene kind's estimator at p - center (RM_PRIM_KIND): a Mandelbulb cut by a box is table data */
  shape(scene: Scene, center?: Vec3, surface?: Surface): this;
  glsl(): string;
}
export class Mandelbulb extends Scene { constructor(power?: number, iterations?: number, bailout?: number, material?: Partial<Material>); }
export function singleSphere(center?: Vec3, radius?: number, material?: Partial<Material>): CsgScene;
export type RenderJobSchema = {
  reflectionIterationCounts: number[];
  normalDelta: number;
  sdfShaderSource: string;
  sdfScene: Scene;
  customShaderParameters: { [key: string]: UniformData };
  fogDensity: number;
  time: number;
  timeDelta: number;
  dof: { amount: number; distance: number; showFocusedArea: boolean };
  camera: {
    position: Vec3; motion: Vec3; rotation: ArrayLike<number>;
    mode: { type: "perspective"; fov: number } | { type: "orthographic"; size: number } | { type: "panoramic"; angleX: number; angleY: number };
  };
  render: {
    samplesPerPixel: number; exposure: number; subdivisions: number; width: number; height: number; frameid: number;
    blendWithPreviousFrameFactor: number; sampleYieldInterval: number; blendMode: "additive" | "mix"; renderMode: "full" | "preview";
  };
  lights: RenderJobLight[];
};
export type RenderJobFramebufferInfo = {
  width: number; height: number; frameid: number; download(plane?: 0 | 1 | 2): Float32Array;
  /** display.frag on the GPU: RGBA8, row 0 = bottom; `denoise` presents the denoised colour (rm_present_denoised), or with
   *  "variance" / { mode: "variance", ... } the variance-guided filter's (rm_present_denoised_variance; needs { moments: true });
   *  `despeckle` runs the firefly filter ahead of either (rm_present_filtered); without it the calls are the ones above */
  present(samples: number, opts?: FrameOptions): Uint8Array;
  /** the blurred, exposed frame as floats (rm_present_linear): (e.r, e.g, e.b, 1) per pixel, row 0 = bottom; the tone is checked, not applied */
  linear(samples: number, opts?: FrameOptions): Float32Array;
  /** the luminance statistics (rm_frame_stats) of the colour plane, or with `despeckle` / `denoise` of the chain's result */
  stats(samples: number, opts?: { denoise?: DenoiseOption; despeckle?: DespeckleOption }): FrameStats;
  /** the colour plane after the chain despeckle -> denoise (rm_filter): colour-plane units, row 0 = bottom */
  filter(samples: number, opts?: { denoise?: DenoiseOption; despeckle?: DespeckleOption }): Float32Array;
  /** the colour plane after the variance-guided filter (rm_denoise_variance; needs { moments: true }) */
  denoiseVariance(samples: number, params?: true | "variance" | DenoiseVarianceParams): Float32Array;
  /** the colour plane after the G-buffer-guided a-trous filter (rm_denoise): colour-plane units, row 0 = bottom */
  denoise(samples: number, params?: true | DenoiseParams): Float32Array;
  /** canvas.toDataURL("image/png") of the presented frame (index.tsx:470-476) */
  toDataURL(samples: number, opts?: FrameOptions): string;
};
/** `display`: the display transform behind the blur (rm_present_display); without it present's calls are the ones above */
export type FrameOptions = { denoise?: DenoiseOption; despeckle?: DespeckleOption; display?: DisplayOption };
/** RmDisplay (include/hip_raymarch.h): e = v * gain, then the tone operator ("clip": none; "reinhard" with `white`; "aces"), then pow and RGBA8 */
export type DisplayParams = { gain?: number; tone?: "clip" | "reinhard" | "aces"; white?: number };
/** "auto" / { auto, tone, white }: the gain is statsExposure of the same chain's stats (auto: true or its parameters) */
export type DisplayOption = DisplayParams | "auto" | { auto: true | AutoExposureParams; tone?: "clip" | "reinhard" | "aces"; white?: number };
export const DISPLAY_DEFAULTS: Required<DisplayParams>;
/** checked as the library checks them; `tone` comes back as its RM_TONE_* number */
export function displayParams(params?: true | DisplayParams | null): { gain: number; tone: number; white: number };
/** RmFrameStats: 512 bins, 16 per octave over [2^-20, 2^12), the classes outside them, min / max over the finite luminances */
export type FrameStats = { pixels: number; below: number; above: number; nonFinite: number; min: number; max: number; hist: Float64Array };
/** RmAutoExposure: fields left out take AUTO_EXPOSURE_DEFAULTS' values */
export type AutoExposureParams = { key?: number; low?: number; high?: number; min_gain?: number; max_gain?: number };
export const AUTO_EXPOSURE_DEFAULTS: Required<AutoExposureParams>;
/** rm_stats_exposure: the gain that brings the log-average luminance between the `low` and `high` percentiles to `key` */
export function statsExposure(stats: FrameStats, opts?: AutoExposureParams | null): number;
/** rm_stats_percentile: the upper edge of the bin that holds the ceil(q N)-th smallest binned pixel; 0 when nothing is binned */
export function statsPercentile(stats: FrameStats, q: number): number;
/** RmDespeckle (include/hip_raymarch.h): the firefly filter; fields left out take DESPECKLE_DEFAULTS' values */
export type DespeckleParams = { radius?: 1 | 2; rank?: 0 | 1 | 2 | 3; gain?: number; floor?: number; repair?: number | boolean };
export type DespeckleOption = true | DespeckleParams;
export const DESPECKLE_DEFAULTS: { radius: number; rank: number; gain: number; floor: number; repair: number };
export function despeckleParams(params?: true | DespeckleParams | null): { radius: number; rank: number; gain: number; floor: number; repair: number };
/** RmDenoiseVariance (include/hip_raymarch.h): fields left out take DENOISE_VARIANCE_DEFAULTS' values */
export type DenoiseVarianceParams = { iterations?: number; sigma_luminance?: number; sigma_normal?: number; sigma_depth?: number };
export type DenoiseOption = true | DenoiseParams | (DenoiseParams & { mode: "atrous" }) | "variance" | (DenoiseVarianceParams & { mode: "variance" });
export const DENOISE_VARIANCE_DEFAULTS: Required<DenoiseVarianceParams>;
export function denoiseVarianceParams(params?: true | "variance" | (DenoiseVarianceParams & { mode?: "variance" }) | null): Required<DenoiseVarianceParams>;
/** RmDenoise (include/hip_raymarch.h): fields left out take DENOISE_DEFAULTS' values */
export type DenoiseParams = { iterations?: number; sigma_color?: number; sigma_normal?: number; sigma_depth?: number };
export const DENOISE_DEFAULTS: Required<DenoiseParams>;
export function denoiseParams(params?: true | DenoiseParams | null): Required<DenoiseParams>;
export type ShaderError = { type: "vertex" | "fragment" | "program"; infoLog: string };
/** The G-buffer format of a context's framebuffers: "f32" (default) or "f16", the reference's RGBA16F normal + DoF radius and
 *  albedo + depth planes (accumulated in half precision; the colour plane stays fp32). */
export type GBufferFormat = "f32" | "f16";
export class RenderJobContext {
  constructor(device?: number, flags?: number);
  /** moments: every framebuffer also keeps the luminance moments plane (RM_FB_MOMENTS) the variance-guided denoiser reads */
  constructor(options: { device?: number; flags?: number; gbuffer?: GBufferFormat; moments?: boolean });
  readonly gbuffer: GBufferFormat;
  readonly moments: boolean;
  fboCreate(width: number, height: number, frameid: number): RenderJobFramebufferInfo;
  fboDelete(width: number, height: number, frameid: number): void;
  /** the scene's distance at every corner of the grid, x fastest (rm_sdf_grid): rm_probe's RM_PROBE_SDF at the corners, bit for bit */
  sdfGrid(scene: Scene, grid: MeshGrid, flags?: number): Float32Array;
  /** the level set `iso` of the scene on the grid as triangles (rm_mesh_extract: sampled and meshed with surface nets on the GPU) */
  extractMesh(scene: Scene, grid: MeshGrid, params?: MeshParams | null): Mesh;
  /** with `sharp` (true = the defaults): rm_mesh_extract_sharp, the same triangles with every vertex at its cell's QEF minimiser, so hard edges and corners stay sharp */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null): Mesh;
  /** with `keep` (true = the defaults, which drop unreferenced vertices): the mesh's connected components filtered on the GPU before anything is copied (rm_mesh_filter); `components`: the result carries labels and componentSizes (rm_mesh_components) */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components?: boolean): Mesh;
  /** with `simplify`: the vertices of every cell of a second grid of clusters merged into one on the GPU (rm_mesh_simplify) before `keep` and `components` are applied, so one filter also removes the vertices the clustering left without triangles; the result's cells index the cluster grid */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null): Mesh;
  /** with `quadric` (true = the defaults; only with `simplify`): every cluster's vertex at the minimiser of the plane quadrics of the source triangles that touch the cluster instead of at the mean of its vertices (rm_mesh_simplify_quadric), which keeps the edges and corners inside a cluster; only the positions differ */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify, quadric: MeshQuadric | true | null): Mesh;
  /** with `occlusion` (true = the defaults): the scene's ambient occlusion at the vertices of the mesh that is returned, behind simplify, keep and components (rm_mesh_occlusion), as Mesh.occlusion; timings gains a fourth entry, its milliseconds */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null | undefined, quadric: MeshQuadric | true | null | undefined, occlusion: MeshOcclusion | true | null): Mesh;
  /** with `measures`: the mesh that is returned is measured on the GPU behind simplify and keep, before anything is copied (rm_mesh_measure), as Mesh.measures */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null | undefined, quadric: MeshQuadric | true | null | undefined, occlusion: MeshOcclusion | true | null | undefined, measures: boolean): Mesh;
  /** with `slabs` (true = the defaults, a number = the cell layers per slab): rm_mesh_extract_slabs / rm_mesh_extract_sharp_slabs, the same mesh byte for byte, made from one window of z layers at a time; it also takes a meshGrid(lo, hi, n, { slabs: true }) beyond 2^28 corners */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null | undefined, quadric: MeshQuadric | true | null | undefined, occlusion: MeshOcclusion | true | null | undefined, measures: boolean | undefined, slabs: MeshSlabs | number | true | null): Mesh;
  /** project: the vertices of the returned mesh are moved onto the scene's level set (rm_mesh_project) behind simplify, quadric and keep, before components, occlusion and measures; iso defaults to params.iso, reach to meshProjectReach of the grid the mesh lies on; the result carries `projection` and `residual` */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null | undefined, quadric: MeshQuadric | true | null | undefined, occlusion: MeshOcclusion | true | null | undefined, measures: boolean | undefined, slabs: MeshSlabs | number | true | null | undefined, project: MeshProject | true | null): Mesh;
  /** deviation: how far the triangles of the returned mesh lie off the scene's level set (rm_mesh_deviation), measured behind every other stage, project included; iso defaults to params.iso; the result carries `deviation` and `triangleDeviation` */
  /** refine: behind project and before measures, components, occlusion and deviation, the edges whose midpoint lies further than `tolerance` off the scene's level set are split for `rounds` rounds (rm_mesh_refine), every round's mesh projected with the project block or its defaults; iso defaults to params.iso, tolerance to meshRefineTolerance of the grid the mesh lies on; the criterion looks at edge midpoints only, `deviation` remains the judge; the result carries `refinement` */
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null | undefined, quadric: MeshQuadric | true | null | undefined, occlusion: MeshOcclusion | true | null | undefined, measures: boolean | undefined, slabs: MeshSlabs | number | true | null | undefined, project: MeshProject | true | null | undefined, deviation: MeshDeviation | true | null): Mesh;
  extractMesh(scene: Scene, grid: MeshGrid, params: MeshParams | null | undefined, sharp: MeshSharp | true | null | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null | undefined, quadric: MeshQuadric | true | null | undefined, occlusion: MeshOcclusion | true | null | undefined, measures: boolean | undefined, slabs: MeshSlabs | number | true | null | undefined, project: MeshProject | true | null | undefined, deviation: MeshDeviation | true | null | undefined, refine: MeshRefine | true | null): Mesh;
  /** the mesher alone on the caller's field (rm_mesh_from_values); keep, components and simplify as in extractMesh */
  meshFromValues(grid: MeshGrid, values: Float32Array, iso?: number, keep?: MeshKeep | true | null, components?: boolean, simplify?: MeshSimplify | null): Mesh;
  /** quadric as in extractMesh */
  meshFromValues(grid: MeshGrid, values: Float32Array, iso: number | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify, quadric: MeshQuadric | true | null): Mesh;
  /** measures as in extractMesh */
  meshFromValues(grid: MeshGrid, values: Float32Array, iso: number | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null | undefined, quadric: MeshQuadric | true | null | undefined, measures: boolean): Mesh;
  /** slabs as in extractMesh (rm_mesh_from_values_slabs) */
  meshFromValues(grid: MeshGrid, values: Float32Array, iso: number | undefined, keep: MeshKeep | true | null | undefined, components: boolean | undefined, simplify: MeshSimplify | null | undefined, quadric: MeshQuadric | true | null | undefined, measures: boolean | undefined, slabs: MeshSlabs | number | true | null): Mesh;
  close(): void;
}
/** A frame sharded over several GPUs by this one process: a native context per device, each holding one part of the frame's
 *  8-row stripes; `present(samples)` of its framebuffer set assembles the canvas on the first GPU (rm_present_sharded). */
export type ShardedFramebufferInfo = {
  width: number; height: number; frameid: number; sharded: true; dof: boolean; rows(): number[];
  /** throws when asked to denoise or to despeckle (the filters read rows other GPUs hold) or for a display transform (not carried yet) */
  present(samples: number, dof?: boolean, opts?: { denoise?: undefined; despeckle?: undefined; display?: undefined }): Uint8Array; toDataURL(samples: number): string;
  /** the present in two halves (rm_present_sharded_start / _finish): the frame travels while the next samples render; one at a time */
  startPresent(samples: number, dof?: boolean): void; finishPresent(): Uint8Array; pendingPresent: boolean;
};
export class ShardedRenderJobContext {
  constructor(devices?: number[], flags?: number, samplesInFlight?: number);
  constructor(options: { devices?: number[]; flags?: number; samplesInFlight?: number; gbuffer?: GBufferFormat });
  readonly gbuffer: GBufferFormat;
  fboCreate(width: number, height: number, frameid: number): ShardedFramebufferInfo;
  fboDelete(width: number, height: number, frameid: number): void;
  close(): void;
}
export type Present = (schema: RenderJobSchema, context: RenderJobContext, framebuffers: RenderJobFramebufferInfo, samplesSoFar: number) => void;
export function doRenderJob(schema: RenderJobSchema, context: RenderJobContext | ShardedRenderJobContext): Promise<
  (present: Present) => Generator<undefined, { success: boolean; why?: ShaderError | { type: "general"; infoLog: string } }, unknown>
>;
export function uniformsFromSchema(schema: RenderJobSchema, randNoise: [number, number]): ArrayBuffer;
export function halton(base: number): Generator<number, never, unknown>;
export function resetHalton(): void;
export function encodePng(rgba: Uint8Array, width: number, height: number, bottomUp?: boolean): Buffer;
export const RM: { [name: string]: number };
/** mesh extraction (include/hip_raymarch.h "mesh extraction"): n = CELLS per axis between the corners lo and hi */
export interface MeshGrid { lo: [number, number, number]; hi: [number, number, number]; n: [number, number, number]; slabs?: true }
export interface MeshParams { iso?: number; normals?: boolean | 0 | 1; normalDelta?: number; colours?: boolean | 0 | 1; flags?: number }
export interface Mesh { positions: Float32Array; normals: Float32Array | null; colours: Float32Array | null; triangles: Uint32Array; cells: Uint32Array; /** ms of sampling, meshing, attributes (rm_mesh_timings); with an occlusion a fourth entry, its probes and taps */ timings: [number, number, number] | [number, number, number, number]; /** only when components were asked for: each vertex's component, and (vertices, triangles) per component */ labels?: Uint32Array; componentSizes?: Uint32Array; /** only when an occlusion was asked for: 1 = open, per vertex (rm_mesh_occlusion) */ occlusion?: Float32Array; /** only when measures were asked for (rm_mesh_measure) */ measures?: MeshMeasures; /** only with `project`: what rm_mesh_project reports, and the distance minus iso at the projected vertices */ projection?: MeshProjection; residual?: Float32Array; /** only with `deviation`: what rm_mesh_deviation reports, and each triangle's largest |distance - iso| over its samples */ deviation?: MeshDeviationReport; triangleDeviation?: Float32Array; /** only with `refine`: what rm_mesh_refine reports */ refinement?: MeshRefinement }
/** what rm_mesh_measure says of a mesh (RmMeshMeasures, include/hip_raymarch.h "measures and edge topology"): the counts as Numbers (all below 2^53), lo / hi of the finite vertices, closed = no boundary and no irregular edge; componentEdges: 4 uint64 per component (edges, boundary, irregular, unbalanced; rm_mesh_measure_components); milliseconds of topology and geometry */
export interface MeshMeasures { vertices: number; triangles: number; usedVertices: number; skippedTriangles: number; unmeasuredTriangles: number; finiteVertices: number; edges: number; boundaryEdges: number; regularEdges: number; irregularEdges: number; unbalancedEdges: number; euler: number; components: number; closedComponents: number; area: number; volume: number; lo: [number, number, number]; hi: [number, number, number]; closed: boolean; componentEdges: BigUint64Array; milliseconds: [number, number] }
export const MESH_DEFAULTS: { iso: number; normals: 0 | 1; normalDelta: number; colours: 0 | 1; flags: number };
export function meshGrid(lo: number[], hi: number[], n: number[]): MeshGrid;
/** with { slabs: true }: without the bound of 2^28 corners -- a grid for extractMesh / meshFromValues with `slabs` */
export function meshGrid(lo: number[], hi: number[], n: number[], opts: { slabs?: boolean } | null): MeshGrid;
export function meshParams(params?: MeshParams | null): { iso: number; normals: 0 | 1; normalDelta: number; colours: 0 | 1; flags: number };
/** the sharp block of extractMesh (RmMeshSharp): bisection rounds per edge crossing (0..16), the step of the normals at the crossings (> 0), the relative eigenvalue below which the QEF is truncated ([0, 1)) */
export interface MeshSharp { refine?: number; normalDelta?: number; threshold?: number }
export const MESH_SHARP_DEFAULTS: { refine: number; normalDelta: number; threshold: number };
export function meshSharp(sharp?: MeshSharp | null): { refine: number; normalDelta: number; threshold: number };
/** the slabs block of extractMesh / meshFromValues (RmMeshSlabs): the cell layers per slab, 0 = chosen by the library; above the grid's nz it means nz */
export interface MeshSlabs { layers?: number }
export const MESH_SLABS_DEFAULTS: { layers: number };
export function meshSlabs(slabs?: MeshSlabs | null): { layers: number };
/** the keep block of extractMesh / meshFromValues (RmMeshKeep): a component passes with at least minTriangles triangles; largest = k > 0 keeps only the k passing components with the most triangles (the lower component index first among equals), 0 keeps every passing one */
export interface MeshKeep { minTriangles?: number; largest?: number }
export const MESH_KEEP_DEFAULTS: { minTriangles: number; largest: number };
export function meshKeep(keep?: MeshKeep | null): { minTriangles: number; largest: number };
/** the simplify block of extractMesh / meshFromValues (RmMeshSimplify and its RmGrid of clusters): one output vertex per occupied cell of `grid`, the mean of the cell's vertices; keepDuplicates keeps the triangles that repeat an earlier one */
export interface MeshSimplify { grid: MeshGrid; keepDuplicates?: boolean | 0 | 1 }
export const MESH_SIMPLIFY_DEFAULTS: { keepDuplicates: 0 | 1 };
export function meshSimplify(simplify: MeshSimplify): { grid: MeshGrid; keepDuplicates: 0 | 1 };
/** the quadric block of extractMesh / meshFromValues (RmMeshQuadric): eigenvalues at or below threshold * the largest are dropped from a cluster's solve, in [0, 1) */
export interface MeshQuadric { threshold?: number }
export const MESH_QUADRIC_DEFAULTS: { threshold: number };
export function meshQuadric(quadric?: MeshQuadric | null): { threshold: number };
/** the occlusion block of extractMesh (RmMeshOcclusion): `directions` (1, 2, 4 ... 64) directions over every vertex, `taps` (1, 2, 4, 8) taps along each, the first at `radius`; ao = 1 - strength * occlusion */
export interface MeshOcclusion { radius?: number; directions?: number; taps?: number; normalDelta?: number; strength?: number; flags?: number }
export const MESH_OCCLUSION_DEFAULTS: { radius: number; directions: number; taps: number; normalDelta: number; strength: number; flags: number };
export function meshOcclusion(occlusion?: MeshOcclusion | null): { radius: number; directions: number; taps: number; normalDelta: number; strength: number; flags: number };
/** the block of rm_mesh_project (RmMeshProject): up to `rounds` (1..16) Newton steps of every vertex onto the level `iso` of the scene, `relax` (in (0, 1]) of each step taken, at most `reach` per axis from where the vertex started (0 = no limit); a vertex within `tolerance` of the level does not move */
export interface MeshProject { iso?: number; rounds?: number; relax?: number; tolerance?: number; reach?: number; normalDelta?: number; flags?: number }
export const MESH_PROJECT_DEFAULTS: Required<MeshProject>;
export function meshProject(project?: MeshProject | null): Required<MeshProject>;
/** the reach extractMesh takes when `project` names none: half the smallest cell side of the grid, in fp32 */
export function meshProjectReach(grid: MeshGrid): number;
/** what rm_mesh_project says of its work (RmMeshProjection): how far off the level set the vertices were and are (|distance - iso|: worst vertex, max, mean, rms), the vertices the reach clamped or that had no usable normal, the triangles whose orientation flipped, the rounds evaluated; milliseconds: the rounds and the normals */
export interface MeshProjection { vertices: number; triangles: number; movedVertices: number; settledBefore: number; settledAfter: number; nonfiniteBefore: number; nonfiniteAfter: number; clampedVertices: number; undirectedVertices: number; flippedTriangles: number; worstBefore: number; worstAfter: number; meanBefore: number; rmsBefore: number; meanAfter: number; rmsAfter: number; maxBefore: number; maxAfter: number; roundsRun: number; milliseconds: number }
/** the block of rm_mesh_deviation (RmMeshDeviation): the scene's distance minus `iso` at order * order (order 1, 2, 4 or 8) fixed samples inside every triangle; a triangle whose largest |distance - iso| exceeds `tolerance` counts as over */
export interface MeshDeviation { iso?: number; order?: number; tolerance?: number; flags?: number }
export const MESH_DEVIATION_DEFAULTS: Required<MeshDeviation>;
export function meshDeviation(deviation?: MeshDeviation | null): Required<MeshDeviation>;
/** the block of rm_mesh_refine (RmMeshRefine): an edge is split iff its midpoint's |distance - iso| exceeds `tolerance` and its length exceeds `minEdge`; `rounds` in 1..8; a round that would give more than `maxTriangles` triangles is not applied (0 = the kernels' own limit) */
export interface MeshRefine { iso?: number; tolerance?: number; minEdge?: number; rounds?: number; maxTriangles?: number; flags?: number }
export const MESH_REFINE_DEFAULTS: Required<MeshRefine>;
export function meshRefine(refine?: MeshRefine | null): Required<MeshRefine>;
/** the tolerance extractMesh(..., refine) takes when none is given: 1/64 of the smallest cell side of `grid`, in fp32 -- a default, not a bar */
export function meshRefineTolerance(grid: MeshGrid): number;
/** what rm_mesh_refine says of its work (RmMeshRefinement): per round evaluated the unique edges, the edges split and the midpoints without a finite distance; maxFirst / maxLast: the largest |distance - iso| over the midpoints of the first / last round; stopped: 0 rounds done, 1 nothing to split, 2 budget; milliseconds: the split rounds, the projections and the normals */
export interface MeshRefinement { verticesBefore: number; trianglesBefore: number; vertices: number; triangles: number; edges: number[]; splitEdges: number[]; nonfiniteMidpoints: number[]; flippedTriangles: number; maxFirst: number; maxLast: number; roundsRun: number; stopped: number; milliseconds: number }
/** what rm_mesh_deviation says of a mesh (RmMeshDeviationReport): one-sided, mesh to surface, at `samples` fixed points per triangle -- a lower bound of the true maximum; area, meanSigned and rms are area-weighted over the evaluated triangles; milliseconds: evaluation and reduction */
export interface MeshDeviationReport { vertices: number; triangles: number; skippedTriangles: number; unevaluatedTriangles: number; nonfiniteSamples: number; overTriangles: number; worstTriangle: number; area: number; overArea: number; meanSigned: number; rms: number; max: number; samples: number; milliseconds: number }
/** binary little-endian PLY (normals, uchar colours and a float `quality` -- the occlusion -- when present): the bytes the Python host's write_ply writes */
/** binary STL of the triangles, facet normals computed in double from the float32 positions: the bytes the Python host's mesh.encode_stl writes */
export function encodeStl(mesh: { positions: Float32Array; triangles: Uint32Array }): Buffer;
export function encodePly(mesh: { positions: Float32Array; triangles: Uint32Array; normals?: Float32Array | null; colours?: Float32Array | null; occlusion?: Float32Array | null }): Buffer;
