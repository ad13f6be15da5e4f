'use strict';
/*
 * main.js -- Node host of the compute pass: the reference's Main()/frame()
 * (src/main.js:7-624) with the browser removed and WebGPU replaced by the
 * HIP library behind the N-API addon.
 *
 *   reference (src/main.js)                       here
 *   8-9    requestAdapter / requestDevice         addon.create(device)
 *   114-393 flatten + pack + createBuffer/unmap   sceneLoader.pack + addon.uploadScene
 *   298-311 zero accumulator, sample = 0          (done by uploadScene / reset)
 *   597-611 per frame: dispatch(1); dispatch(W/8,H/8)   frame(): addon.trace(h, 1)
 *   612-617 blit to the canvas                    readRgba8() / writePPM()   (display only)
 *           (no counterpart)                      denoise(): filtered preview of the same average
 *           queue.writeBuffer(camera / primitives / lights)   setCamera / updatePrimitives + refitAccel / updateLights
 *           (no counterpart)                      transformPrimitives: ranges moved on the device, nothing uploaded
 *           (no counterpart)                      removePrimitives / appendPrimitives: the primitive list edited on the device
 *           (no counterpart)                      queryRays / pick: what caller rays, or the ray under a pixel, hit
 *           (no counterpart)                      radianceRays: the path tracer's radiance along caller rays
 *   620     requestAnimationFrame(frame) forever  run(spp): spp frames, optionally fused
 */
const fs = require('fs');
const path = require('path');
const sceneLoader = require('./sceneLoader');

let addon;
function loadAddon() {
  if (!addon) addon = require(path.join(__dirname, '..', 'addon', 'crt_napi.node')); // throws if not built
  return addon;
}

const ACCEL = { none: 0, brute: 0, bvh2: 1, bvh: 1, lbvh: 2, ploc: 3 };
const QUERY_PLANES = ['hit', 'prim', 'id', 't', 'position', 'normal', 'uv'];
const RADIANCE_PLANES = ['xyz', 'y2', 'rgba8'];

function Main(options = {}) {
  const a = loadAddon();
  const scene = options.scene || sceneLoader.loadScene(options.sceneFile);
  if (options.width) scene.camera = { ...scene.camera, width: options.width, height: options.height || options.width };
  const packed = sceneLoader.pack(scene, options.cie, options.sceneFile ? path.dirname(path.resolve(options.sceneFile)) : undefined);
  const { width, height } = packed;

  const device = a.create(options.device || 0);
  a.uploadScene(device, packed.primitives, packed.lights, packed.spectra, packed.cie, packed.camera);
  a.setPrimitiveIds(device, 0, packed.objectIds); // what renderMattes' source 'object' reports (host only)
  if (options.tile) a.setTile(device, ...options.tile);
  a.buildAccel(device, ACCEL[options.accel || 'bvh2']);

  // one reference frame = { sample++ ; trace } (main.js:598-611)
  const frame = () => a.trace(device, 1);
  const run = (spp, fused = true) => {
    if (fused) a.trace(device, spp); // same result as spp frames (summed in sample order)
    else for (let i = 0; i < spp; i++) frame();
    a.sync(device);
  };

  return {
    width, height, packed, device, frame, run,
    // Promise forms: the job runs on a worker thread, the event loop stays free (the reference's frame() is
    // fire-and-forget too: queue.submit, src/main.js:618-620).  Jobs of one device run in call order; the blocking
    // calls throw ERR_CRT_BUSY while any are pending.
    frameAsync: (n = 1) => a.traceAsync(device, n),
    syncAsync: () => a.syncAsync(device),
    readRgba8Async: () => a.readRgba8Async(device),
    readAccumAsync: () => a.readAccumAsync(device),
    sync: () => a.sync(device),
    reset: () => a.reset(device),
    get sample() { return a.sampleCount(device); },
    readAccum: () => a.readAccum(device),
    readRgba8: () => a.readRgba8(device),
    // denoised preview of the current average (include/crt.h "Denoised preview"): rgba8 of the tile; reads only
    denoise: (opts = {}) => a.denoise(device, opts),
    // ... of the newest COMPLETE frame without finishing what is in flight (crt_denoise_latest): {rgba8, rgb?, sample}, the
    // filtered frame of exactly `sample` samples; Into writes the rgba8 into a (pinned) typed array and returns `sample`
    denoiseLatest: (opts = {}) => a.denoiseLatest(device, opts),
    denoiseLatestInto: (out, opts = {}) => a.denoiseLatestInto(device, out, opts),
    denoiseLatestAsync: (opts = {}) => a.denoiseLatestAsync(device, opts),
    readGbuffer: () => a.readGbuffer(device),
    // feature planes (include/crt.h "Feature planes"): anti-aliased hits, alpha, depth, normal and albedo of the camera
    // rays of n samples (0: the samples the accumulator holds), as typed arrays over the tile; reads only
    renderAovs: (n = 0, planes = ['hits', 'alpha', 'depth', 'normal', 'albedo']) => {
      const [, , tw, th] = a.tile(device), out = {};
      for (const p of planes) {
        if (!['hits', 'alpha', 'depth', 'normal', 'albedo'].includes(p)) throw new TypeError(`renderAovs: unknown plane ${p}`);
        out[p] = p === 'hits' ? new Uint32Array(tw * th) : new Float32Array(tw * th * (p === 'normal' || p === 'albedo' ? 4 : 1));
      }
      a.renderAovs(device, n, out);
      return out;
    },
    // id mattes (include/crt.h "ID mattes"): per pixel the ids its camera rays hit, ranked by how many rays hit each, over
    // n samples (0: the samples the accumulator holds); source 'primitive' | 'object' (the id table) | 'material'; ids and
    // counts are `slots` planes of tw * th, rank 0 first (0xFFFFFFFF / 0: no entry); reads only
    renderMattes: (n = 0, source = 'object', slots = 8, planes = ['ids', 'counts', 'hits', 'overflow']) => {
      const src = ['primitive', 'object', 'material'].indexOf(source);
      if (src < 0) throw new TypeError(`renderMattes: unknown source ${source}`);
      const [, , tw, th] = a.tile(device), out = {};
      for (const p of planes) {
        if (!['ids', 'counts', 'hits', 'overflow'].includes(p)) throw new TypeError(`renderMattes: unknown plane ${p}`);
        out[p] = new Uint32Array(tw * th * (p === 'ids' || p === 'counts' ? slots : 1));
      }
      a.renderMattes(device, n, src, slots, out);
      return out;
    },
    // entries [first, first + ids.length) of the id table source 'object' reports; nothing else changes
    setPrimitiveIds: (first, ids) => a.setPrimitiveIds(device, first, ids instanceof Uint32Array ? ids : Uint32Array.from(ids)),
    // ray queries (include/crt.h "Ray queries"): what caller rays hit -- rays: Float32Array of 8 floats per ray (o, t_max,
    // d, exclude bits; t_max 2139095040 or Infinity = no limit, exclude bits 0xFFFFFFFF = nothing), mode 'closest' | 'any'
    // (which reports `hit` alone) -- as typed arrays of n entries (position, normal: 4 floats each, uv: 2); does not
    // finish or disturb what is in flight
    queryRays: (rays, mode = 'closest', planes = mode === 'any' ? ['hit'] : QUERY_PLANES) => {
      const m = ['closest', 'any'].indexOf(mode);
      if (m < 0) throw new TypeError(`queryRays: unknown mode ${mode}`);
      if (!(rays instanceof Float32Array) || rays.length % 8) throw new TypeError('queryRays: rays must be a Float32Array of 8 floats per ray');
      const n = rays.length / 8, out = {};
      for (const p of planes) {
        if (!QUERY_PLANES.includes(p)) throw new TypeError(`queryRays: unknown plane ${p}`);
        out[p] = ['hit', 'prim', 'id'].includes(p) ? new Uint32Array(n) : new Float32Array(n * (p === 't' ? 1 : p === 'uv' ? 2 : 4));
      }
      a.queryRays(device, rays, m, out);
      return out;
    },
    // how much light arrives along caller rays (include/crt.h "Radiance queries"): rays as for queryRays, keys a
    // Uint32Array of (x, y, first sample, 0) per ray or null (= (i, 0, 1)), nSamples paths per ray summed; returns
    // {xyz: Float32Array(n*4), y2: Float32Array(n), rgba8: Uint8Array(n*4)}, or the planes named.  Blocking for the call
    // alone: work in flight is neither finished nor disturbed.
    radianceRays: (rays, keys = null, nSamples = 1, planes = RADIANCE_PLANES) => {
      if (!(rays instanceof Float32Array) || rays.length % 8) throw new TypeError('radianceRays: rays must be a Float32Array of 8 floats per ray');
      if (keys !== null && (!(keys instanceof Uint32Array) || keys.length !== rays.length / 2)) throw new TypeError('radianceRays: keys must be null or a Uint32Array of 4 per ray');
      if (!Number.isInteger(nSamples) || nSamples < 1 || nSamples > 0xFFFFFFFF) throw new TypeError('radianceRays: nSamples must be an integer from 1 to 2^32 - 1');
      for (const p of planes) if (!RADIANCE_PLANES.includes(p)) throw new TypeError(`radianceRays: unknown plane ${p}`);
      if (!planes.length) throw new TypeError('radianceRays: no plane asked for');
      return a.radianceRays(device, rays, keys, nSamples, planes);
    },
    // what lies under pixel (x, y) of the full image: {prim, id, t, position, normal, uv} of the pixel's camera ray (the
    // G-buffer's), or null where it hits nothing
    pick: (x, y) => {
      const h = a.pick(device, x, y);
      return h.hit ? { prim: h.prim, id: h.id, t: h.t, position: h.position.subarray(0, 3), normal: h.normal.subarray(0, 3), uv: h.uv } : null;
    },
    // scene edits (include/crt.h "Scene edits"): each finishes what is in flight and restarts the accumulation;
    // the reference's queue.writeBuffer of the camera / primitive / light buffer
    setCamera: (camera) => a.setCamera(device, camera),
    updatePrimitives: (first, records) => a.updatePrimitives(device, first, records),
    updateLights: (first, records) => a.updateLights(device, first, records),
    refitAccel: () => a.refitAccel(device),
    // move primitive ranges on the device instead of uploading moved records (include/crt.h crt_transform_primitives):
    // ops = [{first, count, m: 12 numbers (row-major 3x4, rows (R | t)), radiusScale = 1}]; the tree goes stale until
    // refitAccel().  readPrimitives: Uint8Array(count * 80), the records as the device holds them.
    transformPrimitives: (ops) => a.transformPrimitives(device, packTransforms(ops)),
    transformPrimitivesAsync: (ops) => a.transformPrimitivesAsync(device, packTransforms(ops)),
    readPrimitives: (first, count) => a.readPrimitives(device, first, count),
    readPrimitivesAsync: (first, count) => a.readPrimitivesAsync(device, first, count),
    // remove or append primitives on the device instead of uploading the scene again (include/crt.h
    // crt_remove_primitives, crt_append_primitives): ranges = [{first, count}] or [[first, count]]; records = k * 80 bytes,
    // each numbered by its position in the new list; lights = the new light list (m * 80 bytes), or left out / null to
    // keep the list (its primitive indices follow a removal).  With a tree, refitAccel() then rebuilds it.
    removePrimitives: (ranges, lights = null) => a.removePrimitives(device, packRanges(ranges), lights),
    removePrimitivesAsync: (ranges, lights = null) => a.removePrimitivesAsync(device, packRanges(ranges), lights),
    appendPrimitives: (records, lights = null) => a.appendPrimitives(device, records, lights),
    appendPrimitivesAsync: (records, lights = null) => a.appendPrimitivesAsync(device, records, lights),
    // adaptive sampling (include/crt.h "Adaptive sampling"): more samples for the 8x8 tiles that have not converged;
    // returns how many tiles that was (0: done).  readAdaptive: {counts, errors, tilesX, tilesY}
    traceAdaptive: (opts = {}) => a.traceAdaptive(device, opts),
    readAdaptive: () => a.readAdaptive(device),
    // ... judged by the noise denoiseAdaptive leaves instead of the raw pixel error (include/crt.h "Adaptive sampling
    // judged by the filtered preview"): opts = traceAdaptive's plus the filter's {iterations, sigmaVariance, sigmaNormal,
    // sigmaPlane}; readAdaptiveFiltered(the filter's options): readAdaptive's object with that error
    traceAdaptiveFiltered: (opts = {}) => a.traceAdaptiveFiltered(device, opts),
    readAdaptiveFiltered: (opts = {}) => a.readAdaptiveFiltered(device, opts),
    // the variance-guided preview filter of an adaptive render (include/crt.h "Denoised preview of an adaptive render"):
    // rgba8 of the tile, or {rgba8, variance} with opts.variance; reads only.  The Promise form resolves to the rgba8.
    denoiseAdaptive: (opts = {}) => a.denoiseAdaptive(device, opts),
    denoiseAdaptiveAsync: (opts = {}) => a.denoiseAdaptiveAsync(device, opts),
    // temporal reuse (include/crt.h "Sample offset", "Temporal reuse across camera moves"): distinct samples per frame,
    // and the frame blended with the previous frame's reprojected result before the filter; rgba8 of the tile, or
    // {rgba8, history} with opts.history; reads only.  The Promise form resolves to the rgba8.
    setSampleOffset: (offset) => a.setSampleOffset(device, offset),
    get sampleOffset() { return a.sampleOffset(device); },
    denoiseTemporal: (opts = {}) => a.denoiseTemporal(device, opts),
    denoiseTemporalAsync: (opts = {}) => a.denoiseTemporalAsync(device, opts),
    temporalReset: () => a.temporalReset(device),
    // motion vectors (include/crt.h crt_read_motion): Float32Array(tw*th*2), per pixel the film position where the last
    // denoiseTemporal looked for it in the previous frame, NaN where there is none.  setOption('temporal_motion', 1)
    // keeps the history across updatePrimitives and makes the positions follow the edited primitives.
    readMotion: () => a.readMotion(device),
    // the variance-guided temporal filter (include/crt.h "Variance-guided temporal filter"): denoiseTemporal's blend, then
    // the passes of denoiseAdaptive with the variance taken from the spread of the frame means; rgba8 of the tile, or
    // {rgba8, history?, variance?} with opts.history / opts.variance; reads only.  The Promise form resolves to the rgba8.
    denoiseSvgfDefaults: () => a.denoiseSvgfDefaults(),
    denoiseSvgf: (opts = {}) => a.denoiseSvgf(device, opts),
    denoiseSvgfAsync: (opts = {}) => a.denoiseSvgfAsync(device, opts),
    readMoments: () => a.readMoments(device),
    debugReadClipBox: () => a.debugReadClipBox(device),
    setOption: (name, value) => a.setOption(device, name, value),
    counters: () => a.counters(device),
    enableCounters: (on) => a.enableCounters(device, !!on),
    lastTraceMs: () => a.lastTraceMs(device),
    accelStats: () => a.accelStats(device),
    // the surface-area cost of the trees (include/crt.h crt_accel_quality): 12 numbers -- [0..3] boxes2, prims2, boxes4,
    // prims4 now, [4..7] as built, [8] refits since the build, [9] rebuilds that setOption('refit_rebuild_pct', P) has made
    // inside refitAccel, [10] 1 = the 4-wide values are present (else NaN)
    accelQuality: () => a.accelQuality(device),
    destroy: () => a.destroy(device),
  };
}

// The ops of transformPrimitives as packed crt_prim_transform records (60 bytes each: u32 first, u32 count, f32 m[12],
// f32 radius_scale); numbers become float32 by Math.fround's rule, as a Float32Array store rounds them.
function packTransforms(ops) {
  const buf = new ArrayBuffer(60 * ops.length), v = new DataView(buf);
  ops.forEach((op, k) => {
    if (!op.m || op.m.length !== 12) throw new TypeError('transformPrimitives: m must hold 12 numbers');
    v.setUint32(60 * k, op.first, true);
    v.setUint32(60 * k + 4, op.count, true);
    for (let i = 0; i < 12; i++) v.setFloat32(60 * k + 8 + 4 * i, op.m[i], true);
    v.setFloat32(60 * k + 56, op.radiusScale === undefined ? 1 : op.radiusScale, true);
  });
  return new Uint8Array(buf);
}

// The ranges of removePrimitives as packed crt_prim_range records (8 bytes each: u32 first, u32 count).
function packRanges(ranges) {
  const out = new Uint32Array(2 * ranges.length);
  ranges.forEach((r, k) => {
    out[2 * k] = Array.isArray(r) ? r[0] : r.first;
    out[2 * k + 1] = Array.isArray(r) ? r[1] : r.count;
  });
  return new Uint8Array(out.buffer);
}

// n cameras (Float32Array(16) each) whose eye turns about the look-at point around the up axis, k/n of a full turn for
// k = 0..n-1 (Rodrigues' rotation in doubles); look-at, up, width, height and focal length kept (scene.orbit_cameras).
function orbitCameras(camera, n) {
  const e = [0, 1, 2].map((i) => camera[i]), l = [4, 5, 6].map((i) => camera[i]), u = [8, 9, 10].map((i) => camera[i]);
  const un = Math.hypot(...u), k = u.map((x) => x / un), v = e.map((x, i) => x - l[i]);
  const kxv = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]];
  const kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
  const out = [];
  for (let j = 0; j < n; j++) {
    const a = (2 * Math.PI * j) / n, c = Math.cos(a), s = Math.sin(a);
    const cam = Float32Array.from(camera);
    for (let i = 0; i < 3; i++) cam[i] = l[i] + (v[i] * c + kxv[i] * s + k[i] * kv * (1 - c));
    out.push(cam);
  }
  return out;
}

// Binary PPM of the rgba8 framebuffer (row 0 = top, like the reference's blit).
function writePPM(file, rgba, width, height) {
  const out = Buffer.alloc(width * height * 3);
  for (let i = 0, j = 0; i < width * height * 4; i += 4, j += 3) {
    out[j] = rgba[i]; out[j + 1] = rgba[i + 1]; out[j + 2] = rgba[i + 2];
  }
  fs.writeFileSync(file, Buffer.concat([Buffer.from(`P6\n${width} ${height}\n255\n`), out]));
}

module.exports = { Main, writePPM, loadAddon, orbitCameras, packTransforms, packRanges };
