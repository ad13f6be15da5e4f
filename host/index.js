#!/usr/bin/env node
'use strict';
// CLI: node host/index.js [--scene file.json] [--width W --height H] [--spp N] [--accel bvh2|lbvh|ploc|none]
//                         [--out image.ppm] [--dump prefix] [--pack-only prefix] [--denoise K] [--orbit N [--temporal [--clip [PCT]] [--variance [--spatial [PCT]]]]]
// --denoise K: --out gets the image denoised with K a-trous iterations (crt_denoise; with --adaptive the variance-guided
//            crt_denoise_adaptive) instead of the plain average
// --orbit N: N frames of --spp each, the eye turned about the look-at point (one upload and build, then setCamera per
//            frame), written as OUT_000.ppm, OUT_001.ppm, ...
// --temporal: with --orbit N --denoise K, frame k draws samples k * spp + 1 .. (setSampleOffset) and is blended with the
//            reprojected result of frame k - 1 before the filter (denoiseTemporal)
// --variance: with --temporal, the passes after the blend are variance-guided, the variance taken from the spread of the
//            frame means (denoiseSvgf)
// --spatial [PCT]: with --variance, option "svgf_spatial_pct" = PCT (25..10000, 400 when given bare): a pixel with too short
//            a history for a temporal variance takes one from the spread of its 7x7 neighbourhood, times PCT / 100
// --clip [PCT]: with --temporal, option "temporal_clip_pct" = PCT (25..10000, 100 when given bare): the reprojected history of
//            a pixel is clamped to the mean +- PCT / 100 standard deviations of the frame's own colours over its 7x7
//            neighbourhood -- for lighting that changes on surfaces that do not; under a fixed camera with fixed lighting
//            it costs some of the history's benefit
// --adaptive T [--adaptive-step N] [--adaptive-min M]: adaptive sampling (traceAdaptive), rounds of N (16) samples until
//            every 8x8 tile has an error <= T or holds --spp samples; a tile below M (default min(--spp, 2N)) samples is
//            sampled whatever its error; prints rounds, pixel-samples, seconds and the min / median / max tile count.
//            With --orbit N every frame is sampled so and its mean samples per pixel are printed; with --denoise K
//            --temporal [--variance] besides, option "adaptive_temporal" lets frame k start at sample index k * spp + 1
//            and the temporal filters blend every pixel with its own tile's count
// --aov-out PREFIX: the feature planes of the samples the image holds (renderAovs(0); also with --adaptive, not with
//            --orbit), each as the raw bytes of its typed array: PREFIX_hits.bin (u32), PREFIX_alpha.bin, PREFIX_depth.bin
//            (f32), PREFIX_normal.bin, PREFIX_albedo.bin (4 x f32 per pixel)
// --matte-out PREFIX [--matte-source primitive|object|material] [--matte-slots K]: the id mattes of the samples the image
//            holds (renderMattes(0); also with --adaptive, not with --orbit), each as the raw bytes of its Uint32Array:
//            PREFIX_ids.bin, PREFIX_counts.bin (K planes, rank 0 first), PREFIX_hits.bin, PREFIX_overflow.bin
// --pick X,Y: after the render, what lies under pixel (X, Y) of the image (pick): primitive, object id, t, position and
//            normal go into the JSON line as "pick" (null where the pixel's ray hits nothing; not with --orbit)
const fs = require('fs');
const { Main, writePPM, orbitCameras } = require('./main');
const sceneLoader = require('./sceneLoader');

const args = {};
for (let i = 2; i < process.argv.length; i++) {
  const k = process.argv[i];
  if (k.startsWith('--')) args[k.slice(2)] = (i + 1 < process.argv.length && !process.argv[i + 1].startsWith('--')) ? process.argv[++i] : true;
}
const num = (k, d) => (k in args ? Number(args[k]) : d);

if (args['pack-only']) { // dump the packed host buffers (used by the packer parity test; needs no GPU)
  const scene = sceneLoader.loadScene(args.scene);
  if (args.width) scene.camera = { ...scene.camera, width: num('width'), height: num('height', num('width')) };
  const p = sceneLoader.pack(scene, undefined, args.scene ? require('path').dirname(require('path').resolve(args.scene)) : undefined);
  const pre = args['pack-only'];
  fs.writeFileSync(`${pre}.primitives.bin`, Buffer.from(p.primitives));
  fs.writeFileSync(`${pre}.patches.bin`, Buffer.from(p.patches));
  fs.writeFileSync(`${pre}.lights.bin`, Buffer.from(p.lights));
  fs.writeFileSync(`${pre}.camera.bin`, Buffer.from(p.camera.buffer));
  fs.writeFileSync(`${pre}.spectra.bin`, Buffer.from(p.spectra.buffer));
  fs.writeFileSync(`${pre}.cie.bin`, Buffer.from(p.cie.buffer));
  console.log(JSON.stringify({ nprim: p.primitives.byteLength / 80, nlight: p.lights.byteLength / 80, keyIndex: p.keyIndex }));
  process.exit(0);
}

const spp = num('spp', 16);
if (args.temporal && !(args.orbit && 'denoise' in args)) { console.error('--temporal goes with --orbit N --denoise K'); process.exit(2); }
if (args.variance && !args.temporal) { console.error('--variance goes with --orbit N --denoise K --temporal'); process.exit(2); }
const spatial = !('spatial' in args) ? null : args.spatial === true ? 400 : Number(args.spatial);
if (spatial !== null && !(args.variance && Number.isInteger(spatial) && spatial >= 25 && spatial <= 10000)) {
  console.error('--spatial [PCT] goes with --orbit N --denoise K --temporal --variance, PCT in 25..10000'); process.exit(2);
}
const clip = !('clip' in args) ? null : args.clip === true ? 100 : Number(args.clip);
if (clip !== null && !(args.temporal && Number.isInteger(clip) && clip >= 25 && clip <= 10000)) {
  console.error('--clip [PCT] goes with --orbit N --denoise K --temporal, PCT in 25..10000'); process.exit(2);
}
if ('aov-out' in args && (args.orbit || args['aov-out'] === true)) { console.error('--aov-out PREFIX writes the planes of one frame: give it a prefix, and no --orbit'); process.exit(2); }
if ('matte-out' in args && (args.orbit || args['matte-out'] === true)) { console.error('--matte-out PREFIX writes the mattes of one frame: give it a prefix, and no --orbit'); process.exit(2); }
let pickXY = null;
if ('pick' in args) {
  const m = /^(\d+),(\d+)$/.exec(String(args.pick));
  if (!m || args.orbit) { console.error('--pick takes X,Y, two non-negative integers, and no --orbit'); process.exit(2); }
  pickXY = [Number(m[1]), Number(m[2])];
}
const r = Main({ sceneFile: args.scene, width: args.width ? num('width') : undefined, height: args.height ? num('height') : undefined,
  accel: args.accel || 'bvh2', device: num('device', 0) });
function writeAovs() {
  if (!('aov-out' in args)) return;
  for (const [name, plane] of Object.entries(r.renderAovs(0)))
    fs.writeFileSync(`${args['aov-out']}_${name}.bin`, Buffer.from(plane.buffer, plane.byteOffset, plane.byteLength));
}
function writeMattes() {
  if (!('matte-out' in args)) return;
  for (const [name, plane] of Object.entries(r.renderMattes(0, args['matte-source'] || 'object', num('matte-slots', 8))))
    fs.writeFileSync(`${args['matte-out']}_${name}.bin`, Buffer.from(plane.buffer, plane.byteOffset, plane.byteLength));
}
function pickInfo() {
  if (!pickXY) return {};
  if (pickXY[0] >= r.width || pickXY[1] >= r.height) { console.error(`--pick ${pickXY}: outside the ${r.width} x ${r.height} image`); process.exit(2); }
  const h = r.pick(pickXY[0], pickXY[1]);
  return { pick: h && { x: pickXY[0], y: pickXY[1], primitive: h.prim, id: h.id, t: h.t, position: Array.from(h.position), normal: Array.from(h.normal) } };
}
// --adaptive: rounds of --adaptive-step samples until no tile is active; {rounds, ad: readAdaptive(), pixelSamples}
function adaptiveRounds() {
  const step = num('adaptive-step', 16), minS = num('adaptive-min', Math.min(spp, 2 * step));
  let rounds = 0;
  while (r.traceAdaptive({ samples: step, threshold: num('adaptive'), minSamples: minS, maxSamples: spp })) rounds++;
  const ad = r.readAdaptive();
  let pixelSamples = 0;
  for (let ty = 0; ty < ad.tilesY; ty++)
    for (let tx = 0; tx < ad.tilesX; tx++)
      pixelSamples += ad.counts[ty * ad.tilesX + tx] * Math.min(8, r.width - 8 * tx) * Math.min(8, r.height - 8 * ty);
  return { rounds, ad, pixelSamples };
}
if (args.orbit) {
  const n = num('orbit'), base = String(args.out || 'orbit.ppm').replace(/\.ppm$/, ''), outs = [], meanSamples = [];
  const t1 = process.hrtime.bigint();
  // --adaptive with --temporal: few samples per frame, placed where the noise is, accumulated over time
  if ('adaptive' in args && args.temporal) r.setOption('adaptive_temporal', 1);
  if (spatial !== null) r.setOption('svgf_spatial_pct', spatial);
  if (clip !== null) r.setOption('temporal_clip_pct', clip);
  orbitCameras(r.packed.camera, n).forEach((cam, k) => {
    r.setCamera(cam);
    if (args.temporal) r.setSampleOffset(k * spp);
    if ('adaptive' in args) meanSamples.push(adaptiveRounds().pixelSamples / (r.width * r.height));
    else r.run(spp);
    outs.push(`${base}_${String(k).padStart(3, '0')}.ppm`);
    const rgba = args.variance ? r.denoiseSvgf({ iterations: num('denoise') })
      : args.temporal ? r.denoiseTemporal({ iterations: num('denoise') })
      : !('denoise' in args) ? r.readRgba8()
      : 'adaptive' in args ? r.denoiseAdaptive({ iterations: num('denoise') }) : r.denoise({ iterations: num('denoise') });
    writePPM(outs[k], rgba, r.width, r.height);
  });
  console.log(JSON.stringify({ width: r.width, height: r.height, frames: n, spp, seconds: Number(process.hrtime.bigint() - t1) / 1e9, out: outs,
    ...('adaptive' in args ? { adaptive: num('adaptive'), mean_samples: meanSamples } : {}) }));
  r.destroy();
  process.exit(0);
}
if ('adaptive' in args) {
  const t1 = process.hrtime.bigint();
  const { rounds, ad, pixelSamples } = adaptiveRounds(), counts = Array.from(ad.counts).sort((a, b) => a - b);
  const seconds = Number(process.hrtime.bigint() - t1) / 1e9;
  if (args.out) writePPM(args.out, 'denoise' in args ? r.denoiseAdaptive({ iterations: num('denoise') }) : r.readRgba8(), r.width, r.height);
  writeAovs();
  writeMattes();
  const mid = counts.length >> 1, median = counts.length % 2 ? counts[mid] : (counts[mid - 1] + counts[mid]) / 2;
  console.log(JSON.stringify({ width: r.width, height: r.height, adaptive: num('adaptive'), rounds, pixel_samples: pixelSamples, seconds,
    tile_samples: { min: counts[0], median, max: counts[counts.length - 1] }, ...('denoise' in args ? { denoise: num('denoise') } : {}), ...pickInfo() }));
  r.destroy();
  process.exit(0);
}
r.enableCounters(true);
const t0 = process.hrtime.bigint();
r.run(spp, !args.unfused);
const dt = Number(process.hrtime.bigint() - t0) / 1e9;
const c = r.counters();
const rgba = r.readRgba8();
if (args.out) writePPM(args.out, 'denoise' in args ? r.denoise({ iterations: num('denoise') }) : rgba, r.width, r.height);
writeAovs();
writeMattes();
if (args.dump) {
  fs.writeFileSync(`${args.dump}.rgba8.bin`, Buffer.from(rgba.buffer));
  fs.writeFileSync(`${args.dump}.accum.bin`, Buffer.from(r.readAccum().buffer));
}
console.log(JSON.stringify({ width: r.width, height: r.height, spp, sample: r.sample, seconds: dt,
  rays: c[0], mrays_per_s: c[0] / dt / 1e6, kernel_ms: r.lastTraceMs()[0], ...pickInfo() }));
r.destroy();
