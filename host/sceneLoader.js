'use strict';
/*
 * sceneLoader.js -- scene flatten + pack for the compute pass.
 *
 * The reference's src/sceneLoader.js is a 5-line stub; the packing it was
 * meant to hold lives inline in src/main.js:114-393.  This module is that
 * code as a loader: same JSON schema in, byte-identical buffers out
 * (bind group 0, b3..b8 of ComputeShader.wgsl:1-9):
 *
 *   primitives  n x 80 B  main.js:211-246   lights  n x 80 B  main.js:255-296
 *   patches     n x 64 B  main.js:138-209   camera  16 f32    main.js:313-324
 *   spectra     n x 301   main.js:334-378   cie     3 x 471   main.js:380-393
 *
 * Extensions: objects.triangles [{v0,v1,v2,emission,reflectance,type}] and objects.meshes
 * [{obj: 'file.obj' | vertices+indices, scale, translate, emission, reflectance, type}] ->
 * category 2 records (v0, v1-v0, v2-v0), appended after the spheres.
 * The Python twin is computeraytracer_amd/scene.py.
 */
const fs = require('fs');
const path = require('path');

const SCENES_DIR = path.join(__dirname, '..', 'scenes');
const LAMBDA_MIN = 400; // main.js:334
const LAMBDA_MAX = 700; // main.js:335
const RANGE = LAMBDA_MAX - LAMBDA_MIN + 1;
const TYPE_INDEX = { diffuse: 0, light: 1, glass: 2 }; // main.js:166-170

const lerp = (a, b, t) => a * (1 - t) + b * t; // main.js:626

// main.js:340-356
function sampleSpectrum(spectrum, lambda) {
  const index = spectrum.wavelength.findIndex((e) => e >= lambda);
  const startIndex = Math.max(index - 1, 0);
  const endIndex = Math.min(index, spectrum.wavelength.length - 1);
  const start = spectrum.value[startIndex];
  const end = spectrum.value[endIndex];
  const startLambda = spectrum.wavelength[startIndex];
  const endLambda = spectrum.wavelength[endIndex];
  if (startLambda === endLambda) return start;
  return lerp(start, end, (lambda - startLambda) / (endLambda - startLambda));
}

// main.js:157-164 + 358-367
function resampleSpectra(spectra) {
  const keyIndex = {};
  const keys = Object.keys(spectra);
  const table = new Float32Array(keys.length * RANGE);
  keys.forEach((key, j) => {
    keyIndex[key] = j;
    for (let i = 0; i < RANGE; i++) table[j * RANGE + i] = sampleSpectrum(spectra[key], LAMBDA_MIN + i);
  });
  return { table, keyIndex };
}

// Minimal Wavefront OBJ reader: `v x y z`, `f a b c ...` (1-based, negative = relative, a/b/c
// forms accepted, polygons fan-triangulated).
function parseObj(text) {
  const verts = [], tris = [];
  for (const line of text.split(/\r?\n/)) {
    const t = line.trim().split(/\s+/);
    if (!t[0] || t[0].startsWith('#')) continue;
    if (t[0] === 'v' && t.length >= 4) verts.push([Number(t[1]), Number(t[2]), Number(t[3])]);
    else if (t[0] === 'f' && t.length >= 4) {
      const idx = t.slice(1).map((w) => { const k = parseInt(w.split('/')[0], 10); return k > 0 ? k - 1 : verts.length + k; });
      for (let j = 1; j < idx.length - 1; j++) tris.push([idx[0], idx[j], idx[j + 1]]);
    }
  }
  return { verts, tris };
}

// objects.meshes -> triangle objects (vertex = v * scale + translate, in doubles)
function expandMeshes(scene, baseDir) {
  const out = [];
  for (const m of ((scene.objects || {}).meshes || [])) {
    let verts, tris;
    if (m.obj) {
      const file = path.isAbsolute(m.obj) ? m.obj : path.join(baseDir || SCENES_DIR, m.obj);
      ({ verts, tris } = parseObj(fs.readFileSync(file, 'utf8')));
    } else {
      verts = m.vertices;
      tris = Array.isArray(m.indices[0]) ? m.indices : m.indices.reduce((a, v, i) => (i % 3 ? a[a.length - 1].push(v) : a.push([v]), a), []);
    }
    const sc = Array.isArray(m.scale) ? m.scale : [m.scale === undefined ? 1 : m.scale, m.scale === undefined ? 1 : m.scale, m.scale === undefined ? 1 : m.scale];
    const tr = m.translate || [0, 0, 0];
    const P = verts.map((v) => [v[0] * sc[0] + tr[0], v[1] * sc[1] + tr[1], v[2] * sc[2] + tr[2]]);
    for (const [a, b, c] of tris) out.push({ v0: P[a], v1: P[b], v2: P[c], emission: m.emission, reflectance: m.reflectance, type: m.type });
  }
  return out;
}

// main.js:114-137: patches then spheres (then triangles); index = array position
function flatten(scene, baseDir) {
  const objects = scene.objects || {};
  const primitives = [];
  (objects.patches || []).forEach((p) => primitives.push({ ...p, index: primitives.length, category: 'patch' }));
  (objects.spheres || []).forEach((s) => primitives.push({ ...s, index: primitives.length, category: 'sphere' }));
  (objects.triangles || []).concat(expandMeshes(scene, baseDir)).forEach((t) => primitives.push({ ...t, index: primitives.length, category: 'triangle' }));
  return primitives;
}

function writeRecord(buf, offset, category, d1, d2, d3, emission, reflectance, type, index) {
  new Uint32Array(buf, offset, 1).set([category]);
  new Float32Array(buf, offset + 16, 3).set(d1);
  new Float32Array(buf, offset + 32, 3).set(d2);
  new Float32Array(buf, offset + 48, 3).set(d3);
  new Uint32Array(buf, offset + 64, 4).set([emission, reflectance, type, index]);
}

const f32 = Math.fround;
const sub32 = (a, b) => [f32(f32(a[0]) - f32(b[0])), f32(f32(a[1]) - f32(b[1])), f32(f32(a[2]) - f32(b[2]))];

function loadCie(file) {
  const d = JSON.parse(fs.readFileSync(file || path.join(SCENES_DIR, 'cie1931_xyz_1nm.json'), 'utf8'));
  const X = d.X || d.CIE_X, Y = d.Y || d.CIE_Y, Z = d.Z || d.CIE_Z;
  if (X.length !== 471 || Y.length !== 471 || Z.length !== 471) throw new RangeError('CIE table must be 3 x 471');
  return new Float32Array([...X, ...Y, ...Z]); // main.js:382
}

function pack(scene, cie, baseDir) {
  const prims = flatten(scene, baseDir);
  const { table: spectra, keyIndex } = resampleSpectra(scene.spectra);
  const idx = (name) => {
    if (!(name in keyIndex)) throw new Error(`unknown spectrum '${name}'`);
    return keyIndex[name];
  };
  const type = (t) => {
    if (!(t in TYPE_INDEX)) throw new Error(`unknown material type '${t}'`);
    return TYPE_INDEX[t];
  };

  const primitives = new ArrayBuffer(prims.length * 80); // main.js:147-151
  prims.forEach((p, i) => {
    if (p.category === 'patch') {
      writeRecord(primitives, i * 80, 0, p.origin, p.edge1, p.edge2, idx(p.emission), idx(p.reflectance), type(p.type), p.index);
    } else if (p.category === 'sphere') {
      writeRecord(primitives, i * 80, 1, p.center, [p.radius, p.radius, p.radius], [0, 0, 0], idx(p.emission), idx(p.reflectance), type(p.type), p.index);
    } else {
      writeRecord(primitives, i * 80, 2, p.v0, sub32(p.v1, p.v0), sub32(p.v2, p.v0), idx(p.emission), idx(p.reflectance), type(p.type), p.index);
    }
  });

  const pl = (scene.objects && scene.objects.patches) || [];
  const patches = new ArrayBuffer(pl.length * 64); // main.js:138-209
  pl.forEach((p, i) => {
    new Float32Array(patches, i * 64, 3).set(p.origin);
    new Float32Array(patches, i * 64 + 16, 3).set(p.edge1);
    new Float32Array(patches, i * 64 + 32, 3).set(p.edge2);
    new Uint32Array(patches, i * 64 + 44, 4).set([idx(p.emission), idx(p.reflectance), type(p.type), i]);
  });

  const lightPrims = prims.filter((p) => p.type === 'light'); // main.js:255-260
  const lights = new ArrayBuffer(lightPrims.length * 80);
  lightPrims.forEach((p, i) => {
    // main.js:285-292 packs every light with the patch fields (category word 0)
    const d1 = p.origin || p.center || p.v0;
    const d2 = p.edge1 || (p.v1 ? sub32(p.v1, p.v0) : [p.radius, p.radius, p.radius]);
    const d3 = p.edge2 || (p.v2 ? sub32(p.v2, p.v0) : [0, 0, 0]);
    writeRecord(lights, i * 80, 0, d1, d2, d3, idx(p.emission), idx(p.reflectance), type(p.type), p.index);
  });

  // one object id per patch, sphere, loose triangle and mesh, in primitive order (crt_set_primitive_ids): every triangle
  // of a mesh carries the mesh's id
  const ob = scene.objects || {};
  const single = (ob.patches || []).length + (ob.spheres || []).length + (ob.triangles || []).length;
  const objectIds = new Uint32Array(prims.length);
  for (let i = 0; i < single; i++) objectIds[i] = i;
  let at = single;
  (ob.meshes || []).forEach((m, j) => {
    const k = expandMeshes({ objects: { meshes: [m] } }, baseDir).length;
    objectIds.fill(single + j, at, at + k);
    at += k;
  });

  const c = scene.camera; // main.js:313-324
  const camera = new Float32Array([...c.eye, 0, ...c.lookat, 0, ...c.up, c.width, c.height, c.focalLength, 0, 0]);

  return { primitives, patches, lights, camera, spectra, cie: cie || loadCie(), keyIndex, objectIds, width: c.width, height: c.height };
}

function loadScene(file) {
  return JSON.parse(fs.readFileSync(file || path.join(SCENES_DIR, 'cornell_box.json'), 'utf8'));
}

module.exports = { loadScene, loadCie, flatten, pack, parseObj, expandMeshes, resampleSpectra, sampleSpectrum, SCENES_DIR, TYPE_INDEX };
