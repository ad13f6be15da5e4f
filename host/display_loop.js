#!/usr/bin/env node
'use strict';
/*
 * display_loop.js -- the reference's frame loop as a display loop sees it (src/main.js:597-620: one compute pass per
 * sample, then the blit of THAT frame, then requestAnimationFrame): every frame index is shown exactly once, in order,
 * while the renderer runs ahead of the display by `lag` frames (64: a cohort of 16 samples plus the time its longest paths take to
 * retire, DESIGN.md 5.1) -- far enough for small calls to be merged into cohorts and for no read to wait for its frame.
 *
 *   frame k:   trace(1)                       request sample k          (returns at once: the call only notes the sample)
 *              readSampleRgba8(k - lag)       show sample k - lag       (from the ring of the last F frames; waits only for
 *                                                                        the batch that holds it, never flushes)
 *
 *   node host/display_loop.js [--scene f.json | --packed prefix] [--width W --height H] [--frames 640] [--lag 64] [--ring 128] [--check 1]
 *                             [--cohort C] [--denoise K]
 *   --cohort C: option "wf_cohort" = C (calls merged per batch: 16 by default, times up to 8 on a frame below 2 Mpixels).
 *   --check 1: every shown frame is compared with a synchronous trace(1); sync(); readRgba8() loop on a second context.
 * Prints one JSON line: ms per shown frame, frames shown, whether every index appeared once and in order.
 *
 *   --denoise K: the FILTERED display loop (DESIGN.md 6m).  A filtered frame exists only for the newest complete sample
 *   index (the filter reads the accumulator, and no ring keeps accumulators), so this loop shows that one:
 *   frame k:   trace(1)                       request sample k
 *              denoiseLatestInto(frame, K)    show the newest complete frame, filtered with K passes, and its index --
 *                                             no flush: the trace calls stay a cohort ahead
 *   and ends on sync + denoise of the final count.  Prints the sample index shown per frame and one JSON line: ms per
 *   frame, the indices shown (non-decreasing), how many frames had nothing complete to show yet.  With --check 1 every
 *   shown frame is compared with sync + denoise of the same index on a second context.
 */
const path = require('path');
const { loadAddon } = require('./main');
const sceneLoader = require('./sceneLoader');

const args = {};
for (let i = 2; i < process.argv.length; i++) {
  const k = process.argv[i];
  if (k.startsWith('--')) args[k.slice(2)] = (i + 1 < process.argv.length && !process.argv[i + 1].startsWith('--')) ? process.argv[++i] : true;
}
const num = (k, d) => (k in args ? Number(args[k]) : d);
const a = loadAddon();
let packed;
if (args.packed) {
  // buffers packed elsewhere (tools/dump_packed.py writes the synthetic benchmark scenes): <prefix>.{primitives,lights,camera,spectra,cie}.bin
  const fs = require('fs');
  const rd = (n) => { const b = fs.readFileSync(`${args.packed}.${n}.bin`); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
  const camera = new Float32Array(rd('camera'));
  packed = { primitives: rd('primitives'), lights: rd('lights'), camera, spectra: new Float32Array(rd('spectra')), cie: new Float32Array(rd('cie')),
    width: camera[11], height: camera[12] };
} else {
  const scene = sceneLoader.loadScene(args.scene);
  if (args.width) scene.camera = { ...scene.camera, width: num('width'), height: num('height', num('width')) };
  packed = sceneLoader.pack(scene, undefined, args.scene ? path.dirname(path.resolve(args.scene)) : undefined);
}
const frames = num('frames', 640), lag = num('lag', 64), ring = num('ring', 128), check = num('check', 0);

function make() {
  const h = a.create(num('device', 0));
  a.uploadScene(h, packed.primitives, packed.lights, packed.spectra, packed.cie, packed.camera);
  a.buildAccel(h, 1);
  return h;
}
const h = make();
if ('cohort' in args) a.setOption(h, 'wf_cohort', num('cohort'));   // (a small frame merges up to 8 x as many calls per cohort)
if ('denoise' in args) { denoiseLoop(h, args.denoise === true ? 5 : num('denoise')); return; }
a.setOption(h, 'frame_ring', ring);
let ref = null;
if (check) ref = make();

let shown = 0, inOrder = true, equal = true;
// the display's frame buffer: one page-locked array, reused frame after frame (the readback then runs at PCIe speed)
const frame = new Uint8Array(packed.width * packed.height * 4);
a.pinHost(frame);
const show = (k) => {
  a.readSampleRgba8Into(h, k, frame);                        // the display step: frame k, complete, as a synced loop would show it
  shown++;
  if (ref) {
    a.trace(ref, 1); a.sync(ref);
    const want = a.readRgba8(ref);
    if (a.sampleCount(ref) !== k) inOrder = false;
    for (let i = 0; i < want.length; i++) if (want[i] !== frame[i]) { equal = false; break; }
  }
};
const t0 = process.hrtime.bigint();
for (let k = 1; k <= frames; k++) {
  a.trace(h, 1);
  if (k > lag) show(k - lag);
}
for (let k = Math.max(1, frames - lag + 1); k <= frames; k++) show(k);   // the tail: the last frames are shown as they complete
const ms = Number(process.hrtime.bigint() - t0) / 1e6;
console.log(JSON.stringify({ width: packed.width, height: packed.height, frames, lag, ring, shown, every_index_once_in_order: shown === frames && inOrder,
  equal_to_synced_loop: ref ? equal : null, ms_per_frame: ms / frames, latest: a.latestSample(h) }));
a.unpinHost(frame);
a.destroy(h);
if (ref) a.destroy(ref);

function denoiseLoop(h, K) {
  const opts = { iterations: K };
  const ref = check ? make() : null;
  const frame = new Uint8Array(packed.width * packed.height * 4);
  a.pinHost(frame);
  const indices = [];
  let nothingYet = 0, nonDecreasing = true, equal = true, last = 0;
  const t0 = process.hrtime.bigint();
  for (let k = 1; k <= frames; k++) {
    a.trace(h, 1);
    let s = 0;
    try { s = a.denoiseLatestInto(h, frame, opts); } catch (e) {
      if (!/no complete frame yet/.test(String(e.message))) throw e;   // (only that refusal is part of the loop)
      nothingYet++;
      continue;
    }
    if (s < last || s > k) nonDecreasing = false;
    last = s;
    indices.push(s);
    if (!args.quiet) console.log(`frame ${k}: sample ${s}`);
    if (ref) {
      while (a.sampleCount(ref) < s) a.trace(ref, 1);
      a.sync(ref);
      const want = a.denoise(ref, opts);
      for (let i = 0; i < want.length; i++) if (want[i] !== frame[i]) { equal = false; break; }
    }
  }
  const ms = Number(process.hrtime.bigint() - t0) / 1e6;
  a.sync(h);
  const final = a.denoise(h, opts);                            // the loop ends on the synced filter of everything requested
  const end = a.denoiseLatestInto(h, frame, opts);
  let endEqual = end === frames;
  for (let i = 0; endEqual && i < final.length; i++) if (final[i] !== frame[i]) endEqual = false;
  console.log(JSON.stringify({ width: packed.width, height: packed.height, frames, denoise: K, shown: indices.length, nothing_complete_yet: nothingYet,
    samples_shown: indices, non_decreasing: nonDecreasing, equal_to_synced_denoise: ref ? equal : null, ends_on_synced_denoise: endEqual,
    final_sample: end, ms_per_frame: ms / frames }));
  a.unpinHost(frame);
  a.destroy(h);
  if (ref) a.destroy(ref);
}
