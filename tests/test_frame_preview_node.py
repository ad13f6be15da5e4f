"""GPU: the frame-level calls from JS (the N-API addon's readFrameAdaptive, denoiseFrame, denoiseAdaptiveFrame, blocking and
Promise form, on two ranks of the in-process transport) return what the Python path returns, and host/multi.js --denoise
writes the filtered frame."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")
W, H = 72, 61

SCRIPT = r"""
const fs = require('fs');
const { loadAddon } = require(process.argv[1] + '/host/main.js');
const sceneLoader = require(process.argv[1] + '/host/sceneLoader.js');
const dir = process.argv[2];
const a = loadAddon();
const scene = sceneLoader.loadScene(undefined);
scene.camera = { ...scene.camera, width: 72, height: 61 };
const packed = sceneLoader.pack(scene);
const id = new Uint8Array(a.commUniqueId(true));
const hs = [0, 1].map((k) => {
  const h = a.create(0);
  a.commInit(h, id, k, 2);
  a.uploadScene(h, packed.primitives, packed.lights, packed.spectra, packed.cie, packed.camera);
  a.commPartition(h, 8);
  a.buildAccel(h, 1);
  return h;
});
const put = (name, arr) => fs.writeFileSync(`${dir}/${name}`, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength));
for (const h of hs) a.trace(h, 4);
for (const h of hs) a.gather(h, 1 | 4);
put('uniform.bin', a.denoiseFrame(hs[1]));
put('uniform_k2.bin', a.denoiseFrame(hs[0], { iterations: 2, sigmaColor: 0.5 }));
let threw = '';
try { a.denoiseAdaptiveFrame(hs[0]); } catch (e) { threw = String(e.message); }
a.denoiseFrameAsync(hs[0], { iterations: 2, sigmaColor: 0.5 }).then((rgba) => {
  put('uniform_k2_async.bin', rgba);
  for (const h of hs) a.reset(h);
  for (let k = 0; k < 3; k++) for (const h of hs) a.traceAdaptive(h, { samples: 4, threshold: 0.05, minSamples: 4, maxSamples: 24 });
  for (const h of hs) a.gather(h, 1 | 4);
  const ad = a.readFrameAdaptive(hs[1]);
  put('counts.bin', ad.counts);
  put('errors.bin', ad.errors);
  const both = a.denoiseAdaptiveFrame(hs[0], { iterations: 3, sigmaVariance: 4, variance: true });
  put('adaptive.bin', both.rgba8);
  put('adaptive_var.bin', both.variance);
  return a.denoiseAdaptiveFrameAsync(hs[1], { iterations: 3, sigmaVariance: 4 }).then((rgba) => {
    put('adaptive_async.bin', rgba);
    console.log(JSON.stringify({ threw, tilesX: ad.tilesX, tilesY: ad.tilesY }));
    for (const h of hs) a.sync(h);
    for (const h of hs) a.destroy(h);
  });
}).catch((e) => { console.error(e); process.exit(1); });
"""


@pytest.fixture()
def pair():
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(W, H)
    cid = Renderer.comm_unique_id(local=True)
    rs = [Renderer(0) for _ in range(2)]
    for k, r in enumerate(rs):
        r.comm_init(cid, k, 2).upload(ps).comm_partition(8).build_accel("bvh2")
    yield rs
    for r in rs:
        r.sync()
    for r in rs:
        r.close()


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_frame_calls_equal_the_python_path(tmp_path, pair):
    out = subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, check=True, cwd=ROOT)
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert "uniform" in info["threw"] and (info["tilesX"], info["tilesY"]) == (9, 8)
    read = lambda name, dt, shape: np.frombuffer((tmp_path / name).read_bytes(), dt).reshape(shape)    # noqa: E731
    rs = pair
    for r in rs:
        r.frame(4)
    for r in rs:
        r.gather(rgba8=True, preview=True)
    assert np.array_equal(read("uniform.bin", np.uint8, (H, W, 4)), rs[1].denoise_frame())
    k2 = rs[0].denoise_frame(iterations=2, sigma_color=0.5)
    assert np.array_equal(read("uniform_k2.bin", np.uint8, (H, W, 4)), k2)
    assert np.array_equal(read("uniform_k2_async.bin", np.uint8, (H, W, 4)), k2)
    for r in rs:
        r.reset()
    for _ in range(3):
        for r in rs:
            r.trace_adaptive(samples=4, threshold=0.05, min_samples=4, max_samples=24)
    for r in rs:
        r.gather(rgba8=True, preview=True)
    counts, errors = rs[1].read_frame_adaptive()
    assert np.array_equal(read("counts.bin", np.uint32, (8, 9)), counts)
    assert np.array_equal(bits(read("errors.bin", np.float32, (8, 9))), bits(errors))
    rgba, var = rs[0].denoise_adaptive_frame(iterations=3, sigma_variance=4.0, var=True)
    assert np.array_equal(read("adaptive.bin", np.uint8, (H, W, 4)), rgba)
    assert np.array_equal(read("adaptive_async.bin", np.uint8, (H, W, 4)), rgba)
    assert np.array_equal(bits(read("adaptive_var.bin", np.float32, (H, W))), bits(var))


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_multi_gpu_host_writes_the_filtered_frame(tmp_path, pair):
    cmd = [NODE, os.path.join(ROOT, "host", "multi.js"), "--gpus", "2", "--local", "--width", str(W), "--height", str(H),
           "--spp", "2", "--frames", "2", "--band", "8", "--denoise", "3", "--dump", str(tmp_path / "frame.bin")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True)
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info["gpus"] == 2 and info["samples"] == 4
    for r in pair:
        r.frame(4)
    for r in pair:
        r.gather(rgba8=True, preview=True)
    rgba = np.frombuffer((tmp_path / "frame.bin").read_bytes(), np.uint8).reshape(H, W, 4)
    assert np.array_equal(rgba, pair[0].denoise_frame(iterations=3))
