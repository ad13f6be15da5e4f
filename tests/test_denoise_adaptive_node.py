"""GPU: the variance-guided preview filter from JS (host/main.js denoiseAdaptive through the N-API addon, blocking and
Promise form) returns the bytes the Python path returns, and the command line writes it with --adaptive --denoise."""
import json
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")

SCRIPT = r"""
const fs = require('fs');
const { Main } = require(process.argv[1] + '/host/main.js');
const dir = process.argv[2];
const r = Main({ width: 64, height: 64, accel: 'bvh2' });
for (let k = 0; k < 4; k++) r.traceAdaptive({ samples: 4, threshold: 0.05, minSamples: 8, maxSamples: 24 });
fs.writeFileSync(`${dir}/default.bin`, Buffer.from(r.denoiseAdaptive().buffer));
const both = r.denoiseAdaptive({ iterations: 3, sigmaVariance: 4, sigmaNormal: 0.25, sigmaPlane: 0.2, variance: true });
fs.writeFileSync(`${dir}/k3.bin`, Buffer.from(both.rgba8.buffer));
fs.writeFileSync(`${dir}/k3_var.bin`, Buffer.from(both.variance.buffer));
let threw = '';
try { r.denoiseAdaptive({ iterations: 11 }); } catch (e) { threw = String(e.message); }
r.denoiseAdaptiveAsync({ iterations: 3, sigmaVariance: 4, sigmaNormal: 0.25, sigmaPlane: 0.2 }).then((rgba) => {
  fs.writeFileSync(`${dir}/k3_async.bin`, Buffer.from(rgba.buffer));
  console.log(JSON.stringify({ threw }));
  r.destroy();
});
"""


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_denoise_adaptive_equals_the_python_path(tmp_path, renderer):
    from computeraytracer_amd import cornell
    out = subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, check=True, cwd=ROOT)
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert "iterations" in info["threw"]
    renderer.upload(cornell(64, 64)).build_accel("bvh2")
    try:
        for _ in range(4):
            renderer.trace_adaptive(samples=4, threshold=0.05, min_samples=8, max_samples=24)
        read = lambda name, dt, shape: np.frombuffer((tmp_path / name).read_bytes(), dt).reshape(shape)    # noqa: E731
        assert np.array_equal(read("default.bin", np.uint8, (64, 64, 4)), renderer.denoise_adaptive())
        rgba, var = renderer.denoise_adaptive(3, 4.0, 0.25, 0.2, var=True)
        assert np.array_equal(read("k3.bin", np.uint8, (64, 64, 4)), rgba)
        assert np.array_equal(read("k3_async.bin", np.uint8, (64, 64, 4)), rgba)
        assert np.array_equal(bits(read("k3_var.bin", np.float32, (64, 64))), bits(var))
    finally:
        renderer.reset()


def test_command_line_writes_the_filtered_adaptive_image(tmp_path, renderer):
    from computeraytracer_amd import cornell, image
    out = tmp_path / "ad.png"
    run = subprocess.run([sys.executable, "-m", "computeraytracer_amd", "--width", "64", "--height", "48", "--spp", "32",
                          "--adaptive", "0.05", "--adaptive-step", "8", "--denoise", "4", "--out", str(out)],
                         capture_output=True, text=True, check=True, cwd=ROOT)
    info = json.loads(run.stdout.strip().splitlines()[-1])
    assert info["adaptive"] == 0.05 and info["denoise"] == 4 and info["out"] == str(out)
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    renderer.upload(cornell(64, 48)).build_accel("bvh2")
    try:
        while renderer.trace_adaptive(samples=8, threshold=0.05, min_samples=16, max_samples=32):
            pass
        want = tmp_path / "want.png"
        image.write_png(str(want), renderer.denoise_adaptive(4))
        assert out.read_bytes() == want.read_bytes()
    finally:
        renderer.reset()


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_command_line_writes_the_filtered_adaptive_image(tmp_path, renderer):
    import os
    from computeraytracer_amd import cornell
    out = tmp_path / "ad.ppm"
    run = subprocess.run([NODE, os.path.join(ROOT, "host", "index.js"), "--width", "64", "--height", "48", "--spp", "32",
                          "--adaptive", "0.05", "--adaptive-step", "8", "--denoise", "4", "--out", str(out)],
                         capture_output=True, text=True, check=True)
    info = json.loads(run.stdout.strip().splitlines()[-1])
    assert info["adaptive"] == 0.05 and info["denoise"] == 4
    renderer.upload(cornell(64, 48)).build_accel("bvh2")
    try:
        while renderer.trace_adaptive(samples=8, threshold=0.05, min_samples=16, max_samples=32):
            pass
        rgba = renderer.denoise_adaptive(4)
        assert out.read_bytes() == b"P6\n64 48\n255\n" + np.ascontiguousarray(rgba[..., :3]).tobytes()
    finally:
        renderer.reset()
