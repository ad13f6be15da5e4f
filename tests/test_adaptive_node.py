"""GPU: adaptive sampling from JS (host/main.js traceAdaptive / readAdaptive through the N-API addon) gives the same bits
as the Python path."""
import json
import shutil
import subprocess

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
const active = [];
for (let k = 0; k < 4; k++) active.push(r.traceAdaptive({ samples: 4, threshold: 0.05, minSamples: 8, maxSamples: 24 }));
const ad = r.readAdaptive();
fs.writeFileSync(`${dir}/accum.bin`, Buffer.from(r.readAccum().buffer));
fs.writeFileSync(`${dir}/rgba8.bin`, Buffer.from(r.readRgba8().buffer));
fs.writeFileSync(`${dir}/counts.bin`, Buffer.from(ad.counts.buffer));
fs.writeFileSync(`${dir}/errors.bin`, Buffer.from(ad.errors.buffer));
console.log(JSON.stringify({ active, tilesX: ad.tilesX, tilesY: ad.tilesY }));
r.destroy();
"""


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_trace_adaptive_equals_the_python_path(tmp_path, renderer):
    from computeraytracer_amd import cornell
    out = subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, check=True, cwd=ROOT)
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info["tilesX"] == 8 and info["tilesY"] == 8
    renderer.upload(cornell(64, 64)).build_accel("bvh2")
    try:
        active = [renderer.trace_adaptive(samples=4, threshold=0.05, min_samples=8, max_samples=24) for _ in range(4)]
        counts, errors = renderer.read_adaptive()
        assert info["active"] == active
        assert np.array_equal(np.frombuffer((tmp_path / "counts.bin").read_bytes(), np.uint32).reshape(8, 8), counts)
        assert np.array_equal(np.frombuffer((tmp_path / "errors.bin").read_bytes(), np.float32).reshape(8, 8).view(np.uint32),
                              errors.view(np.uint32))
        acc = np.frombuffer((tmp_path / "accum.bin").read_bytes(), np.float32).reshape(64, 64, 4)
        rgba = np.frombuffer((tmp_path / "rgba8.bin").read_bytes(), np.uint8).reshape(64, 64, 4)
        assert np.array_equal(bits(acc), bits(renderer.read_accum())) and np.array_equal(rgba, renderer.read_rgba8())
    finally:
        renderer.reset()
