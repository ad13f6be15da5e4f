"""GPU: crt_trace_adaptive_filtered / crt_read_adaptive_filtered from JS (host/main.js traceAdaptiveFiltered /
readAdaptiveFiltered through the N-API addon) give the counts and errors the Python binding gives."""
import json
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")
W, H = 72, 61                                                # partial 8x8 tiles on both edges: 9 x 8

SCRIPT = r"""
const fs = require('fs');
const { Main } = require(process.argv[1] + '/host/main.js');
const dir = process.argv[2];
const r = Main({ width: 72, height: 61, accel: 'bvh2' });
const rule = { samples: 4, threshold: 0.02, minSamples: 8, maxSamples: 24 };
const narrow = { iterations: 3, sigmaVariance: 2.0, sigmaNormal: 0.25, sigmaPlane: 0.1 };
const active = [];
for (let k = 0; k < 4; k++) active.push(r.traceAdaptiveFiltered(rule));
active.push(r.traceAdaptiveFiltered({ ...rule, ...narrow }));
const ad = r.readAdaptiveFiltered();
const an = r.readAdaptiveFiltered(narrow);
fs.writeFileSync(`${dir}/accum.bin`, Buffer.from(r.readAccum().buffer));
fs.writeFileSync(`${dir}/counts.bin`, Buffer.from(ad.counts.buffer));
fs.writeFileSync(`${dir}/errors.bin`, Buffer.from(ad.errors.buffer));
fs.writeFileSync(`${dir}/errors_narrow.bin`, Buffer.from(an.errors.buffer));
let refusal = '';
try { r.traceAdaptiveFiltered({ ...rule, iterations: 11 }); } catch (e) { refusal = String(e.message); }
console.log(JSON.stringify({ active, tilesX: ad.tilesX, tilesY: ad.tilesY, refusal }));
r.destroy();
"""


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_filtered_selection_equals_the_python_path(tmp_path, renderer):
    from computeraytracer_amd import cornell
    out = subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, check=True, cwd=ROOT)
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info["tilesX"] == 9 and info["tilesY"] == 8
    assert "iterations" in info["refusal"]
    rule = dict(samples=4, threshold=0.02, min_samples=8, max_samples=24)
    narrow = dict(iterations=3, sigma_variance=2.0, sigma_normal=0.25, sigma_plane=0.1)
    renderer.upload(cornell(W, H)).build_accel("bvh2")
    try:
        active = [renderer.trace_adaptive_filtered(**rule) for _ in range(4)] + [renderer.trace_adaptive_filtered(**rule, **narrow)]
        counts, errors = renderer.read_adaptive_filtered()
        errors_narrow = renderer.read_adaptive_filtered(**narrow)[1]
        assert info["active"] == active and 0 < active[2] < 72
        assert np.array_equal(np.frombuffer((tmp_path / "counts.bin").read_bytes(), np.uint32).reshape(8, 9), counts)
        for name, want in (("errors.bin", errors), ("errors_narrow.bin", errors_narrow)):
            got = np.frombuffer((tmp_path / name).read_bytes(), np.float32).reshape(8, 9)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        assert not np.array_equal(errors.view(np.uint32), errors_narrow.view(np.uint32))      # (the filter's options arrive)
        acc = np.frombuffer((tmp_path / "accum.bin").read_bytes(), np.float32).reshape(H, W, 4)
        assert np.array_equal(bits(acc), bits(renderer.read_accum()))
    finally:
        renderer.reset()
