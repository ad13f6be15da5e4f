"""GPU: option "svgf_spatial_pct" from JS.  node host/index.js --temporal --variance --spatial writes the
bytes that setOption + denoiseSvgf return through the N-API addon, and refuses --spatial without --variance."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")

SCRIPT = r"""
const fs = require('fs');
const { Main, orbitCameras } = require(process.argv[1] + '/host/main.js');
const dir = process.argv[2];
const r = Main({ width: 64, height: 48, accel: 'bvh2' });
let refused = '';
try { r.setOption('svgf_spatial_pct', 24); } catch (e) { refused = String(e.message); }
orbitCameras(r.packed.camera, 3).forEach((cam, k) => {
  r.setCamera(cam); r.setSampleOffset(4 * k); r.run(4);
  r.setOption('svgf_spatial_pct', 0);
  fs.writeFileSync(`${dir}/off_${k}.bin`, Buffer.from(r.denoiseSvgf({ iterations: 4 }).buffer));
  r.setOption('svgf_spatial_pct', 400);
  fs.writeFileSync(`${dir}/on_${k}.bin`, Buffer.from(r.denoiseSvgf({ iterations: 4 }).buffer));
});
console.log(JSON.stringify({ refused }));
r.destroy();
"""


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_command_line_writes_what_the_addon_returns(tmp_path):
    index = os.path.join(ROOT, "host", "index.js")
    base = [NODE, index, "--width", "64", "--height", "48", "--spp", "4", "--orbit", "3", "--denoise", "4", "--temporal"]
    bad = subprocess.run(base + ["--spatial", "--out", str(tmp_path / "bad.ppm")], capture_output=True, text=True)
    assert bad.returncode == 2 and "--spatial" in bad.stderr and not list(tmp_path.glob("bad*"))
    bad = subprocess.run(base + ["--variance", "--spatial", "24", "--out", str(tmp_path / "bad.ppm")], capture_output=True, text=True)
    assert bad.returncode == 2 and "--spatial" in bad.stderr
    run = subprocess.run(base + ["--variance", "--spatial", "--out", str(tmp_path / "orb.ppm")], capture_output=True, text=True, check=True)
    assert json.loads(run.stdout.strip().splitlines()[-1])["frames"] == 3
    out = subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, check=True, cwd=ROOT)
    assert "svgf_spatial_pct" in json.loads(out.stdout.strip().splitlines()[-1])["refused"]
    differs = []
    for k in range(3):
        on = np.frombuffer((tmp_path / f"on_{k}.bin").read_bytes(), np.uint8).reshape(48, 64, 4)
        off = np.frombuffer((tmp_path / f"off_{k}.bin").read_bytes(), np.uint8).reshape(48, 64, 4)
        assert (tmp_path / f"orb_{k:03d}.ppm").read_bytes() == b"P6\n64 48\n255\n" + np.ascontiguousarray(on[..., :3]).tobytes()
        differs.append(not np.array_equal(on, off))
    assert differs[0]                                           # the first frame: no pixel's variance is known, the box is in view
