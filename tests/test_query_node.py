"""GPU: the ray queries from JS (host/main.js queryRays / pick through the N-API addon) return the bytes the Python path
returns, and the Node CLI's --pick reports the pixel's hit."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")
W, H = 40, 24

SCRIPT = r"""
const fs = require('fs');
const { Main } = require(process.argv[1] + '/host/main.js');
const dir = process.argv[2];
const r = Main({ width: 40, height: 24, accel: 'bvh2' });
const raw = fs.readFileSync(`${dir}/rays.bin`);
const rays = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
const put = (name, arr) => fs.writeFileSync(`${dir}/${name}`, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength));
r.run(2);
for (let k = 0; k < 3; k++) r.frame();        // in flight while the queries run
for (const [p, a] of Object.entries(r.queryRays(rays))) put(`closest_${p}.bin`, a);
const any = r.queryRays(rays, 'any');
put('any_hit.bin', any.hit);
const part = r.queryRays(rays, 'closest', ['t', 'uv']);
const picks = [[5, 7], [39, 23], [0, 0], [20, 12]].map(([x, y]) => {
  const h = r.pick(x, y);
  return h && { prim: h.prim, id: h.id, t: h.t, position: Array.from(h.position), normal: Array.from(h.normal), uv: Array.from(h.uv) };
});
let threw = [];
for (const f of [() => r.queryRays(rays, 'nearest'), () => r.queryRays(rays, 'closest', ['depth']), () => r.queryRays(rays.subarray(0, 7)),
                 () => r.queryRays(rays, 'any', ['hit', 't']), () => r.pick(40, 0)]) {
  try { f(); threw.push(''); } catch (e) { threw.push(String(e.message)); }
}
r.sync();
console.log(JSON.stringify({ picks, threw, keys: Object.keys(any), part: Object.keys(part).sort(), sample: r.sample }));
r.destroy();
"""


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_queries_equal_the_python_path(tmp_path, renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.renderer import pack_rays
    ps = cornell(W, H)
    rng = np.random.default_rng(12)
    n = 333
    o = np.tile(ps.camera[0:3].astype(np.float32), (n, 1)) + rng.normal(size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    t_max = np.where(np.arange(n) % 4 == 0, np.float32(300.0), np.float32(np.inf)).astype(np.float32)
    ex = np.where(np.arange(n) % 5 == 0, np.uint32(3), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    rays = pack_rays(o, d, t_max, ex)
    (tmp_path / "rays.bin").write_bytes(rays.tobytes())
    out = subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, check=True, cwd=ROOT)
    info = json.loads(out.stdout.strip().splitlines()[-1])
    renderer.upload(ps).build_accel("bvh2")
    want = renderer.query_rays(rays=rays)
    assert want["hit"].any() and not want["hit"].all()
    for p, a in want.items():
        got = np.frombuffer((tmp_path / f"closest_{p}.bin").read_bytes(), a.dtype).reshape(a.shape)
        assert np.array_equal(got.view(np.uint32), a.view(np.uint32)), p
    assert np.array_equal(np.frombuffer((tmp_path / "any_hit.bin").read_bytes(), np.uint32), want["hit"])
    assert info["keys"] == ["hit"] and info["part"] == ["t", "uv"] and info["sample"] == 5
    for (x, y), got in zip([(5, 7), (39, 23), (0, 0), (20, 12)], info["picks"]):
        w = renderer.pick(x, y)
        assert (got is None) == (w is None)
        if w is not None:
            assert (got["prim"], got["id"]) == (w["prim"], w["id"]) and np.float32(got["t"]) == np.float32(w["t"])
            for k in ("position", "normal", "uv"):
                assert np.array_equal(np.array(got[k], np.float32), w[k]), k      # (by value: JSON does not carry the sign of a zero)
    t = info["threw"]
    assert "unknown mode" in t[0] and "unknown plane" in t[1] and "8 floats per ray" in t[2]
    assert "CRT_QUERY_ANY" in t[3] and "(-1)" in t[3] and "outside" in t[4] and "(-1)" in t[4]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_cli_pick(tmp_path, renderer):
    from computeraytracer_amd import cornell
    out = subprocess.run([NODE, os.path.join(ROOT, "host", "index.js"), "--width", "32", "--height", "32", "--spp", "2", "--pick", "16,20",
                          "--out", str(tmp_path / "o.ppm")], capture_output=True, text=True, check=True)
    info = json.loads(out.stdout.strip().splitlines()[-1])
    ps = cornell(32, 32)
    renderer.upload(ps).build_accel("bvh2")
    w = renderer.pick(16, 20)
    assert w is not None and info["pick"]["primitive"] == w["prim"] and (info["pick"]["x"], info["pick"]["y"]) == (16, 20)
    assert np.float32(info["pick"]["t"]) == np.float32(w["t"])
    assert np.array_equal(np.array(info["pick"]["position"], np.float32), w["position"])      # (by value: JSON has no -0)
    assert np.array_equal(np.array(info["pick"]["normal"], np.float32), w["normal"])
    bad = subprocess.run([NODE, os.path.join(ROOT, "host", "index.js"), "--width", "32", "--height", "32", "--spp", "1", "--pick", "32,0"],
                         capture_output=True, text=True)
    assert bad.returncode == 2 and "outside" in bad.stderr
