"""GPU: crt_denoise_latest from JS.  denoiseLatest / denoiseLatestInto / denoiseLatestAsync of the N-API
addon return what the Python path returns for the same sample index, a blocking call is refused while a Promise is queued,
and node host/display_loop.js --denoise K shows non-decreasing sample indices and ends on the synced denoise."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")
W, H = 72, 61

SCRIPT = r"""
const fs = require('fs');
const { Main } = require(process.argv[1] + '/host/main.js');
const dir = process.argv[2];
(async () => {
  const r = Main({ width: 72, height: 61, accel: 'bvh2' });
  const info = { early: '', busy: '', samples: [] };
  try { r.denoiseLatest(); } catch (e) { info.early = String(e.message); }
  r.setOption('wf_cohort', 16);
  r.run(16);
  for (let k = 0; k < 5; k++) r.frame();                       // requested, merged, unpublished
  const a = r.denoiseLatest({ rgb: true });
  const b = r.denoiseLatest({ iterations: 3, sigmaColor: 0.7 });
  const into = new Uint8Array(72 * 61 * 4);
  const s = r.denoiseLatestInto(into, { iterations: 3, sigmaColor: 0.7 });
  info.samples = [a.sample, b.sample, s, r.sample];
  info.keys = [Object.keys(a).sort(), Object.keys(b).sort()];
  fs.writeFileSync(`${dir}/a_rgba8.bin`, Buffer.from(a.rgba8.buffer));
  fs.writeFileSync(`${dir}/a_rgb.bin`, Buffer.from(a.rgb.buffer));
  fs.writeFileSync(`${dir}/b_rgba8.bin`, Buffer.from(b.rgba8.buffer));
  fs.writeFileSync(`${dir}/into.bin`, Buffer.from(into.buffer));
  const p = r.denoiseLatestAsync({ rgb: true });
  try { r.denoiseLatest(); } catch (e) { info.busy = String(e.code) + ' ' + String(e.message); }
  const c = await p;
  info.samples.push(c.sample);
  fs.writeFileSync(`${dir}/c_rgba8.bin`, Buffer.from(c.rgba8.buffer));
  fs.writeFileSync(`${dir}/c_rgb.bin`, Buffer.from(c.rgb.buffer));
  const d = await r.denoiseLatestAsync();
  info.keys.push(Object.keys(d).sort());
  r.sync();
  info.samples.push(r.denoiseLatest().sample);
  console.log(JSON.stringify(info));
  r.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
"""


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_returns_what_the_library_returns(tmp_path):
    from computeraytracer_amd import Renderer, cornell
    out = subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert "no complete frame yet" in info["early"]
    assert "BUSY" in info["busy"]
    assert info["samples"] == [16, 16, 16, 21, 16, 21]
    assert info["keys"] == [["rgb", "rgba8", "sample"], ["rgba8", "sample"], ["rgba8", "sample"]]
    with Renderer(0) as r:
        r.upload(cornell(W, H)).build_accel("bvh2").set_option("wf_cohort", 16)
        r.frame(16).sync()
        for _ in range(5):
            r.frame(1)
        rgb, rgba, s = r.denoise_latest()
        rgb3, rgba3, s3 = r.denoise_latest(3, 0.7)
        assert (s, s3) == (16, 16)

    def blob(name, dtype):
        return np.frombuffer((tmp_path / name).read_bytes(), dtype).reshape(H, W, 4)

    for name in ("a", "c"):
        assert np.array_equal(blob(f"{name}_rgba8.bin", np.uint8), rgba)
        assert np.array_equal(blob(f"{name}_rgb.bin", np.uint32), rgb.view(np.uint32))
    assert np.array_equal(blob("b_rgba8.bin", np.uint8), rgba3)
    assert np.array_equal(blob("into.bin", np.uint8), rgba3)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_display_loop_denoise():
    loop = os.path.join(ROOT, "host", "display_loop.js")
    run = subprocess.run([NODE, loop, "--width", str(W), "--height", str(H), "--frames", "2000", "--cohort", "2", "--denoise", "5", "--check", "1"],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    info = json.loads(lines[-1])
    shown = info["samples_shown"]
    assert info["denoise"] == 5 and info["shown"] == len(shown) and info["shown"] + info["nothing_complete_yet"] == 2000
    # (cohorts of 16 on this frame; 2000 frames because a frame of the loop takes the host microseconds while nothing is
    # complete, and the first batch needs a few kernel launches' time to retire)
    assert shown
    assert shown == sorted(shown) and info["non_decreasing"] and all(1 <= s <= 2000 for s in shown)
    assert [ln for ln in lines[:-1] if ln.startswith("frame ")][-1].endswith(f"sample {shown[-1]}")
    assert info["equal_to_synced_denoise"] is True
    assert info["ends_on_synced_denoise"] is True and info["final_sample"] == 2000
