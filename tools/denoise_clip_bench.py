"""crt_denoise_temporal with option "temporal_clip_pct" on S2 (atrium250k) at 1920 x 1080: two contexts in one
process render the same two frames of an orbit, --spp samples each with distinct samples.  In the first the option is
--pct (100), so the second frame's call runs k_dn_clip_box before the blend; in the second the option is never set.  Then
the host clock around the synchronous K = 5 call on the second frame with no outputs requested (the launches and the sync
alone), warm, the two contexts alternately, median of --reps.  Calls within one frame blend against the same previous
slot: every repetition does the same work.

  clip.k5_compute       K = 5 with the box pass and the clamp
  plain.k5_compute      the same call, the option never set: the call as it was before the option existed
  k5_ratio              clip.k5_compute / plain.k5_compute (medians)
  spread                |median of the first half - median of the second half| / median of plain.k5_compute's repetitions:
                        what two runs of the same call differ by; a difference between commits below it is none

--pct 0 times the plain context alone and sets no option (the form that also runs on a commit without the option).  Compare
commits with that form: beside a second context in the process the same call took 1 % longer (two contexts' buffers share
the caches), which is why the ratio is taken inside one process and never across the two forms.
Prints one JSON line; --out also writes it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from computeraytracer_amd import Renderer, _lib  # noqa: E402
from computeraytracer_amd.scene import orbit_cameras  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "p90_ms": round(float(np.percentile(ts, 90)), 4)}


def clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--pct", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ps = atrium250k(a.width, a.height)
    cams = orbit_cameras(ps.camera, 64)
    ctx = {}
    for name, pct in (("clip", a.pct), ("plain", 0)):
        if name == "clip" and not a.pct:
            continue
        r = Renderer(0)
        r.upload(ps).build_accel("bvh2")
        if pct:
            r.set_option("temporal_clip_pct", pct)
        r.set_camera(cams[0]).frame(a.spp).sync()
        r.denoise_temporal()
        r.set_camera(cams[1]).set_sample_offset(a.spp).frame(a.spp).sync()
        _, hw = r.denoise_temporal(history=True)
        ctx[name] = (r, float((hw > a.spp).mean()))
    d = _lib.denoise_temporal_defaults()
    t5 = _lib.DenoiseTemporalParams(5, d.sigma_color, d.sigma_normal, d.sigma_plane, d.max_history, d.normal_tol, d.plane_tol)
    calls = {k: (lambda r=r: r._chk(r._lib.crt_denoise_temporal(r._h, C.byref(t5), None, None, None))) for k, (r, _) in ctx.items()}
    ts = {k: [] for k in calls}
    for i in range(10 + a.reps):                                # alternately: what shares the machine hits both alike
        for k, fn in calls.items():
            t = clock(fn)
            if i >= 10:
                ts[k].append(t)
    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "spp": a.spp, "reps": a.reps, "pct": a.pct,
           "reused_pixels": {k: round(v, 4) for k, (_, v) in ctx.items()}}
    for k in ts:
        res[k] = {"k5_compute": summary(ts[k])}
    half = len(ts["plain"]) // 2
    res["spread"] = round(abs(statistics.median(ts["plain"][:half]) - statistics.median(ts["plain"][half:]))
                          / statistics.median(ts["plain"]), 4)
    if "clip" in ts:
        box = ctx["clip"][0].debug_read_clip_box()
        res["valid_boxes"] = round(float((box[..., 7] == 1).mean()), 4)
        res["k5_ratio"] = round(res["clip"]["k5_compute"]["median_ms"] / res["plain"]["k5_compute"]["median_ms"], 4)
    for r, _ in ctx.values():
        r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
