"""crt_denoise_temporal with option "temporal_motion" on S2 (atrium250k) at 1920 x 1080: two contexts in one
process render the same two frames of --spp samples with distinct samples.  In the first the option is on and a tenth of
the triangles (the block of tests/test_scene_edit_gpu.py's test_s2_rigid_move_of_a_tenth) is moved rigidly between the
frames, so the second frame's blend runs k_dn_reproject<true> against the geometry snapshot; in the second the option is
off and nothing is edited.  Then the host clock around the synchronous call on the second frame, warm, the two contexts
alternately, median of --reps.  Calls within one frame blend against the same previous slot: every repetition does the
same work.

  motion.k5_compute     K = 5 with the map, no outputs requested (the launches and the sync alone)
  plain.k5_compute      the same call, option off, no edit
  k5_ratio              motion.k5_compute / plain.k5_compute (medians); DESIGN.md 6f expects <= 1.15
  read_motion           crt_read_motion with the map (kernel, 16 MB readback, sync)
  update_primitives     crt_update_primitives of the moved block with the option on (the first takes the 20 MB snapshot:
                        allocation and device-to-device copy) and off, host clock around the call, median of --edits;
                        refit_accel next to it, as tools/refit_bench.py times it

Prints one JSON line; --out also writes it."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from computeraytracer_amd import Renderer, _lib  # noqa: E402
from computeraytracer_amd.scene import transform_records  # noqa: E402
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
    ap.add_argument("--edits", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ps = atrium250k(a.width, a.height)
    n = len(ps.primitives)
    tri = np.flatnonzero(ps.primitives["category"] == 2)
    first, cnt = int(tri[len(tri) // 3]), n // 10
    ang = math.radians(3.0)
    R = [[math.cos(ang), 0.0, math.sin(ang)], [0.0, 1.0, 0.0], [-math.sin(ang), 0.0, math.cos(ang)]]
    block = ps.primitives[first:first + cnt]
    moved = transform_records(block, R, (4.0, 2.0, -3.0))
    ctx = {}
    for name, on in (("motion", 1), ("plain", 0)):
        r = Renderer(0)
        r.upload(ps).build_accel("bvh2").set_option("temporal_motion", on)
        r.frame(a.spp).sync()
        r.denoise_temporal()
        if on:
            r.update_primitives(first, moved)
            r.refit_accel()
        else:
            r.reset()
        r.set_sample_offset(a.spp).frame(a.spp).sync()
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
    rm = ctx["motion"][0]
    uv = rm.read_motion()
    t_uv = [clock(rm.read_motion) for _ in range(a.reps)]
    idx = np.ascontiguousarray(rm.read_gbuffer()[..., 7]).view(np.uint32)
    on_moved = (idx >= first) & (idx < first + cnt)
    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "spp": a.spp, "reps": a.reps,
           "moved_primitives": cnt, "pixels_on_moved_primitives": round(float(on_moved.mean()), 4),
           "positions": round(float((~np.isnan(uv[..., 0])).mean()), 4),
           "reused_pixels": {k: round(v, 4) for k, (_, v) in ctx.items()},
           "motion": {"k5_compute": summary(ts["motion"])}, "plain": {"k5_compute": summary(ts["plain"])},
           "read_motion": summary(t_uv)}
    res["k5_ratio"] = round(res["motion"]["k5_compute"]["median_ms"] / res["plain"]["k5_compute"]["median_ms"], 4)
    # the edit itself: with the option on every round starts from a fresh history slot, so every update takes a snapshot
    edit = {"on": [], "off": [], "refit": []}
    for i in range(a.edits):
        for name, key in (("motion", "on"), ("plain", "off")):
            r = ctx[name][0]
            r.frame(1).sync()
            r.denoise_temporal(0)
            edit[key].append(clock(lambda: r.update_primitives(first, moved if i % 2 == 0 else block)))
            t = clock(r.refit_accel)
            if key == "on":
                edit["refit"].append(t)
    res["update_primitives"] = {"option_on": summary(edit["on"]), "option_off": summary(edit["off"]),
                                "snapshot_bytes": n * 80, "refit_accel": summary(edit["refit"])}
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
