"""The radiance queries on S2 (atrium250k), one context of one build, the device form on torch's current
stream timed with torch events:

  panorama  a 2048 x 1024 equirectangular view from the middle of the atrium's box (Renderer.panorama_rays)
  camera    one ray per pixel of the context's 1920 x 1080 camera: from the eye towards what the pixel's camera ray of
            sample 8 hits (crt_pick's position; a pixel that sees nothing looks straight ahead), key (x, y, 1).  These
            are NOT the rays crt_trace draws for the same pixels -- it jitters each sample's ray, here one fixed ray per
            pixel is traced --samples times -- so the ratio to crt_trace compares the same pixels and scene content, not
            the same paths

each at --samples paths per ray.  Reported: the median, minimum and maximum of --reps launches after --warmup, and PATHS
per second (rays x samples / time) -- not rays as crt_counters counts them: the kernel keeps no counters.  For the camera
set also crt_trace's wall time for the same number of samples (reset, trace, sync), the pipeline's own paths per second
and, from crt_counters, its rays per path.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from computeraytracer_amd import Renderer  # noqa: E402
from computeraytracer_amd.renderer import pack_keys, pack_rays  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pano", default="2048x1024")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--accel", default="bvh2")
    ap.add_argument("--no-trace", action="store_true", help="leave crt_trace's time out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    ps = atrium250k(a.width, a.height)
    r = Renderer(0)
    r.upload(ps).build_accel(a.accel)
    dev = torch.device(f"cuda:{r.device}")
    p = ps.primitives
    tri = p["category"] == 2
    pts = np.concatenate([p["data1"], (p["data1"] + p["data2"])[tri], (p["data1"] + p["data3"])[tri]])
    lo, hi = pts.min(0), pts.max(0)
    pw, ph = (int(v) for v in a.pano.split("x"))
    sets = {"panorama": Renderer.panorama_rays(pw, ph, ((lo + hi) / 2).astype(np.float32))}
    eye = ps.camera[0:3].astype(np.float32)
    xs, ys = np.meshgrid(np.arange(a.width), np.arange(a.height))
    seen = r.pick_pixels(np.stack([xs.ravel(), ys.ravel()], 1), planes=("hit", "position"))
    d = seen["position"][:, :3] - eye
    d[seen["hit"] == 0] = (ps.camera[4:7] - eye).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    sets["camera"] = (pack_rays(np.tile(eye, (len(d), 1)), d), pack_keys(xs.ravel(), ys.ravel(), 1))
    res = {"scene": "S2 atrium250k", "accel": a.accel, "samples": a.samples, "reps": a.reps, "warmup": a.warmup,
           "lanes": r.radiance_lanes(1 << 30), "lib": os.path.basename(os.environ.get("CRT_LIB") or "libcrt.so")}
    for name, (rays, keys) in sets.items():
        n = len(rays)
        t_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to(dev)
        t_keys = torch.from_numpy(keys.view(np.uint32).reshape(-1, 4).view(np.int32).copy()).to(dev)
        ms = []
        for k in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = r.radiance_rays(rays=t_rays, keys=t_keys, n_samples=a.samples, planes=("xyz",))
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        res[name] = {"rays": n, "hit_rate": round(float(r.query_rays(rays=rays, planes=("hit",))["hit"].mean()), 4),
                     "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                     "mpaths_per_s": round(n * a.samples / med / 1e3, 2), "mean_Y": round(float(out["xyz"][:, 1].mean()) / a.samples, 5)}
    if not a.no_trace:
        r.enable_counters(False)
        ms = []
        for k in range(a.warmup + a.reps):
            r.reset()
            r.sync()
            t = time.perf_counter()
            r.frame(a.samples)
            r.sync()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t) * 1e3)
        med = statistics.median(ms)
        n = a.width * a.height
        r.enable_counters(True)
        r.reset()
        r.reset_counters()
        r.frame(1)
        r.sync()
        c = r.counters()
        res["crt_trace"] = {"paths": n * a.samples, "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                            "mpaths_per_s": round(n * a.samples / med / 1e3, 2), "rays_per_path": round(c["rays"] / max(1, c["paths"]), 3)}
        res["camera"]["over_crt_trace"] = round(res["camera"]["median_ms"] / med, 3)
    r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
