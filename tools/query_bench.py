"""The ray queries on S2 (atrium250k) at 1920 x 1080, one context of one build, host clock around each call:

  camera      2 073 600 coherent rays, one per pixel: from the eye towards what the pixel's camera ray of sample 8 hits
              (crt_pick's position; a pixel that sees nothing looks straight ahead)
  incoherent  as many rays with seeded numpy origins uniform in the scene box and uniform directions

Per set: crt_query_rays (host form, all planes and `hit` alone), crt_query_rays_device (torch tensors, the call plus a
stream synchronise), crt_debug_intersect on the same rays, Mrays/s of each, and ANY against CLOSEST at t_max = the scene
diagonal.  Each is the median of --reps calls after --warmup.  k_query's kernel time comes from a separate run of this
script under a kernel trace.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from computeraytracer_amd import Renderer  # noqa: E402
from computeraytracer_amd.renderer import pack_rays  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--accel", default="bvh2")
    ap.add_argument("--no-debug", action="store_true", help="leave crt_debug_intersect out (a kernel-trace run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    ps = atrium250k(a.width, a.height)
    r = Renderer(0)
    r.upload(ps).build_accel(a.accel)
    n = a.width * a.height

    def timed(fn):
        ms = []
        for k in range(a.warmup + a.reps):
            t = time.perf_counter()
            fn()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t) * 1e3)
        med = statistics.median(ms)
        return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "mrays_per_s": round(n / med / 1e3, 2)}

    # the scene box and its diagonal, from the records
    p = ps.primitives
    tri = p["category"] == 2
    pts = np.concatenate([p["data1"], (p["data1"] + p["data2"])[tri], (p["data1"] + p["data3"])[tri]])
    lo, hi = pts.min(0), pts.max(0)
    diag = float(np.linalg.norm(hi - lo))
    eye = ps.camera[0:3].astype(np.float32)
    # the camera rays: towards what each pixel's pick sees (a pixel that sees nothing: straight ahead)
    xs, ys = np.meshgrid(np.arange(a.width), np.arange(a.height))
    seen = r.pick_pixels(np.stack([xs.ravel(), ys.ravel()], 1), planes=("hit", "position"))
    d = seen["position"][:, :3] - eye
    d[seen["hit"] == 0] = (ps.camera[4:7] - eye).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rng = np.random.default_rng(20261021)
    sets = {"camera": (np.tile(eye, (n, 1)), d),
            "incoherent": (rng.uniform(lo, hi, (n, 3)).astype(np.float32),
                           (lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3))))}
    res = {"scene": "S2 atrium250k", "accel": a.accel, "width": a.width, "height": a.height, "rays": n, "reps": a.reps, "warmup": a.warmup,
           "scene_diagonal": round(diag, 3)}
    dev = torch.device(f"cuda:{r.device}")
    for name, (o, dd) in sets.items():
        rays = pack_rays(o, dd)
        near = pack_rays(o, dd, t_max=np.float32(diag))
        t_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to(dev)
        t_near = torch.from_numpy(near.view(np.float32).reshape(-1, 8).copy()).to(dev)

        def device(t, mode="closest", planes=None):
            r.query_rays(rays=t, mode=mode, planes=planes)
            torch.cuda.current_stream(dev).synchronize()
        s = {"hit_rate": round(float(r.query_rays(rays=rays, planes=("hit",))["hit"].mean()), 4),
             "host_all_planes": timed(lambda: r.query_rays(rays=rays)),
             "host_hit_only": timed(lambda: r.query_rays(rays=rays, planes=("hit",))),
             "device_all_planes": timed(lambda: device(t_rays)),
             "device_closest_hit_only_diag": timed(lambda: device(t_near, "closest", ("hit",))),
             "device_any_diag": timed(lambda: device(t_near, "any"))}
        s["any_over_closest"] = round(s["device_any_diag"]["median_ms"] / s["device_closest_hit_only_diag"]["median_ms"], 4)
        if not a.no_debug:
            s["debug_intersect"] = timed(lambda: r.debug_intersect(o, dd))
        res[name] = s
    r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
