"""The feature planes on S2 (atrium250k) at 1920 x 1080, one context of one build, host clock around each call:

  aov_all    crt_render_aovs, all five planes, n = 1, 16, 64 (the call reads 44 bytes per pixel back into pageable memory)
  aov_alpha  crt_render_aovs, the alpha plane alone, the same n (4 bytes per pixel: the kernel with little else)
  gbuffer    crt_read_gbuffer where it has to build the G-buffer first (crt_set_camera with the same camera drops it; one
             camera ray per pixel, 32 bytes per pixel read back)
  trace      crt_trace(n) + crt_sync from crt_reset, the same n: the beauty render the planes accompany

Each is the median of --reps calls after --warmup.  Kernel times come from a separate run of this script under a
kernel trace.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from computeraytracer_amd import Renderer  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ps = atrium250k(a.width, a.height)
    r = Renderer(0)
    r.upload(ps).build_accel("bvh2")
    rays = a.width * a.height

    def timed(fn, before=None):
        ms = []
        for k in range(a.warmup + a.reps):
            if before:
                before()
            t = time.perf_counter()
            fn()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t) * 1e3)
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "reps": a.reps, "warmup": a.warmup,
           "aov_all": {}, "aov_alpha": {}, "trace": {}}
    r.frame(1).sync()
    for n in a.samples:
        res["aov_all"][str(n)] = timed(lambda: r.render_aovs(n))
        res["aov_alpha"][str(n)] = timed(lambda: r.render_aovs(n, planes=("alpha",)))
    res["gbuffer"] = timed(r.read_gbuffer, before=lambda: r.set_camera(ps.camera).frame(1).sync())
    res["gbuffer_kept"] = timed(r.read_gbuffer)                  # the readback alone: the G-buffer is there
    for n in a.samples:
        res["trace"][str(n)] = timed(lambda: r.frame(n).sync(), before=lambda: r.reset().sync())
    gb = max(res["gbuffer"]["median_ms"] - res["gbuffer_kept"]["median_ms"], 0.0)
    res["gbuffer_build_ms"] = round(gb, 4)
    res["ns_per_camera_ray"] = {"gbuffer_build": round(gb * 1e6 / rays, 4),
                                "aov_alpha": {str(n): round(res["aov_alpha"][str(n)]["median_ms"] * 1e6 / (rays * n), 4) for n in a.samples}}
    res["aov_all_share_of_trace"] = {str(n): round(res["aov_all"][str(n)]["median_ms"] / res["trace"][str(n)]["median_ms"], 4)
                                     for n in a.samples}
    res["aov_alpha_share_of_trace"] = {str(n): round(res["aov_alpha"][str(n)]["median_ms"] / res["trace"][str(n)]["median_ms"], 4)
                                       for n in a.samples}
    r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
