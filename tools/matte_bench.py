"""The id mattes on S2 (atrium250k) at 1920 x 1080, one context of one build, host clock around each call:

  matte      crt_render_mattes, all four planes, n = 1, 16, 64, slots 4 and 16, sources primitive and object (the call reads
             (2 * slots + 2) * 4 bytes per pixel back into pageable memory)
  matte_hits crt_render_mattes, the hits plane alone, slots 4, source primitive (4 bytes per pixel: the kernel with little else)
  aov_alpha  crt_render_aovs, the alpha plane alone, the same n: the same walk without the table

Each is the median of --reps calls after --warmup.  Kernel times come from a separate run of this script under a
kernel trace (k_matte against k_aov).  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from computeraytracer_amd import Renderer  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k, atrium250k_object_ids  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--slots", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--sources", nargs="+", default=["primitive", "object"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ps = atrium250k(a.width, a.height)
    r = Renderer(0)
    r.upload(ps).build_accel("bvh2").set_primitive_ids(0, atrium250k_object_ids())

    def timed(fn):
        ms = []
        for k in range(a.warmup + a.reps):
            t = time.perf_counter()
            fn()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t) * 1e3)
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "reps": a.reps, "warmup": a.warmup,
           "matte": {}, "matte_hits": {}, "aov_alpha": {}, "overflow_pixels": {}}
    for n in a.samples:
        for source in a.sources:
            for slots in a.slots:
                key = f"{source}/slots{slots}/n{n}"
                res["matte"][key] = timed(lambda: r.render_mattes(n, source, slots))
                res["overflow_pixels"][key] = int((r.render_mattes(n, source, slots, planes=("overflow",))["overflow"] > 0).sum())
        res["matte_hits"][str(n)] = timed(lambda: r.render_mattes(n, "primitive", a.slots[0], planes=("hits",)))
        res["aov_alpha"][str(n)] = timed(lambda: r.render_aovs(n, planes=("alpha",)))
    r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
