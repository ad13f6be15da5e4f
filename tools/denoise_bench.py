"""crt_denoise on S2 (atrium250k) at 1920 x 1080: host clock around the synchronous call, warm, median of --reps.

  first        the first call after the render: G-buffer + filter + rgba8 readback
  k5_compute   K = 5, no outputs requested (the launches and the sync alone)
  k5_pinned    K = 5, rgba8 into page-locked memory
  k5_pageable  K = 5 through Renderer.denoise (numpy, pageable)
  k0_pinned    K = 0, rgba8 into page-locked memory (what the filter passes add: k5_pinned - k0_pinned)

Per-kernel times come from a separate run under rocprofv3 --kernel-trace --stats (k_dn_gbuffer, k_dn_prepare,
k_dn_atrous).  Prints one JSON line; --out also writes it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from computeraytracer_amd import Renderer, _lib  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = Renderer(0)
    r.upload(atrium250k(a.width, a.height)).build_accel("bvh2").frame(a.spp).sync()
    lib, h = r._lib, r._h
    n = a.width * a.height
    rgba = np.empty((a.height, a.width, 4), np.uint8)
    r._chk(lib.crt_pin_host(rgba.ctypes.data, rgba.nbytes))
    p5, p0 = _lib.DenoiseParams(5, 1.0, 0.5, 0.3), _lib.DenoiseParams(0, 1.0, 0.5, 0.3)

    def call(p, out):
        r._chk(lib.crt_denoise(h, C.byref(p), None, out))

    t0 = time.perf_counter()
    call(p5, rgba.ctypes.data)
    first = (time.perf_counter() - t0) * 1e3

    def timed(fn):
        for _ in range(10):
            fn()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4),
                "p90_ms": round(float(np.percentile(ts, 90)), 4)}

    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "spp": a.spp, "reps": a.reps,
           "first_call_ms": round(first, 4),
           "k5_compute": timed(lambda: call(p5, None)),
           "k5_pinned": timed(lambda: call(p5, rgba.ctypes.data)),
           "k0_pinned": timed(lambda: call(p0, rgba.ctypes.data)),
           "k5_pageable": timed(lambda: r.denoise(5)),
           "tap_loads_per_iteration_M": round(25 * n / 1e6, 1)}
    r._chk(lib.crt_unpin_host(rgba.ctypes.data))
    r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
