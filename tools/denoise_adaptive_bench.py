"""crt_denoise_adaptive on S2 (atrium250k) at 1920 x 1080 after an adaptive run to the defaults of DESIGN.md 6c, next to
crt_denoise on a uniform render of the same scene and size in the same process: host clock around the synchronous
call, warm, median of --reps.

  adaptive.k5_compute   K = 5, no outputs requested (the launches and the sync alone)
  adaptive.k5_pinned    K = 5, rgba8 into page-locked memory
  adaptive.k0_pinned    K = 0, rgba8 into page-locked memory
  uniform.*             the same three for crt_denoise (--uniform-spp samples)

--quality instead measures S2 at 480 x 270: four rounds of trace_adaptive(samples=16, min_samples=16, max_samples=64,
threshold = median of the errors after the first round), MSE in display space T of the noisy per-tile average, the
plain filter (tests/denoise_ref.py, 6a's defaults, on that average) and the variance-guided filter, for sigma_variance
in --sigmas, against --converged-spp samples of the same context.

Per-kernel times come from a separate run under rocprofv3 --kernel-trace --stats (k_dn_prepare_as, k_dn_vblur,
k_dn_atrous_as, k_dn_atrous).  Prints one JSON line; --out also writes it."""
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
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402


def timed(fn, reps):
    for _ in range(10):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4),
            "p90_ms": round(float(np.percentile(ts, 90)), 4)}


def speed(a):
    r = Renderer(0)
    r.upload(atrium250k(a.width, a.height)).build_accel("bvh2")
    lib, h = r._lib, r._h
    rgba = np.empty((a.height, a.width, 4), np.uint8)
    r._chk(lib.crt_pin_host(rgba.ctypes.data, rgba.nbytes))
    rounds = 0
    while r.trace_adaptive():                                  # the library's defaults (crt_adaptive_defaults)
        rounds += 1
    counts, _ = r.read_adaptive()
    d = _lib.denoise_adaptive_defaults()
    a5 = _lib.DenoiseAdaptiveParams(5, d.sigma_variance, d.sigma_normal, d.sigma_plane)
    a0 = _lib.DenoiseAdaptiveParams(0, d.sigma_variance, d.sigma_normal, d.sigma_plane)

    def call_a(p, out):
        r._chk(lib.crt_denoise_adaptive(h, C.byref(p), None, out, None))
    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "reps": a.reps,
           "adaptive_run": {"rounds": rounds, "tile_min": int(counts.min()), "tile_median": float(np.median(counts)),
                            "tile_max": int(counts.max())}}
    t0 = time.perf_counter()
    call_a(a5, rgba.ctypes.data)
    res["adaptive"] = {"first_call_ms": round((time.perf_counter() - t0) * 1e3, 4),
                       "k5_compute": timed(lambda: call_a(a5, None), a.reps),
                       "k5_pinned": timed(lambda: call_a(a5, rgba.ctypes.data), a.reps),
                       "k0_pinned": timed(lambda: call_a(a0, rgba.ctypes.data), a.reps)}
    r.reset().frame(a.uniform_spp).sync()
    u5, u0 = _lib.DenoiseParams(5, 1.0, 0.5, 0.3), _lib.DenoiseParams(0, 1.0, 0.5, 0.3)

    def call_u(p, out):
        r._chk(lib.crt_denoise(h, C.byref(p), None, out))
    call_u(u5, rgba.ctypes.data)
    res["uniform"] = {"spp": a.uniform_spp,
                      "k5_compute": timed(lambda: call_u(u5, None), a.reps),
                      "k5_pinned": timed(lambda: call_u(u5, rgba.ctypes.data), a.reps),
                      "k0_pinned": timed(lambda: call_u(u0, rgba.ctypes.data), a.reps)}
    res["k5_compute_ratio"] = round(res["adaptive"]["k5_compute"]["median_ms"] / res["uniform"]["k5_compute"]["median_ms"], 4)
    r._chk(lib.crt_unpin_host(rgba.ctypes.data))
    r.close()
    return res


def quality(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import denoise_ref as ref
    w, hgt = 480, 270
    ps = atrium250k(w, hgt)
    r = Renderer(0)
    r.upload(ps).build_accel("bvh2").frame(1).sync()
    g = r.read_gbuffer()
    r.reset()
    r.trace_adaptive(samples=16, threshold=0.0, min_samples=16, max_samples=64)
    _, errors = r.read_adaptive()
    thr = float(np.median(errors))
    for _ in range(3):
        r.trace_adaptive(samples=16, threshold=thr, min_samples=16, max_samples=64)
    counts, _ = r.read_adaptive()
    npx = np.repeat(np.repeat(counts, 8, 0), 8, 1)[:hgt, :w]
    noisy = (r.read_accum().astype(np.float64)[..., :3] / npx[..., None]) @ ref.M.T
    guided = {s: r.denoise_adaptive(sigma_variance=s, rgb=True)[1][..., :3] for s in a.sigmas}
    plain = ref.atrous_gbuffer(noisy, g, ps.primitives)
    r.reset().frame(a.converged_spp).sync()
    conv = ref.linear_rgb(r.read_accum(), a.converged_spp)
    r.close()
    return {"scene": "S2 atrium250k", "width": w, "height": hgt, "converged_spp": a.converged_spp,
            "mean_spp": round(float(npx.mean()), 2), "threshold": thr,
            "tiles_at": {int(k): int(v) for k, v in zip(*np.unique(counts, return_counts=True))},
            "mse_noisy": ref.mse_display(noisy, conv), "mse_plain": ref.mse_display(plain, conv),
            "mse_variance_guided": {str(s): ref.mse_display(c, conv) for s, c in guided.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--uniform-spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--sigmas", type=float, nargs="+", default=[2.0, 4.0, 8.0, 16.0])
    ap.add_argument("--converged-spp", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(quality(a) if a.quality else speed(a))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
