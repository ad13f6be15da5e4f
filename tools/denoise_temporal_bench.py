"""crt_denoise_temporal on S2 (atrium250k) at 1920 x 1080 next to crt_denoise in the same process, timed alternately:
two orbit frames of --spp samples (1/64 turn apart, distinct samples), then on the second frame the host clock around
the synchronous call, warm, median of --reps.  Calls within one frame blend against the same previous slot, so every
repetition does the same work.

  temporal.k5_compute   K = 5, no outputs requested (the launches and the sync alone)
  temporal.k0_compute   K = 0: k_dn_reproject alone
  plain.k5_compute      crt_denoise, K = 5
  k5_ratio              temporal.k5_compute / plain.k5_compute (medians)

--sweep instead measures quality: an orbit of --frames frames of --spp samples, 1/--turn of a turn apart, on the Cornell
box 64 x 64 and on S2 at 480 x 270; MSE in display space T of the last frame's crt_denoise_temporal (K = 5) over that of
crt_denoise on the same frame, against --converged-spp samples, for max_history, normal_tol and plane_tol varied one
at a time around the defaults.

Per-kernel times come from a separate run of the default mode under rocprofv3 --kernel-trace --stats (k_dn_reproject,
k_dn_atrous).  Prints one JSON line; --out also writes it."""
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

from computeraytracer_amd import Renderer, _lib, cornell  # noqa: E402
from computeraytracer_amd.scene import orbit_cameras  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "p90_ms": round(float(np.percentile(ts, 90)), 4)}


def speed(a):
    ps = atrium250k(a.width, a.height)
    cams = orbit_cameras(ps.camera, a.turn)
    r = Renderer(0)
    r.upload(ps).build_accel("bvh2")
    lib, h = r._lib, r._h
    for k in range(2):
        r.set_camera(cams[k]).set_sample_offset(k * a.spp).frame(a.spp).sync()
        _, hw = r.denoise_temporal(history=True)
    d = _lib.denoise_temporal_defaults()
    t5 = _lib.DenoiseTemporalParams(5, d.sigma_color, d.sigma_normal, d.sigma_plane, d.max_history, d.normal_tol, d.plane_tol)
    t0 = _lib.DenoiseTemporalParams(0, d.sigma_color, d.sigma_normal, d.sigma_plane, d.max_history, d.normal_tol, d.plane_tol)
    p5 = _lib.DenoiseParams(5, d.sigma_color, d.sigma_normal, d.sigma_plane)
    calls = {"temporal_k5": lambda: r._chk(lib.crt_denoise_temporal(h, C.byref(t5), None, None, None)),
             "plain_k5": lambda: r._chk(lib.crt_denoise(h, C.byref(p5), None, None)),
             "temporal_k0": lambda: r._chk(lib.crt_denoise_temporal(h, C.byref(t0), None, None, None))}
    ts = {k: [] for k in calls}
    for i in range(10 + a.reps):                                # alternately: what shares the machine hits all three alike
        for k, fn in calls.items():
            t = time.perf_counter()
            fn()
            if i >= 10:
                ts[k].append((time.perf_counter() - t) * 1e3)
    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "spp": a.spp, "reps": a.reps,
           "reused_pixels": round(float((hw > a.spp).mean()), 4),
           "temporal": {"k5_compute": summary(ts["temporal_k5"]), "k0_compute": summary(ts["temporal_k0"])},
           "plain": {"k5_compute": summary(ts["plain_k5"])}}
    res["k5_ratio"] = round(res["temporal"]["k5_compute"]["median_ms"] / res["plain"]["k5_compute"]["median_ms"], 4)
    r.close()
    return res


def sweep(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import denoise_ref as ref
    d = _lib.denoise_temporal_defaults()
    base = dict(max_history=d.max_history, normal_tol=d.normal_tol, plane_tol=d.plane_tol)
    grid = [dict(base)]
    for name, values in (("max_history", a.max_history), ("normal_tol", a.normal_tol), ("plane_tol", a.plane_tol)):
        grid += [dict(base, **{name: v}) for v in values if v != base[name]]
    out = {"frames": a.frames, "spp": a.spp, "turn": a.turn, "converged_spp": a.converged_spp, "defaults": base, "scenes": {}}
    r = Renderer(0)
    for label, ps in (("cornell 64x64", cornell(64, 64)), ("S2 atrium250k 480x270", atrium250k(480, 270))):
        cams = orbit_cameras(ps.camera, a.turn)[:a.frames]
        r.upload(ps).build_accel("bvh2")
        r.set_camera(cams[-1]).set_sample_offset(100000).frame(a.converged_spp).sync()
        truth = ref.linear_rgb(r.read_accum(), a.converged_spp)
        rows = []
        for p in grid:
            r.temporal_reset()
            for k, cam in enumerate(cams):
                r.set_camera(cam).set_sample_offset(k * a.spp).frame(a.spp).sync()
                _, rgb, hw = r.denoise_temporal(rgb=True, history=True, **p)
            _, plain = r.denoise(rgb=True)
            noisy = ref.linear_rgb(r.read_accum(), a.spp)
            m = [ref.mse_display(x, truth) for x in (noisy, plain[..., :3], rgb[..., :3])]
            rows.append(dict(p, mse_noisy=m[0], mse_plain=m[1], mse_temporal=m[2], ratio=round(m[2] / m[1], 4),
                             reused_pixels=round(float((hw > a.spp).mean()), 4)))
        out["scenes"][label] = rows
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--turn", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--converged-spp", type=int, default=1024)
    ap.add_argument("--max-history", type=float, nargs="+", default=[8.0, 16.0, 32.0, 64.0, 128.0])
    ap.add_argument("--normal-tol", type=float, nargs="+", default=[0.1, 0.25, 0.5, 1.0])
    ap.add_argument("--plane-tol", type=float, nargs="+", default=[0.5, 1.0, 2.0, 4.0, 8.0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(sweep(a) if a.sweep else speed(a))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
