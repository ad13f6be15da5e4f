"""crt_denoise_svgf on S2 (atrium250k) at 1920 x 1080 next to crt_denoise_temporal in the same process, timed alternately:
--frames orbit frames of --spp samples (1/64 turn apart, distinct samples) filtered with crt_denoise_svgf, so that the last
one has history and moments behind it, then on that frame the host clock around the synchronous call, warm, median of
--reps.  Calls within one frame blend against the same previous slot, so every repetition does the same work; the
alternation also exercises the hand-over of CURRENT between the two calls.

  svgf.k5_compute       K = 5, no outputs requested (the launches and the sync alone)
  svgf.k0_compute       K = 0: k_dn_reproject<*, true> alone
  temporal.k5_compute   crt_denoise_temporal, K = 5
  k5_ratio              svgf.k5_compute / temporal.k5_compute (medians); DESIGN.md 6g accepts <= 1.5
  svgf.k5_compute_pP    with --spatial-pct P [P ...]: the K = 5 call under option "svgf_spatial_pct" = P, in the
                        same alternation; the option is set outside the timed region.  --frames 1 times the frame on which no
                        pixel's variance is known, --frames 8 a frame of the steady orbit

--sweep instead measures quality on S2 at 480 x 270: an orbit of --frames frames of --spp samples, 1/--turn of a turn
apart; MSE in display space T of the last frame's crt_denoise_svgf (K = 5) over that of crt_denoise_temporal on the same
frames, against --converged-spp samples, for sigma_variance x min_frames (x --spatial-pct, where given).

Per-kernel times come from a separate run of the default mode under rocprofv3 --kernel-trace --stats.  Prints one JSON
line; --out also writes it."""
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


def speed(a):
    ps = atrium250k(a.width, a.height)
    cams = orbit_cameras(ps.camera, a.turn)
    r = Renderer(0)
    r.upload(ps).build_accel("bvh2")
    lib, h = r._lib, r._h
    for k in range(a.frames):
        r.set_camera(cams[k]).set_sample_offset(k * a.spp).frame(a.spp).sync()
        _, hw, var = r.denoise_svgf(history=True, var=True)
    mom = r.read_moments()
    d, dt = _lib.denoise_svgf_defaults(), _lib.denoise_temporal_defaults()
    s5 = _lib.DenoiseSvgfParams(5, d.sigma_variance, d.sigma_normal, d.sigma_plane, d.max_history, d.normal_tol, d.plane_tol, d.min_frames)
    s0 = _lib.DenoiseSvgfParams(0, d.sigma_variance, d.sigma_normal, d.sigma_plane, d.max_history, d.normal_tol, d.plane_tol, d.min_frames)
    t5 = _lib.DenoiseTemporalParams(5, dt.sigma_color, dt.sigma_normal, dt.sigma_plane, dt.max_history, dt.normal_tol, dt.plane_tol)
    calls = {"svgf_k5": lambda: r._chk(lib.crt_denoise_svgf(h, C.byref(s5), None, None, None, None)),
             "temporal_k5": lambda: r._chk(lib.crt_denoise_temporal(h, C.byref(t5), None, None, None)),
             "svgf_k0": lambda: r._chk(lib.crt_denoise_svgf(h, C.byref(s0), None, None, None, None))}
    pct = {k: 0 for k in calls}
    for p in a.spatial_pct or []:
        calls[f"svgf_k5_p{p}"], pct[f"svgf_k5_p{p}"] = calls["svgf_k5"], p
    ts = {k: [] for k in calls}
    for i in range(10 + a.reps):                                # alternately: what shares the machine hits all of them alike
        for k, fn in calls.items():
            if a.spatial_pct:
                r.set_option("svgf_spatial_pct", pct[k])
            t = time.perf_counter()
            fn()
            if i >= 10:
                ts[k].append((time.perf_counter() - t) * 1e3)
    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "spp": a.spp, "frames": a.frames, "reps": a.reps,
           "reused_pixels": round(float((hw > a.spp).mean()), 4),
           "pixels_with_moments": round(float((mom[..., 2] > a.spp).mean()), 4),
           "pixels_with_known_variance": round(float((mom[..., 2] / np.float32(a.spp) >= d.min_frames).mean()), 4),
           "svgf": {"k5_compute": summary(ts["svgf_k5"]), "k0_compute": summary(ts["svgf_k0"])},
           "temporal": {"k5_compute": summary(ts["temporal_k5"])}}
    for p in a.spatial_pct or []:
        res["svgf"][f"k5_compute_p{p}"] = summary(ts[f"svgf_k5_p{p}"])
    res["k5_ratio"] = round(res["svgf"]["k5_compute"]["median_ms"] / res["temporal"]["k5_compute"]["median_ms"], 4)
    r.close()
    return res


def sweep(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import denoise_ref as ref
    ps = atrium250k(480, 270)
    cams = orbit_cameras(ps.camera, a.turn)[:a.frames]
    out = {"scene": "S2 atrium250k 480x270", "frames": a.frames, "spp": a.spp, "turn": a.turn, "converged_spp": a.converged_spp, "rows": []}
    r = Renderer(0)
    r.upload(ps).build_accel("bvh2")
    r.set_camera(cams[-1]).set_sample_offset(100000).frame(a.converged_spp).sync()
    truth = ref.linear_rgb(r.read_accum(), a.converged_spp)

    def orbit(call):
        r.temporal_reset()
        for k, cam in enumerate(cams):
            r.set_camera(cam).set_sample_offset(k * a.spp).frame(a.spp).sync()
            rgb = call()[1]
        return ref.mse_display(rgb[..., :3], truth)
    out["mse_blend"] = orbit(lambda: r.denoise_temporal(0, rgb=True))
    out["mse_temporal"] = orbit(lambda: r.denoise_temporal(rgb=True))
    for sv in a.sigma_variance:
        for mf in a.min_frames:
            for p in a.spatial_pct or [None]:
                if p is not None:
                    r.set_option("svgf_spatial_pct", p)
                m = orbit(lambda: r.denoise_svgf(sigma_variance=sv, min_frames=mf, rgb=True))
                row = {"sigma_variance": sv, "min_frames": mf, "mse_svgf": m, "ratio": round(m / out["mse_temporal"], 4)}
                out["rows"].append(row if p is None else dict(row, spatial_pct=p))
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--turn", type=int, default=64)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--converged-spp", type=int, default=1024)
    ap.add_argument("--sigma-variance", type=float, nargs="+", default=[1.0, 2.0, 4.0, 8.0])
    ap.add_argument("--min-frames", type=float, nargs="+", default=[2.0, 3.0, 4.0])
    ap.add_argument("--spatial-pct", type=int, nargs="+", default=None, metavar="P",
                    help="option svgf_spatial_pct: the values to time the K = 5 call under, or with --sweep to measure")
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
