"""The filtered display loop on S2 (atrium250k) at 1920 x 1080: one crt_trace(1) per displayed frame, K = 5,
rgba8 into page-locked memory.  Five loops on one context of one build:

  a  no read                         the trace calls alone
  b  crt_read_latest_rgba8           the unfiltered display loop that does not stop the pipeline
  c  crt_denoise                     the only filtered loop without crt_denoise_latest: a flush per frame
  d  crt_denoise_latest, 256 lanes   option "denoise_latest_wave_blocks" = 0 (k_dn_atrous, 16 x 16 pixels per block)
  e  crt_denoise_latest, 64 lanes    option "denoise_latest_wave_blocks" = 1 (k_dn_atrous_w64, 8 x 8 pixels per block)

A repetition runs the five loops one after the other (so they alternate), each from crt_reset for --frames frames and then
crt_sync.  Per loop: the host time of every frame after the first --warmup of its run (median, min, p90 over all
repetitions), and per run the samples completed per second = frames / (time from the first crt_trace to the end of the
closing crt_sync).  d and e also report how far the frame shown lags the frame requested.
Prints one JSON line; --out also writes it."""
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
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = Renderer(0)
    r.upload(atrium250k(a.width, a.height)).build_accel("bvh2")
    lib, h = r._lib, r._h
    frame = np.zeros((a.height, a.width, 4), np.uint8)
    r._chk(lib.crt_pin_host(frame.ctypes.data, frame.nbytes))
    p = _lib.DenoiseParams(a.iterations, 1.0, 0.5, 0.3)
    s = C.c_uint32()
    lag = {"d": [], "e": []}

    def latest(k):
        rc = lib.crt_denoise_latest(h, C.byref(p), None, frame.ctypes.data, C.byref(s))
        if rc == -3 and s.value == 0:                            # no complete frame yet
            return None
        r._chk(rc)
        return k - s.value

    loops = {
        "a": lambda k: None,
        "b": lambda k: r._chk(lib.crt_read_latest_rgba8(h, frame.ctypes.data, C.byref(s))),
        "c": lambda k: r._chk(lib.crt_denoise(h, C.byref(p), None, frame.ctypes.data)),
        "d": latest,
        "e": latest,
    }
    # the five loops show the same thing where they show the same sample
    r.frame(4).sync()
    r.set_option("denoise_latest_wave_blocks", 0)
    latest(4)
    shown = [frame.copy()]
    r.set_option("denoise_latest_wave_blocks", 1)
    latest(4)
    shown.append(frame.copy())
    loops["c"](4)
    same = bool(np.array_equal(shown[0], frame) and np.array_equal(shown[1], frame))

    ms = {k: [] for k in loops}
    rate = {k: [] for k in loops}
    for rep in range(a.reps + 1):                                # (repetition 0 warms everything up and is dropped)
        for name, fn in loops.items():
            if name in ("d", "e"):
                r.set_option("denoise_latest_wave_blocks", 1 if name == "e" else 0)
            r.reset().sync()
            t_run = time.perf_counter()
            for k in range(1, a.frames + 1):
                t = time.perf_counter()
                r._chk(lib.crt_trace(h, 1))
                behind = fn(k)
                dt = (time.perf_counter() - t) * 1e3
                if rep and k > a.warmup:
                    ms[name].append(dt)
                    if name in lag and behind is not None:
                        lag[name].append(behind)
            r.sync()
            if rep:
                rate[name].append(a.frames / (time.perf_counter() - t_run))

    def stats(v, digits=4):
        return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "p90": round(float(np.percentile(v, 90)), digits),
                "max": round(max(v), digits)}

    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "iterations": a.iterations, "frames_per_run": a.frames,
           "warmup_frames": a.warmup, "reps": a.reps, "timed_frames_per_loop": len(ms["a"]), "same_image_for_the_same_sample": same,
           "loops": {"a": "no read", "b": "crt_read_latest_rgba8", "c": "crt_denoise", "d": "crt_denoise_latest, 256-lane passes",
                     "e": "crt_denoise_latest, 64-lane passes"}}
    for name in loops:
        res[name] = {"ms_per_frame": stats(ms[name]), "samples_per_s": stats(rate[name], 1)}
        if name in lag:
            res[name]["frames_behind"] = stats(lag[name], 1)
    base = res["a"]["samples_per_s"]["median"]
    for name in "bcde":
        res[name]["trace_rate_vs_a"] = round(res[name]["samples_per_s"]["median"] / base, 4)
    r._chk(lib.crt_unpin_host(frame.ctypes.data))
    r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
