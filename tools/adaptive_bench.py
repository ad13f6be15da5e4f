"""Adaptive sampling (include/crt.h "Adaptive sampling") on S2 (atrium250k) and the Cornell box at
1920 x 1080: host clock around synchronous calls, warm.

  overhead   ms per call of an all-tiles-active crt_trace_adaptive(n) + crt_sync against crt_trace(n) + crt_sync, n = 16, 64
             (median of --reps), and their ratio
  select_ms  crt_read_adaptive (k_as_select over every tile + the count / error readback), median of --reps
  payoff     per tau and per step (samples per round): rounds, pixel-samples and seconds until every tile has E <= tau
             (or holds --max samples), adaptive (min_samples --min) against the control -- every tile active every round
             (min_samples = max_samples), stopped once its worst tile reaches tau -- and the wall-time ratio

Kernel times (k_as_select, k_as_compact, the sampling kernels) come from a separate run under rocprofv3 --kernel-trace
--stats (--quick keeps it short).  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from computeraytracer_amd import Renderer, cornell  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402

ALL = dict(threshold=3.0e38, min_samples=0xFFFFFFFF, max_samples=0)      # every tile active


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 4)


def pixel_samples(counts, w, h):
    return int(np.repeat(np.repeat(counts.astype(np.int64), 8, 0), 8, 1)[:h, :w].sum())


def run_adaptive(r, w, h, tau, step, mn, mx):
    r.reset()
    t0 = time.perf_counter()
    rounds = 0
    while r.trace_adaptive(samples=step, threshold=tau, min_samples=mn, max_samples=mx):
        rounds += 1
    r.sync()
    dt = time.perf_counter() - t0
    counts, errors = r.read_adaptive()
    return dict(rounds=rounds, pixel_samples=pixel_samples(counts, w, h), seconds=round(dt, 4),
                tile_min=int(counts.min()), tile_median=float(np.median(counts)), tile_max=int(counts.max()),
                worst_E=float(errors.max()), at_max=int((counts >= mx).sum()))


def run_control(r, w, h, tau, step, mx):
    r.reset()
    t0 = time.perf_counter()
    rounds = 0
    while r.trace_adaptive(samples=step, threshold=tau, min_samples=mx, max_samples=mx):
        rounds += 1
        counts, errors = r.read_adaptive()                    # the stop test: the worst tile
        if float(errors.max()) <= tau:
            break
    r.sync()
    dt = time.perf_counter() - t0
    counts, errors = r.read_adaptive()
    return dict(rounds=rounds, pixel_samples=pixel_samples(counts, w, h), seconds=round(dt, 4), spp=int(counts.max()),
                worst_E=float(errors.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="s2,cornell")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--taus", default="0.01,0.005")
    ap.add_argument("--steps", default="16,64")
    ap.add_argument("--min", type=int, default=32)
    ap.add_argument("--max", type=int, default=4096)
    ap.add_argument("--quick", action="store_true", help="S2 overhead and one adaptive run at the first tau (profiling)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = a.width, a.height
    taus = [float(t) for t in a.taus.split(",")]
    steps = [int(s) for s in a.steps.split(",")]
    scenes = {"s2": lambda: atrium250k(w, h), "cornell": lambda: cornell(w, h)}
    names = ["s2"] if a.quick else a.scenes.split(",")
    out = dict(width=w, height=h, min_samples=a.min, max_samples=a.max, scenes={})
    with Renderer(0) as r:
        for name in names:
            r.upload(scenes[name]()).build_accel("bvh2")
            res = dict(overhead={})
            for n in (16, 64):
                r.reset()
                un = timed(lambda: r.frame(n).sync(), a.reps)
                r.reset()
                ad = timed(lambda: (r.trace_adaptive(samples=n, **ALL), r.sync()), a.reps)
                res["overhead"][str(n)] = dict(trace_ms=un, adaptive_ms=ad, ratio=round(ad / un, 4))
            res["select_ms"] = timed(r.read_adaptive, a.reps)
            res["payoff"] = {}
            for tau in (taus[:1] if a.quick else taus):
                for step in (steps[:1] if a.quick else steps):
                    ad = run_adaptive(r, w, h, tau, step, a.min, a.max)
                    key = f"tau={tau},step={step}"
                    if a.quick:
                        res["payoff"][key] = dict(adaptive=ad)
                        continue
                    ct = run_control(r, w, h, tau, step, a.max)
                    res["payoff"][key] = dict(adaptive=ad, control=ct, time_ratio=round(ad["seconds"] / ct["seconds"], 4),
                                              pixel_sample_ratio=round(ad["pixel_samples"] / ct["pixel_samples"], 4))
            r.reset()
            out["scenes"][name] = res
            print(json.dumps({name: res}), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
