"""crt_trace_adaptive_filtered next to crt_trace_adaptive on S2 (atrium250k), one GPU.

  selection   1920 x 1080, every tile at --round samples = max_samples, so a call is its selection step alone (the filter's
              launches, k_as_select_var, k_as_compact, the 4-byte readback; nothing is active): host clock around the
              call, warm, median of --reps, for both rules, next to one --round-sample round of every tile and to
              crt_denoise_adaptive's launches without outputs
  payoff      480 x 270, rounds of 16 samples from 16 to a cap of 256, for each rule and threshold: mean samples per pixel
              and the MSE in display space T of crt_denoise_adaptive's image against --converged-spp samples of the same
              context; and the fewest mean samples with which each rule reaches the old rule's MSE at threshold 0.05

k_as_select_var's own kernel time comes from a separate run under rocprofv3 --kernel-trace --stats (--kernel-only runs
just the calls for it).  Prints one JSON line; --out also writes it."""
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

from computeraytracer_amd import Renderer  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4),
            "p90_ms": round(float(np.percentile(ts, 90)), 4)}


def selection(a):
    r = Renderer(0)
    r.upload(atrium250k(a.width, a.height)).build_accel("bvh2")
    n = a.round
    rule = dict(samples=n, threshold=0.0, min_samples=n, max_samples=n)
    t0 = time.perf_counter()
    r.trace_adaptive(**rule)
    r.sync()
    first_round_ms = (time.perf_counter() - t0) * 1e3
    assert (r.read_adaptive()[0] == n).all()

    def none_active(trace):
        assert trace(**rule) == 0
    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "reps": a.reps, "round_samples": n}
    if a.kernel_only:
        for _ in range(a.reps):
            none_active(r.trace_adaptive_filtered)
        r.close()
        return res
    res["raw_ms"] = timed(lambda: none_active(r.trace_adaptive), a.reps)
    res["filtered_ms"] = timed(lambda: none_active(r.trace_adaptive_filtered), a.reps)
    res["filtered_k0_ms"] = timed(lambda: assert_zero(r.trace_adaptive_filtered(iterations=0, **rule)), a.reps)
    res["denoise_adaptive_compute_ms"] = timed(lambda: r._chk(r._lib.crt_denoise_adaptive(r._h, None, None, None, None)), a.reps)
    # one round of every tile, warm: the wall time the selection is a share of
    ts = []
    for _ in range(3):
        r.reset()
        r.trace_adaptive(**rule)
        r.sync()
        r.reset()
        t = time.perf_counter()
        r.trace_adaptive(**rule)
        r.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    res["first_round_ms"] = round(first_round_ms, 3)
    res["round_ms"] = round(statistics.median(ts), 3)
    res["filtered_share_of_round"] = round(res["filtered_ms"]["median_ms"] / res["round_ms"], 5)
    r.close()
    return res


def assert_zero(n):
    assert n == 0


def payoff(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import denoise_ref as ref
    w, h = 480, 270
    r = Renderer(0)
    r.upload(atrium250k(w, h)).build_accel("bvh2")
    r.frame(a.converged_spp).sync()
    conv = ref.linear_rgb(r.read_accum(), a.converged_spp)
    r.reset()

    def run(trace, tau):
        rounds, t0 = 0, time.perf_counter()
        while trace(samples=16, threshold=tau, min_samples=16, max_samples=256):
            rounds += 1
        r.sync()
        dt = time.perf_counter() - t0
        counts = r.read_adaptive()[0]
        npx = np.repeat(np.repeat(counts, 8, 0), 8, 1)[:h, :w]
        rgb = r.denoise_adaptive(rgb=True)[1][..., :3]
        noisy = (r.read_accum().astype(np.float64)[..., :3] / npx[..., None]) @ ref.M.T
        r.reset()
        return {"threshold": tau, "rounds": rounds, "mean_spp": round(float(npx.mean()), 3), "seconds": round(dt, 4),
                "mse_filtered": ref.mse_display(rgb, conv), "mse_unfiltered": ref.mse_display(noisy, conv)}
    res = {"scene": "S2 atrium250k", "width": w, "height": h, "converged_spp": a.converged_spp, "step": 16, "cap": 256,
           "raw": [run(r.trace_adaptive, t) for t in a.raw_thresholds],
           "filtered": [run(r.trace_adaptive_filtered, t) for t in a.filtered_thresholds]}
    target = [x for x in res["raw"] if x["threshold"] == 0.05]
    if target:
        goal = target[0]["mse_filtered"]

        def fewest(runs):
            ok = [x["mean_spp"] for x in runs if x["mse_filtered"] <= goal]
            return min(ok) if ok else None
        res["samples_for_raw_0.05_mse"] = {"mse": goal, "raw": fewest(res["raw"]), "filtered": fewest(res["filtered"])}
    r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--round", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--skip-selection", action="store_true")
    ap.add_argument("--skip-payoff", action="store_true")
    ap.add_argument("--converged-spp", type=int, default=2048)
    ap.add_argument("--raw-thresholds", type=float, nargs="+", default=[0.2, 0.1, 0.05, 0.025])
    ap.add_argument("--filtered-thresholds", type=float, nargs="+", default=[0.04, 0.02, 0.01, 0.005, 0.004, 0.0035, 0.003, 0.0025])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.skip_selection:
        res["selection"] = selection(a)
    if not a.skip_payoff and not a.kernel_only:
        res["payoff"] = payoff(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
