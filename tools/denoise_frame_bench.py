"""crt_denoise_frame against crt_denoise on S2 (atrium250k) at 1920 x 1080: two ranks of the in-process
transport on ONE GPU, bands of 8 rows, 4 samples per pixel, K = 5, no outputs; beside them one unpartitioned context of the
same build.  Host clock around the synchronous calls, warm; the four measurements alternate within every repetition, and
the medians of --reps repetitions after --warmup are reported:

  denoise              crt_denoise on the unpartitioned context (launches + sync)
  denoise_frame        crt_denoise_frame on rank 0, the frame of the gather assembled already (launches + sync)
  gather_preview       crt_gather(PREVIEW) on both ranks, then crt_sync on both: the copies of the strips
  gather_denoise_frame crt_gather(PREVIEW) on both ranks, then crt_denoise_frame on rank 0: the copies, the assembly of the
                       33 MB accumulator and the filter
  assembly             gather_denoise_frame - gather_preview - denoise_frame, per repetition

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
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ps = atrium250k(a.width, a.height)
    one = Renderer(0)
    one.upload(ps).build_accel("bvh2").frame(a.spp).sync()
    cid = Renderer.comm_unique_id(local=True)
    rs = [Renderer(0) for _ in range(2)]
    for k, r in enumerate(rs):
        r.comm_init(cid, k, 2).upload(ps).comm_partition(a.band).build_accel("bvh2").frame(a.spp)
    for r in rs:
        r.gather(rgba8=False, preview=True)
    lib = one._lib
    p5 = _lib.DenoiseParams(5, 1.0, 0.5, 0.3)

    def denoise():
        one._chk(lib.crt_denoise(one._h, C.byref(p5), None, None))

    def denoise_frame():
        rs[0]._chk(lib.crt_denoise_frame(rs[0]._h, C.byref(p5), None, None))

    def gather():
        for r in rs:
            r.gather(rgba8=False, preview=True)

    def gather_sync():
        gather()
        for r in rs:
            r.sync()

    def gather_denoise_frame():
        gather()
        denoise_frame()

    # the filtered frame is the unpartitioned context's
    same = bool(np.array_equal(one.denoise(5), rs[0].denoise_frame(5)))
    fns = dict(denoise=denoise, denoise_frame=denoise_frame, gather_preview=gather_sync, gather_denoise_frame=gather_denoise_frame)
    ts = {k: [] for k in fns}
    for i in range(a.warmup + a.reps):
        for k, fn in fns.items():
            t = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t) * 1e3
            if i >= a.warmup:
                ts[k].append(dt)
    ts["assembly"] = [g - c - f for g, c, f in zip(ts["gather_denoise_frame"], ts["gather_preview"], ts["denoise_frame"])]

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                "p90_ms": round(float(np.percentile(v, 90)), 4)}

    res = {"scene": "S2 atrium250k", "width": a.width, "height": a.height, "spp": a.spp, "world": 2, "band": a.band, "transport": "local, one GPU",
           "iterations": 5, "reps": a.reps, "warmup": a.warmup, "equal_to_unpartitioned": same}
    res.update({k: stats(v) for k, v in ts.items()})
    res["denoise_frame_minus_denoise_ms"] = round(res["denoise_frame"]["median_ms"] - res["denoise"]["median_ms"], 4)
    for r in rs:
        r.sync()
    for r in rs + [one]:
        r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
