#!/usr/bin/env python3
"""Generate tests/golden/denoise_pins.json: SHA-256 of the raw bytes of every output of the three preview filters on a
few small renders (run on an MI355X; tests/test_denoise_pins_gpu.py recomputes them with pins()).

The renders are the oracle's bit for bit, so the hashes depend on the filters alone.  The plain filter is also pinned
against the C oracle (tests/test_denoise_parity_gpu.py); the adaptive and temporal filters are held to 1e-4 elsewhere, and
here to the bit, so that a change which is meant to leave them alone can show that it does.  A change that is meant to
move them regenerates the file and says so.

  adaptive/full/k{0,1,5}   Cornell 100x76 (no multiple of 8 or 16), two trace_adaptive rounds that leave tiles at 4 and
                           at 8 samples; at k = 5 the step is 16 and taps leave the frame on every side
  adaptive/tile/k{0,1,5}   the same in the tile (16, 8)..(53, 29), 37x21
  temporal/{defaults,other}/f{0,1,2}/k{0,5}
                           Cornell 100x76, three orbit cameras, 4 samples each at sample offset 4 f; `other` has the
                           parameters of test_blend_matches_the_reference_other_parameters
  plain/k5                 crt_denoise on frame 0 of that orbit
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoise_pins.json")
W, H = 100, 76
TILE = (16, 8, 53, 29)
SPP = 4
OTHER = dict(sigma_color=0.5, sigma_normal=0.25, sigma_plane=0.1, max_history=6.0, normal_tol=0.1, plane_tol=0.5)


def _put(out, name, arrays, planes):
    for plane, a in zip(planes, arrays):
        out[f"{name}/{plane}"] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _temporal(r, ps, out):
    from computeraytracer_amd.scene import orbit_cameras
    cams = orbit_cameras(ps.camera, 64)[:3]
    for label, params in (("defaults", {}), ("other", OTHER)):
        r.temporal_reset()
        for f, cam in enumerate(cams):
            r.set_camera(cam).set_sample_offset(f * SPP).frame(SPP).sync()
            for k in (0, 5):
                _put(out, f"temporal/{label}/f{f}/k{k}", r.denoise_temporal(k, rgb=True, history=True, **params),
                     ("rgba8", "rgb", "history"))
            if f == 0 and not params:
                _put(out, "plain/k5", r.denoise(5, rgb=True), ("rgba8", "rgb"))


def _adaptive(r, out, name, shape):
    """Every tile to 4 samples, then the tiles above the median error to 8."""
    r.trace_adaptive(samples=SPP, threshold=0.0, min_samples=SPP, max_samples=2 * SPP)
    _, errors = r.read_adaptive()
    thr = float(np.median(errors[np.isfinite(errors)]))
    r.trace_adaptive(samples=SPP, threshold=thr, min_samples=SPP, max_samples=2 * SPP)
    counts, _ = r.read_adaptive()
    assert sorted(np.unique(counts).tolist()) == [SPP, 2 * SPP], np.unique(counts)
    for k in (0, 1, 5):
        res = r.denoise_adaptive(k, rgb=True, var=True)
        assert res[0].shape == shape + (4,) and res[2].shape == shape
        _put(out, f"adaptive/{name}/k{k}", res, ("rgba8", "rgb", "var"))


def pins(r):
    """{case/plane: sha256} from the context r, which is left at sample 0 on the full Cornell frame without history."""
    from computeraytracer_amd import cornell
    ps = cornell(W, H)
    out = {}
    try:
        r.upload(ps).build_accel("bvh2")
        _temporal(r, ps, out)
        r.temporal_reset().reset().set_sample_offset(0)
        _adaptive(r, out, "full", (H, W))
        r.reset().set_tile(*TILE)
        _adaptive(r, out, "tile", (TILE[3] - TILE[1], TILE[2] - TILE[0]))
    finally:
        r.set_tile(0, 0, W, H)
        r.temporal_reset().reset().set_sample_offset(0)
    return out


def dump(out):
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from computeraytracer_amd import Renderer
    with Renderer(0) as r:
        out = pins(r)
    with open(a.out, "w") as f:
        f.write(dump(out))
    print(f"wrote {len(out)} hashes to {a.out}")


if __name__ == "__main__":
    main()
