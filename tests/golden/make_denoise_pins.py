#!/usr/bin/env python3
"""Generate tests/golden/denoise_pins.json: SHA-256 of the raw bytes of every output of the preview filters on a few
small renders (run on an MI355X; tests/test_denoise_pins_gpu.py recomputes them with pins()).

The renders are the oracle's bit for bit, so the hashes depend on the filters and on the bookkeeping of the two history
slots alone.  The plain filter is also pinned against the C oracle (tests/test_denoise_parity_gpu.py); the adaptive,
temporal and svgf filters and the motion map are held to 1e-4 elsewhere, and here to the bit, so that a change which is
meant to leave them alone can show that it does.  A change that is meant to move them regenerates the file and says so.

  adaptive/full/k{0,1,5}   Cornell 100x76 (no multiple of 8 or 16), two trace_adaptive rounds that leave tiles at 4 and
                           at 8 samples; at k = 5 the step is 16 and taps leave the frame on every side
  adaptive/tile/k{0,1,5}   the same in the tile (16, 8)..(53, 29), 37x21
  temporal/{defaults,other}/f{0,1,2}/k{0,5}
                           Cornell 100x76, three orbit cameras, 4 samples each at sample offset 4 f; `other` has the
                           parameters of test_blend_matches_the_reference_other_parameters
  plain/k5                 crt_denoise on frame 0 of that orbit

The rest is Cornell 64x48 on the same orbit, 4 samples per frame at sample offset 4 f, filters at their defaults:

  svgf/{defaults,other}/f{0,1,2}/k{0,5}
                           crt_denoise_svgf and crt_debug_read_moments; `other` has the parameters of
                           test_moments_variance_and_filter_match_the_reference_other_parameters
  slots/skip/f2            temporal on f0, crt_denoise alone on f1, temporal on f2 and its crt_read_motion
  slots/park/{motion,again,f2}
                           temporal on f0 and f1, then crt_build_accel (the G-buffer goes, history and samples stay),
                           crt_denoise (which rebuilds it), crt_read_motion, temporal again in f1, temporal on f2
  slots/mixed/{f0,f1,f2}   svgf on f0, temporal and then svgf on f1, svgf on f2: the three svgf calls
  slots/reset/f1           temporal on f0, crt_reset and 4 more samples from the same camera, temporal: no event between
                           the two frames invalidates the G-buffer
  motion/{f1,f2,f4}        option temporal_motion on: temporal on f0; patch MOVED shifted by two crt_update_primitives
                           before one crt_refit_accel, temporal on f1; a second shift, svgf on f2; a third shift and
                           crt_denoise alone on f3, temporal on f4 (PREVIOUS is still f2's slot and needs the records
                           as f2 saw them); crt_read_motion with each
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
SW, SH = 64, 48
SVGF_OTHER = dict(sigma_variance=1.5, min_frames=2.0, max_history=6.0)
MOVED = 6                                                      # a white diffuse patch of the short box
SHIFTS = ((2.0, 0.0, 0.0), (4.0, 0.0, 1.0), (7.0, 0.0, 2.0), (9.0, 0.0, 4.0))   # of its origin: the 1st is overwritten before the refit
TEMPORAL = ("rgba8", "rgb", "history")
SVGF = ("rgba8", "rgb", "history", "var", "moments")


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


def _frame(r, cams, f):
    r.set_camera(cams[f]).set_sample_offset(f * SPP).frame(SPP).sync()


def _t(r):
    return r.denoise_temporal(rgb=True, history=True)


def _s(r, iterations=None, **params):
    return r.denoise_svgf(iterations, rgb=True, history=True, var=True, **params) + (r.read_moments(),)


def _svgf(r, cams, out):
    for label, params in (("defaults", {}), ("other", SVGF_OTHER)):
        r.temporal_reset()
        for f in range(3):
            _frame(r, cams, f)
            for k in (0, 5):
                _put(out, f"svgf/{label}/f{f}/k{k}", _s(r, k, **params), SVGF)


def _slots(r, cams, out):
    r.temporal_reset()                                          # skip: PREVIOUS is two frames old, the guides in between are crt_denoise's
    _frame(r, cams, 0)
    _t(r)
    _frame(r, cams, 1)
    r.denoise(5)
    _frame(r, cams, 2)
    _put(out, "slots/skip/f2", _t(r) + (r.read_motion(),), TEMPORAL + ("motion",))

    r.temporal_reset()                                          # park: the G-buffer is rebuilt while CURRENT still needs its own
    _frame(r, cams, 0)
    _t(r)
    _frame(r, cams, 1)
    _t(r)
    r.build_accel("bvh2")
    r.denoise(5)
    _put(out, "slots/park", (r.read_motion(),), ("motion",))
    _put(out, "slots/park/again", _t(r), TEMPORAL)
    _frame(r, cams, 2)
    _put(out, "slots/park/f2", _t(r), TEMPORAL)

    r.temporal_reset()                                          # mixed: a slot without moments between two with
    _frame(r, cams, 0)
    _put(out, "slots/mixed/f0", _s(r), SVGF)
    _frame(r, cams, 1)
    _t(r)
    _put(out, "slots/mixed/f1", _s(r), SVGF)
    _frame(r, cams, 2)
    _put(out, "slots/mixed/f2", _s(r), SVGF)

    r.temporal_reset()                                          # reset: both slots are blended with one G-buffer
    _frame(r, cams, 0)
    _t(r)
    r.reset().set_sample_offset(SPP).frame(SPP).sync()
    _put(out, "slots/reset/f1", _t(r), TEMPORAL)


def _motion(r, ps, cams, out):
    def shifted(i):
        rec = np.array(ps.primitives[MOVED:MOVED + 1], copy=True)
        rec["data1"] += np.asarray(SHIFTS[i], np.float32)
        return rec

    r.temporal_reset().set_option("temporal_motion", 1)
    try:
        _frame(r, cams, 0)
        _t(r)
        r.update_primitives(MOVED, shifted(0)).update_primitives(MOVED, shifted(1)).refit_accel()
        _frame(r, cams, 1)
        _put(out, "motion/f1", _t(r) + (r.read_motion(),), TEMPORAL + ("motion",))
        r.update_primitives(MOVED, shifted(2)).refit_accel()
        _frame(r, cams, 2)
        _put(out, "motion/f2", _s(r) + (r.read_motion(),), SVGF + ("motion",))
        r.update_primitives(MOVED, shifted(3)).refit_accel()
        _frame(r, cams, 3)
        r.denoise(5)
        _frame(r, cams, 4)
        _put(out, "motion/f4", _t(r) + (r.read_motion(),), TEMPORAL + ("motion",))
    finally:
        r.set_option("temporal_motion", 0)
        r.update_primitives(MOVED, ps.primitives[MOVED:MOVED + 1]).refit_accel()


def pins(r):
    """{case/plane: sha256} from the context r, which is left at sample 0 on the full frame of the 64x48 Cornell with its
    records as uploaded, without history and with option temporal_motion off."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps, small = cornell(W, H), cornell(SW, SH)
    cams = orbit_cameras(small.camera, 64)[:5]
    out = {}
    try:
        r.upload(ps).build_accel("bvh2")
        _temporal(r, ps, out)
        r.temporal_reset().reset().set_sample_offset(0)
        _adaptive(r, out, "full", (H, W))
        r.reset().set_tile(*TILE)
        _adaptive(r, out, "tile", (TILE[3] - TILE[1], TILE[2] - TILE[0]))
        r.set_tile(0, 0, W, H)
        r.temporal_reset().reset().set_sample_offset(0)
        r.upload(small).build_accel("bvh2")
        _svgf(r, cams, out)
        _slots(r, cams, out)
        _motion(r, small, cams, out)
    finally:
        r.set_tile(0, 0, *r.image_size)
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
