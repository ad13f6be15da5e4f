"""GPU tests of option "adaptive_temporal" (include/crt.h "Sample offset" and "Temporal reuse across camera moves",
DESIGN.md 6i; run with -m gpu on an MI355X): under a sample offset B every pixel of an adaptive render holds the oracle's
samples B+1 .. B+n_t of its tile's count, bit for bit; where every tile holds the same count the temporal calls return the
uniform calls' bits; where the counts differ they are the float64 restatement of tests/denoise_temporal_adaptive_ref.py
fed the GPU's own accumulators, counts, G-buffers, camera frames and previous slot, within the bounds of
tests/test_denoise_svgf_gpu.py; uniform and adaptive frames share one history; and the calls change nothing a render
depends on."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_adaptive_ref as aref
import denoise_motion_ref as mref
import denoise_ref as ref
import denoise_temporal_adaptive_ref as taref
from conftest import ROOT, bits
from test_denoise_motion_gpu import send
from test_denoise_svgf_gpu import S_FLOOR, VAR_TOL, no_history, same, svgf_all
from test_denoise_temporal_gpu import TOL, cam_frame

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")
F = np.float32
B = 37
W, H = 72, 61                                                # partial 8x8 tiles on both edges


def tidy(r):
    r.set_option("temporal_motion", 0)
    r.set_option("adaptive_temporal", 0)
    r.temporal_reset().reset().set_sample_offset(0)


def refused(fn, code, match=None):
    from computeraytracer_amd._lib import CrtError
    with pytest.raises(CrtError, match=match) as e:
        fn()
    assert e.value.code == code


def rounds(r, step, min_samples, max_samples, threshold=None):
    """Adaptive rounds until no tile is active; threshold None: the median tile error after the first round.  Returns the
    tile counts."""
    thr, k = (0.0 if threshold is None else threshold), 0
    while r.trace_adaptive(samples=step, threshold=float(thr), min_samples=min_samples, max_samples=max_samples):
        k += 1
        assert k <= 64
        if k == 1 and threshold is None:
            e = r.read_adaptive()[1]
            thr = F(np.median(e[np.isfinite(e)]))
    return r.read_adaptive()[0]


# ------------------------------------------------------------------ 1. offsets
@pytest.fixture(scope="module")
def offset_truth(orc):
    """The oracle's frames of samples B+1 .. B+n of the 72 x 61 Cornell box, each rendered once."""
    from computeraytracer_amd import cornell
    ps = cornell(W, H)
    sc = orc.Scene.from_packed(ps)
    frames = {}

    def frame(n):
        if n not in frames:
            frames[n] = sc.render(n, first_sample=B + 1)[0]
        return frames[n]
    return ps, sc, frame


def assert_pixels_are_the_oracles(r, sc, frame, counts):
    """Every pixel: the accumulator of samples B+1 .. B+n_t, and the rgba8 tone-mapped with n_t."""
    acc, rgba = r.read_accum(), r.read_rgba8()
    g = np.zeros(acc.shape[:2] + (8,), F)                       # (no pass runs at iterations = 0: the guides are not read)
    npx = taref.pixel_counts(counts, *acc.shape[:2])
    for n in np.unique(npx):
        m = npx == n
        want = frame(int(n))
        assert np.array_equal(bits(acc)[m][:, :3], bits(want)[m][:, :3]), f"accumulator at count {n} differs from the oracle"
        assert np.array_equal(rgba[m], sc.denoise(want, int(n), g, iterations=0)[1][m]), f"rgba8 at count {n}"


@pytest.mark.parametrize("accel", ["bvh2", "lbvh", "ploc"])
def test_uniform_counts_under_an_offset_are_the_oracles_samples(renderer, offset_truth, accel):
    ps, sc, frame = offset_truth
    r = renderer
    try:
        r.upload(ps).build_accel(accel).set_option("adaptive_temporal", 1)
        r.set_sample_offset(B)
        for _ in range(2):
            assert r.trace_adaptive(samples=3, threshold=0.0, min_samples=3, max_samples=6) == 9 * 8
        assert r.trace_adaptive(samples=3, threshold=0.0, min_samples=3, max_samples=6) == 0
        counts = r.read_adaptive()[0]
        assert (counts == 6).all() and r.sample_offset == B
        acc, rgba = r.read_accum(), r.read_rgba8()
        assert_pixels_are_the_oracles(r, sc, frame, counts)
        r.reset()
        assert r.sample_offset == B
        r.frame(6).sync()                                       # ... and the uniform call under the same offset
        assert np.array_equal(bits(acc)[..., :3], bits(r.read_accum())[..., :3]) and np.array_equal(rgba, r.read_rgba8())
    finally:
        tidy(r)


@pytest.mark.parametrize("accel", ["bvh2", "lbvh", "ploc"])
def test_varying_counts_under_an_offset_are_the_oracles_samples(renderer, offset_truth, accel):
    ps, sc, frame = offset_truth
    r = renderer
    try:
        r.upload(ps).build_accel(accel).set_option("adaptive_temporal", 1)
        r.set_sample_offset(B)
        assert r.trace_adaptive(samples=2, threshold=0.0, min_samples=2, max_samples=6) == 9 * 8
        e = r.read_adaptive()[1]
        thr = float(F(np.median(e[np.isfinite(e)])))
        for _ in range(2):
            r.trace_adaptive(samples=2, threshold=thr, min_samples=2, max_samples=6)
            assert_pixels_are_the_oracles(r, sc, frame, r.read_adaptive()[0])
        counts = r.read_adaptive()[0]
        print(f"{accel}: counts {dict(zip(*np.unique(counts, return_counts=True)))}")
        assert len(np.unique(counts)) >= 2 and counts.min() == 2 and counts.max() == 6
    finally:
        tidy(r)


def test_offset_rules_of_the_adaptive_state():
    """The refusals, the context unchanged after each; on a context of its own."""
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(W, H)
    every = dict(threshold=1e30, min_samples=1000, max_samples=0)   # every tile is active in every call
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2")
        for bad in (2, -1, 1 << 32):
            refused(lambda: r.set_option("adaptive_temporal", bad), -1, "adaptive_temporal")
        r.set_sample_offset(B)
        refused(lambda: r.trace_adaptive(samples=2), -3, "sample offset")       # the option is 0: as without it
        assert r.sample == 0 and r.sample_offset == B and not r.read_accum().any()
        r.set_option("adaptive_temporal", 1)
        r.set_option("pipeline", 0)
        refused(lambda: r.trace_adaptive(samples=2), -3, "wavefront")
        assert r.sample == 0 and not r.read_accum().any()
        r.set_option("pipeline", 1).build_accel("none")
        refused(lambda: r.trace_adaptive(samples=2), -3, "wavefront")
        assert r.sample == 0 and not r.read_accum().any()
        r.set_sample_offset(0)
        assert r.trace_adaptive(samples=2, **every) == 72           # offset 0 goes with every form, as before
        r.build_accel("bvh2").reset()
        # B + the samples requested in this adaptive state may not pass 2^32 - 1
        top = 0xFFFFFFFF - 3
        r.set_sample_offset(top)
        refused(lambda: r.trace_adaptive(samples=4, **every), -1, "2\\^32")
        assert r.sample == 0 and r.sample_offset == top and not r.read_accum().any()   # (still the uniform state)
        assert r.trace_adaptive(samples=2, **every) == 72
        acc, counts = r.read_accum(), r.read_adaptive()[0]
        refused(lambda: r.trace_adaptive(samples=2, **every), -1, "2\\^32")  # 2 so far + 2 more
        assert np.array_equal(r.read_adaptive()[0], counts) and np.array_equal(bits(r.read_accum()), bits(acc))
        assert r.trace_adaptive(samples=1, **every) == 72           # index 2^32 - 1 itself is drawn
        assert (r.read_adaptive()[0] == 3).all()
        r.reset()                                                   # a new adaptive state counts from 0 again
        assert r.trace_adaptive(samples=3, **every) == 72
        # the option back at 0 in the adaptive state: the calls refuse again and nothing is dropped
        r.reset().set_sample_offset(B)
        assert r.trace_adaptive(samples=2, **every) == 72
        hw = r.denoise_temporal(0, history=True)[1]
        r.set_option("adaptive_temporal", 0)
        for call in (r.denoise_temporal, r.denoise_svgf, r.read_motion, r.read_moments):
            refused(call, -3, "adaptive state")
        refused(lambda: r.trace_adaptive(samples=2, **every), -3, "sample offset")
        r.set_option("adaptive_temporal", 1)
        assert np.array_equal(bits(r.denoise_temporal(0, history=True)[1]), bits(hw))
        assert r.read_motion().shape == (H, W, 2)
        r.set_row_bands(8, 2, 1)                                    # row bands keep refusing
        assert r.trace_adaptive(samples=2, **every) > 0
        refused(r.denoise_temporal, -3, "row-band")
        refused(r.denoise_svgf, -3, "row-band")


# ------------------------------------------------------------------ 2. uniform counts are the uniform call, bit for bit
def _everything(r):
    """Both filters at K = 0 and K = 5 with every output, in one fixed order (each call overwrites CURRENT)."""
    out = []
    for k in (0, 5):
        out += list(r.denoise_temporal(k, rgb=True, history=True))
    out.append(r.read_motion())
    for k in (0, 5):
        out += list(svgf_all(r, k, min_frames=2.0))
    out.append(r.read_motion())
    return out


def _same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("moving", [False, True])
def test_uniform_counts_are_the_uniform_call_bit_for_bit(renderer, moving):
    """One context renders frame(4); a second one, with the option, trace_adaptive(samples 4, min 4, max 4)."""
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = [ps.camera] * 3 if moving else orbit_cameras(ps.camera, 64)[:4]
    u = renderer
    with Renderer(0) as a:
        try:
            for r in (u, a):
                r.upload(ps).build_accel("bvh2").set_option("temporal_motion", 1 if moving else 0)
            a.set_option("adaptive_temporal", 1)
            prims = ps.primitives
            for k, cam in enumerate(cams):
                if moving and k:
                    new = mref.animate(ps.primitives, k)
                    for r in (u, a):
                        send(r, new, prims)
                    prims = new
                for r in (u, a):
                    r.set_camera(cam).set_sample_offset(4 * k)
                u.frame(4).sync()
                assert a.trace_adaptive(samples=4, threshold=0.0, min_samples=4, max_samples=4) == 13 * 10
                assert np.array_equal(bits(u.read_accum())[..., :3], bits(a.read_accum())[..., :3])
                got, want = _everything(a), _everything(u)
                assert _same_bits(got, want), f"frame {k}: " + str([i for i, (x, y) in enumerate(zip(got, want)) if not _same_bits([x], [y])])
            hw, mom = want[2], want[-2]
            # (4 per frame up to rounding: from the fourth frame on sum(w Hw') / sum(w) is inexact)
            assert abs(hw.max() - 4 * len(cams)) <= TOL * 4 * len(cams) and (hw > 4).mean() > 0.5 and (mom[..., 2] > 4).mean() > 0.5
            assert np.isnan(want[-1]).any() and not np.isnan(want[-1]).all()           # (glass has no position, the walls have)
        finally:
            tidy(u)


# ------------------------------------------------------------------ 3. varying counts against the restatement
def gbuffer_of(r):
    """The G-buffer of the current camera (crt_read_gbuffer wants a uniform sample; it depends on the camera alone)."""
    r.frame(1).sync()
    g = r.read_gbuffer()
    r.reset()
    return g


def check_frame(r, orc, prims, cam, g, prev, size, **params):
    """tests/test_denoise_svgf_gpu.check_frame with a count per pixel: crt_denoise_temporal's and crt_denoise_svgf's blend,
    the moments and the variance against taref.blend / taref.variance fed `prev` (the GPU's own previous slot) and the
    GPU's own counts; K = 5 against aref.atrous_var on the GPU's own (c, v).  The bounds are that file's.  Returns (the
    slot this frame leaves, the counts per pixel, Hw, moments, variance at K = 0)."""
    Wd, Hh = size
    p = dict(taref.DEFAULTS, **params)
    acc = r.read_accum()
    npx = taref.pixel_counts(r.read_adaptive()[0], Hh, Wd)
    n = npx.astype(np.float64)
    key, frame = ref.keys(g, prims), cam_frame(orc, cam)
    t_rgba0, t_rgb0, t_hw0 = r.denoise_temporal(0, rgb=True, history=True, **{k: p[k] for k in taref.BLEND})
    rgba0, rgb0, hw0, v0, mom = svgf_all(r, 0, **params)
    assert same((t_rgba0, t_rgb0[..., :3].copy(), t_hw0), (rgba0, rgb0[..., :3].copy(), hw0))          # one blend
    want, want_hw, want_m, doubt = taref.blend(acc, npx, g, key, frame, prev, Wd, Hh, **{k: p[k] for k in taref.BLEND})
    keep = ~doubt
    err = (np.abs(rgb0[..., :3] - want) / np.maximum(1.0, np.abs(want)))[keep]
    herr = (np.abs(hw0 - want_hw) / want_hw)[keep]
    d0 = np.abs(rgba0.astype(np.int32) - ref.to_rgba8(want).astype(np.int32))[keep]
    m1, s, mw = (mom[..., k].astype(np.float64) for k in range(3))
    w1, ws, wmw = (want_m[..., k] for k in range(3))
    with np.errstate(all="ignore"):
        e1 = (np.abs(m1 - w1) / np.abs(w1))[keep & (w1 != 0)]
        es = (np.abs(s - ws) / np.maximum(ws, S_FLOOR * np.maximum(1.0, w1) ** 2))[keep]
    emw = (np.abs(mw - wmw) / wmw)[keep]
    print(f"{Wd}x{Hh} counts {dict(zip(*np.unique(npx, return_counts=True)))}: left out {doubt.mean():.5f}; K=0 colour max rel err "
          f"{err.max():.3g}, Hw {herr.max():.3g}, rgba8 max {d0.max()}; m1 {e1.max():.3g}, s {es.max():.3g}, Mw {emw.max():.3g}; "
          f"reused {float((want_hw > n).mean()):.4f}, with moments {float((wmw > n).mean()):.4f}")
    assert doubt.mean() <= 0.02
    assert err.max() <= TOL and herr.max() <= TOL and d0.max() <= 1
    assert e1.max() <= TOL and emw.max() <= TOL and es.max() <= TOL
    assert np.array_equal(m1[keep & (w1 == 0)], w1[keep & (w1 == 0)]) and (mom[..., 3] == 0).all()
    want_v, known = taref.variance(mom, npx, p["min_frames"])
    ev = np.abs(v0 - want_v) / np.maximum(want_v, aref.EPS)
    frames = mom[..., 2] / npx.astype(F)
    print(f"    v: known {known.mean():.4f}, max err {ev.max():.3g} of max(v, EPS)")
    assert ev.max() <= TOL
    assert (v0[frames < F(p["min_frames"])] == 1.0).all() and (v0[no_history(g, prims)] == 1.0).all()
    if prev is None:
        assert (v0 == 1.0).all() and (mw == n).all() and (s == 0).all() and (hw0 == n).all()
        assert np.array_equal(bits(mom[..., 0]), bits(acc[..., 1] / npx.astype(F)))
    assert np.array_equal(bits(rgb0[..., 3]), bits(v0))
    rgba5, rgb5, hw5, v5, mom5 = svgf_all(r, 5, **params)
    want5, want_v5 = aref.atrous_var(rgb0[..., :3], v0, g[..., 1:4], g[..., 4:7], key, **{k: p[k] for k in taref.FILTER})
    err5 = np.abs(rgb5[..., :3] - want5) / np.maximum(1.0, np.abs(want5))
    d5 = np.abs(rgba5.astype(np.int32) - ref.to_rgba8(want5).astype(np.int32))
    ev5 = np.abs(v5 - want_v5) / np.maximum(want_v5, aref.EPS)
    print(f"    K=5 colour max rel err {err5.max():.3g}, rgba8 max {d5.max()}, variance {ev5.max():.3g}")
    assert err5.max() <= TOL and d5.max() <= 1 and ev5.max() <= VAR_TOL
    assert np.array_equal(bits(hw5), bits(hw0)) and np.array_equal(bits(mom5), bits(mom))    # CURRENT stays unfiltered
    return taref.slot(rgb0, hw0, mom, g, key, frame, prims), npx, hw0, mom, v0


@pytest.mark.parametrize("params", [dict(min_frames=2.0), dict()], ids=["min_frames2", "defaults"])
def test_varying_counts_match_the_restatement(renderer, orc, params):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("adaptive_temporal", 1)
        prev = None
        for k, cam in enumerate(orbit_cameras(ps.camera, 64)[:4]):
            r.set_camera(cam)
            g = gbuffer_of(r)
            r.set_sample_offset(8 * k)
            rounds(r, 2, 2, 8)
            prev, npx, hw, mom, v = check_frame(r, orc, ps.primitives, cam, g, prev, (100, 76), **params)
            assert len(np.unique(npx)) >= 3, "the threshold should leave at least three distinct counts"
        assert (hw > npx).mean() > 0.5 and (mom[..., 2] > npx).mean() > 0.5
        # (with F = Mw / n_p a pixel is trusted once its history weighs min_frames - 1 times its own count: after four frames
        # most of the pixels that reuse history at min_frames 2, and at the default 4 those whose own count is low)
        assert (v != 1.0).mean() > 0.3 if params else (v != 1.0).any()
    finally:
        tidy(r)


# ------------------------------------------------------------------ 4. mixing and state
def test_uniform_and_adaptive_frames_share_one_history(renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = orbit_cameras(ps.camera, 64)
    r = renderer

    def uniform(k):
        r.set_camera(cams[k]).set_sample_offset(8 * k).frame(4).sync()
        return np.full((76, 100), 4.0)

    def adaptive(k):
        r.set_camera(cams[k]).set_sample_offset(8 * k)
        return taref.pixel_counts(rounds(r, 2, 2, 8), 76, 100).astype(np.float64)
    try:
        r.upload(ps).build_accel("bvh2").set_option("adaptive_temporal", 1)
        for first, second in ((uniform, adaptive), (adaptive, uniform)):
            r.temporal_reset()
            n0 = first(0)
            hw0 = svgf_all(r, 0)[2]
            assert np.array_equal(hw0, n0)
            n1 = second(1)
            _, _, hw1, _, mom1 = svgf_all(r, 0, min_frames=2.0)
            assert (hw1 > n1).mean() > 0.5 and (mom1[..., 2] > n1).mean() > 0.5, (first.__name__, second.__name__)
            assert n1.max() < hw1.max() <= n0.max() + n1.max()
        # what drops the history drops it in the adaptive state too: the next frame blends with nothing
        events = {"temporal_reset": lambda: r.temporal_reset(),
                  "set_tile": lambda: r.set_tile(0, 0, 100, 76),
                  "update_primitives": lambda: (r.update_primitives(0, ps.primitives[:1]), r.refit_accel()),
                  "update_lights": lambda: r.update_lights(0, ps.lights[:1]),
                  "write_accum": lambda: r.write_accum(np.zeros((76, 100, 4), F), 0)}
        for name, event in events.items():
            adaptive(0)
            r.denoise_svgf()
            event()
            n1 = adaptive(1)
            _, _, hw, v, mom = svgf_all(r, 0, min_frames=2.0)
            assert np.array_equal(hw, n1) and np.array_equal(mom[..., 2], n1) and (mom[..., 1] == 0).all() and (v == 1.0).all(), name
        adaptive(0)                                              # ... and what keeps it keeps it: crt_reset
        r.denoise_svgf()
        r.reset()
        n1 = taref.pixel_counts(rounds(r, 2, 2, 8), 76, 100)
        assert (svgf_all(r, 0)[2] > n1).mean() > 0.5
    finally:
        tidy(r)


def test_the_filters_change_nothing_an_adaptive_render_depends_on(renderer, offset_truth):
    ps, sc, frame = offset_truth
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("adaptive_temporal", 1)
        r.set_sample_offset(B)
        assert r.trace_adaptive(samples=2, threshold=0.0, min_samples=2, max_samples=6) == 72
        counts, errors = r.read_adaptive()
        thr = float(F(np.median(errors[np.isfinite(errors)])))
        before = (r.read_accum(), r.read_rgba8(), counts, errors)
        r.denoise_temporal()
        r.read_motion()
        svgf_all(r, 5)
        r.read_motion()
        after = (r.read_accum(), r.read_rgba8()) + r.read_adaptive()
        assert same(before, after)
        for _ in range(2):
            r.trace_adaptive(samples=2, threshold=thr, min_samples=2, max_samples=6)
            r.denoise_svgf()
        counts = r.read_adaptive()[0]
        assert len(np.unique(counts)) >= 2
        assert_pixels_are_the_oracles(r, sc, frame, counts)
    finally:
        tidy(r)


# ------------------------------------------------------------------ 5. from Node
SCRIPT = r"""
const fs = require('fs');
const { Main, orbitCameras } = require(process.argv[1] + '/host/main.js');
const r = Main({ width: 72, height: 61 });
r.setOption('adaptive_temporal', 1);
const cams = orbitCameras(r.packed.camera, 64);
let out;
for (let k = 0; k < 2; k++) {
  r.setCamera(cams[k]);
  r.setSampleOffset(6 * k);
  while (r.traceAdaptive({ samples: 2, threshold: 0.25, minSamples: 2, maxSamples: 6 }));
  out = r.denoiseSvgf({ iterations: 5, minFrames: 2, history: true, variance: true });
}
const dir = process.argv[2];
fs.writeFileSync(dir + '/counts.bin', Buffer.from(r.readAdaptive().counts.buffer));
fs.writeFileSync(dir + '/accum.bin', Buffer.from(r.readAccum().buffer));
fs.writeFileSync(dir + '/rgba8.bin', Buffer.from(out.rgba8.buffer));
fs.writeFileSync(dir + '/history.bin', Buffer.from(out.history.buffer));
fs.writeFileSync(dir + '/variance.bin', Buffer.from(out.variance.buffer));
fs.writeFileSync(dir + '/moments.bin', Buffer.from(r.readMoments().buffer));
r.destroy();
"""


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_returns_the_python_paths_bytes(tmp_path, renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, check=True, cwd=ROOT, timeout=120)
    ps = cornell(W, H)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("adaptive_temporal", 1)
        for k, cam in enumerate(orbit_cameras(ps.camera, 64)[:2]):
            r.set_camera(cam).set_sample_offset(6 * k)
            counts = rounds(r, 2, 2, 6, threshold=0.25)
            rgba, hw, v, mom = r.denoise_svgf(5, min_frames=2.0, history=True, var=True) + (r.read_moments(),)
        assert len(np.unique(counts)) >= 2 and (hw > taref.pixel_counts(counts, H, W)).mean() > 0.5
        for name, want in (("counts", counts), ("accum", r.read_accum()), ("rgba8", rgba), ("history", hw), ("variance", v),
                           ("moments", mom)):
            assert (tmp_path / (name + ".bin")).read_bytes() == np.ascontiguousarray(want).tobytes(), name
    finally:
        tidy(r)
