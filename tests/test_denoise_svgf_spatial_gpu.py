"""GPU tests of option "svgf_spatial_pct" (include/crt.h "Variance-guided temporal filter"; run with -m gpu on
an MI355X): with 0 crt_denoise_svgf is the call it was, bit for bit; with P the pixels whose variance the moments do not
give carry the float64 restatement of tests/denoise_svgf_spatial_ref.py fed the GPU's own moments and G-buffer, every other
pixel and everything the call leaves behind keeps its bits; the passes are denoise_adaptive_ref.atrous_var on the GPU's own
(c, v); rectangles, the early-out, moving geometry and the adaptive state take the same path; and the call changes nothing
a render depends on."""
import numpy as np
import pytest

import denoise_adaptive_ref as aref
import denoise_motion_ref as mref
import denoise_ref as ref
import denoise_svgf_ref as sref
import denoise_svgf_spatial_ref as spref
import denoise_temporal_adaptive_ref as taref
from conftest import bits
from test_adaptive_temporal_gpu import gbuffer_of, rounds
from test_denoise_motion_gpu import send
from test_denoise_svgf_gpu import VAR_TOL, no_history, same, svgf_all
from test_denoise_temporal_gpu import TOL

pytestmark = pytest.mark.gpu
F = np.float32
SPP = 4
OPT = "svgf_spatial_pct"


def tidy(r):
    r.set_option(OPT, 0)
    r.set_option("temporal_motion", 0)
    r.set_option("adaptive_temporal", 0)
    r.temporal_reset().reset().set_sample_offset(0)


def call(r, pct, iterations, **params):
    r.set_option(OPT, pct)
    try:
        return svgf_all(r, iterations, **params)
    finally:
        r.set_option(OPT, 0)


def check_spatial(r, prims, g, n, pct=400, passes=True, **params):
    """The current frame of the context at option value pct against the same frame at 0 and against the restatement.  n: the
    frame's sample count, or the counts per pixel (the adaptive state).  Returns (v at 0, v at pct, known, A, doubt)."""
    p = dict(sref.DEFAULTS, **params)
    key = ref.keys(g, prims)
    a0 = call(r, 0, 0, **params)
    ap = call(r, pct, 0, **params)
    rgba0, rgb0, hw0, v0, mom = a0
    rgbap, rgbp, hwp, vp, momp = ap
    # what the call leaves in CURRENT, and every output but v, does not depend on the option
    assert np.array_equal(rgba0, rgbap) and np.array_equal(bits(rgb0[..., :3]), bits(rgbp[..., :3]))
    assert np.array_equal(bits(hw0), bits(hwp)) and np.array_equal(bits(mom), bits(momp))
    assert np.array_equal(bits(rgbp[..., 3]), bits(vp))
    known = (taref if np.ndim(n) else sref).variance(mom, n, p["min_frames"])[1]
    assert np.array_equal(bits(vp[known]), bits(v0[known])) and (v0[~known] == 1.0).all()
    vs, A, doubt = spref.spatial_variance(mom, known, g, key, pct / 100.0, p["sigma_normal"], p["sigma_plane"])
    want = np.where(known, v0.astype(np.float64), vs)
    keep = ~doubt
    ev = (np.abs(vp - want) / np.maximum(want, aref.EPS))[keep]
    est = ~known & (A >= spref.A_MIN) & keep
    print(f"{g.shape[1]}x{g.shape[0]} P {pct}: known {known.mean():.4f}, estimated {est.mean():.4f}, A < 4 "
          f"{float((~known & (A > 0) & (A < spref.A_MIN)).mean()):.4f}, doubt {doubt.mean():.5f}; max err {ev.max():.3g} of max(v, EPS); "
          f"median estimate {float(np.median(vs[est])) if est.any() else float('nan'):.3g}")
    assert doubt.mean() <= 0.02
    assert ev.max() <= TOL
    assert (vp[no_history(g, prims)] == 1.0).all()
    assert (vp[~known & (A < spref.A_MIN) & keep] == 1.0).all()
    if passes:
        rgba5, rgb5, hw5, v5, mom5 = call(r, pct, 5, **params)
        want5, want_v5 = aref.atrous_var(rgbp[..., :3], vp, g[..., 1:4], g[..., 4:7], key, **{k: p[k] for k in sref.FILTER})
        err5 = np.abs(rgb5[..., :3] - want5) / np.maximum(1.0, np.abs(want5))
        d5 = np.abs(rgba5.astype(np.int32) - ref.to_rgba8(want5).astype(np.int32))
        ev5 = np.abs(v5 - want_v5) / np.maximum(want_v5, aref.EPS)
        print(f"    K=5 colour max rel err {err5.max():.3g}, rgba8 max {d5.max()}, variance {ev5.max():.3g}")
        assert err5.max() <= TOL and d5.max() <= 1 and ev5.max() <= VAR_TOL
        assert np.array_equal(bits(hw5), bits(hw0)) and np.array_equal(bits(mom5), bits(mom))    # CURRENT stays unfiltered
    return v0, vp, known, A, doubt


def orbit_frame(r, cams, k):
    r.set_camera(cams[k]).set_sample_offset(k * SPP).frame(SPP).sync()


@pytest.fixture(scope="module")
def box():
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)                                       # no multiple of 16: partial blocks, halos at all four borders
    return ps, orbit_cameras(ps.camera, 64)


# ------------------------------------------------------------------ 1. the option
def test_the_option_is_read_and_refuses_what_it_cannot_be(renderer, box):
    from computeraytracer_amd._lib import CrtError
    ps, cams = box
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2")
        r.set_option(OPT, 400)                                  # (unknown on the parent: CRT_EINVAL)
        orbit_frame(r, cams, 0)
        want = svgf_all(r, 0)
        assert (want[3] != 1.0).mean() > 0.5                    # frame 1: no pixel is known, most are estimated
        for bad in (1, 24, 10001, -1):
            with pytest.raises(CrtError, match=OPT) as e:
                r.set_option(OPT, bad)
            assert e.value.code == -1
            assert same(want, svgf_all(r, 0))                   # ... and the option stays what it was
        for good in (25, 10000, 0):
            r.set_option(OPT, good)
        assert (svgf_all(r, 0)[3] == 1.0).all()
    finally:
        tidy(r)


def test_zero_is_the_call_as_it_was(renderer, box):
    """Three frames: a context that never set the option, one that set it to 400 and back to 0."""
    from computeraytracer_amd import Renderer
    ps, cams = box
    r = renderer
    try:
        with Renderer(0) as u:
            u.upload(ps).build_accel("bvh2")
            r.upload(ps).build_accel("bvh2")
            r.set_option(OPT, 400)
            r.set_option(OPT, 0)
            for k in range(3):
                orbit_frame(u, cams, k)
                orbit_frame(r, cams, k)
                for it in (0, 5):
                    assert same(svgf_all(u, it, min_frames=2.0), svgf_all(r, it, min_frames=2.0)), (k, it)
    finally:
        tidy(r)


# ------------------------------------------------------------------ 2. the estimate and the passes
def test_the_estimate_matches_the_reference_over_five_frames(renderer, box):
    """At the defaults no pixel is known before the fourth frame.  The option may change between frames (every frame here is
    filtered at 0 and at 400), and twice in a frame is idempotent."""
    ps, cams = box
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2")
        for k in range(5):
            orbit_frame(r, cams, k)
            v0, vp, known, A, doubt = check_spatial(r, ps.primitives, r.read_gbuffer(), r.sample)
            assert known.any() == (k >= 3)
        assert 0.3 < known.mean() < 0.9 and (~known & (vp != 1.0)).mean() > 0.01   # (what the last three frames disoccluded)
        r.set_option(OPT, 400)
        assert same(svgf_all(r), svgf_all(r))
        # the factor multiplies and nothing else
        orbit_frame(r, cams, 5)
        (_, _, _, v100, mom), v10000 = call(r, 100, 0), call(r, 10000, 0)[3]
        both = ~sref.variance(mom, r.sample)[1] & (v100 != 1.0) & (v10000 != 1.0)
        assert both.mean() > 0.01
        assert (np.abs(v10000[both] - F(100.0) * v100[both]) <= 2 * np.spacing(v10000[both])).all()
    finally:
        tidy(r)


# ------------------------------------------------------------------ 3. the geometry of the launch
@pytest.mark.parametrize("rect", [(13, 9, 71, 50), (40, 30, 5, 3)], ids=["71x50", "5x3"])
def test_a_rectangle_stops_the_window_at_its_own_border(renderer, box, rect):
    ps, cams = box
    r = renderer
    x0, y0, w, h = rect
    try:
        r.upload(ps).set_tile(x0, y0, x0 + w, y0 + h).build_accel("bvh2")
        for k in range(2):
            orbit_frame(r, cams, k)
            g = r.read_gbuffer()
            assert g.shape[:2] == (h, w)
            v0, vp, known, A, doubt = check_spatial(r, ps.primitives, g, r.sample, min_frames=2.0)
        assert (vp != 1.0).any()
    finally:
        r.set_tile(0, 0, 100, 76)
        tidy(r)


def test_a_frame_in_which_every_pixel_is_known_is_left_alone(renderer, box):
    """The camera rests, min_frames is 2: on the third frame every pixel is known or excluded, every block returns after its
    vote, and the call is the call at 0 in every output."""
    ps, cams = box
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2")
        for k in range(3):
            orbit_frame(r, [cams[0]] * 3, k)
            a = call(r, 0, 0, min_frames=2.0)
            b = call(r, 400, 0, min_frames=2.0)
            if k == 0:
                assert not same(a, b)
        g, mom = r.read_gbuffer(), a[4]
        known = sref.variance(mom, r.sample, 2.0)[1]
        assert not spref.eligible(mom, known, ref.keys(g, ps.primitives)).any() and known.mean() > 0.5
        assert same(a, b) and same(call(r, 0, 5, min_frames=2.0), call(r, 400, 5, min_frames=2.0))
    finally:
        tidy(r)


# ------------------------------------------------------------------ 4. moving geometry and the adaptive state
def test_the_estimate_under_temporal_motion(renderer, box):
    ps, _ = box
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_motion", 1)
        prims = ps.primitives
        for k in range(3):
            if k:
                new = mref.animate(ps.primitives, k)
                send(r, new, prims)
                prims = new
            r.set_camera(ps.camera).set_sample_offset(SPP * k).frame(SPP).sync()
            if k:
                v0, vp, known, A, doubt = check_spatial(r, prims, r.read_gbuffer(), r.sample, min_frames=2.0)
                assert known.mean() > 0.5 and (~known & (vp != 1.0)).any()
            else:
                r.denoise_svgf()
    finally:
        tidy(r)


def test_the_estimate_in_the_adaptive_state(renderer, box):
    """`known` is F = Mw / n_p with the count of the pixel's own tile; the estimate itself reads Mw alone."""
    ps, cams = box
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("adaptive_temporal", 1)
        for k in range(3):
            r.set_camera(cams[k])
            g = gbuffer_of(r)
            r.set_sample_offset(8 * k)
            npx = taref.pixel_counts(rounds(r, 2, 2, 8), 76, 100)
            if k:
                v0, vp, known, A, doubt = check_spatial(r, ps.primitives, g, npx, min_frames=2.0)
                assert len(np.unique(npx)) >= 2 and known.mean() > 0.3 and (~known & (vp != 1.0)).any()
            else:
                r.denoise_svgf()
    finally:
        tidy(r)


# ------------------------------------------------------------------ 5. read-only
def test_it_changes_nothing_a_render_depends_on(orc):
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(100, 76)
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2").set_option(OPT, 400)
        r.frame(SPP).sync()
        before = (r.read_accum(), r.read_rgba8(), r.sample, r.counters())
        r.denoise_svgf()
        svgf_all(r, 0)
        after = (r.read_accum(), r.read_rgba8(), r.sample, r.counters())
        assert same(before[:2], after[:2]) and before[2] == after[2] == SPP and before[3] == after[3]
        r.frame(SPP).sync()
        acc = r.read_accum()
    want = orc.Scene.from_packed(ps).render(2 * SPP)[0]
    assert np.array_equal(bits(acc)[..., :3], bits(want)[..., :3])
