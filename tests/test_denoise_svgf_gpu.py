"""GPU tests of crt_denoise_svgf (include/crt.h "Variance-guided temporal filter"; run with -m gpu on an
MI355X): its blend is crt_denoise_temporal's bit for bit; the moments and the variance are the float64 restatement of
tests/denoise_svgf_ref.py fed the GPU's own accumulators, G-buffers, camera frames and previous slot; the passes after it
are denoise_adaptive_ref.atrous_var on the GPU's own (c, v); the moments live and die with their slot; and the call changes
nothing a render depends on."""
import ctypes as C

import numpy as np
import pytest

import denoise_adaptive_ref as aref
import denoise_motion_ref as mref
import denoise_ref as ref
import denoise_svgf_ref as sref
from conftest import bits
from test_denoise_motion_gpu import send
from test_denoise_temporal_gpu import TOL, cam_frame

pytestmark = pytest.mark.gpu
F = np.float32
SPP = 4
VAR_TOL = 1e-3              # the variance after the passes: 6d's bound (tests/test_denoise_adaptive_gpu.py)
S_FLOOR = 2e-5              # s is compared within TOL of max(s, S_FLOOR max(1, m1)^2): (y - h1)^2 carries an absolute error of
                            # about 4 * 2^-23 |y| |y - h1|, relatively small only above |y - h1| ~ 4e-3 |y|; below that the term is
                            # under the floor and moves v by less than 1e-8 against EPS = (0.5 / 255)^2


def tidy(r):
    r.set_option("temporal_motion", 0)
    r.temporal_reset().reset().set_sample_offset(0)


def same(a, b):
    return all(np.array_equal(bits(x) if x.dtype == F else x, bits(y) if y.dtype == F else y) for x, y in zip(a, b))


def svgf_all(r, iterations=None, **params):
    """(rgba8, rgb, Hw, var, moments) of one call."""
    return r.denoise_svgf(iterations, rgb=True, history=True, var=True, **params) + (r.read_moments(),)


def no_history(g, prims):
    key = ref.keys(g, prims)
    return (key == ref.MISS) | ((key >> np.uint64(24)) == np.uint64(2))


def check_frame(r, orc, prims, cam, prev, size, rect=None, motion=False, **params):
    """One frame of the context against the restatement.  K = 0: blend, moments and variance against sref.blend fed `prev`
    (the GPU's own previous slot) and sref.variance fed the GPU's own moments; K = 5: aref.atrous_var on the GPU's own
    (c, v).  Returns (the slot this frame leaves, Hw, moments, variance at K = 0)."""
    W, Hh = size
    x0, y0 = (rect[0], rect[1]) if rect else (0, 0)
    p = dict(sref.DEFAULTS, **params)
    n = r.sample
    acc, g = r.read_accum(), r.read_gbuffer()
    key, frame = ref.keys(g, prims), cam_frame(orc, cam)
    rgba0, rgb0, hw0, v0, mom = svgf_all(r, 0, **params)
    want, want_hw, want_m, doubt = sref.blend(acc, n, g, key, frame, prev, W, Hh, x0, y0, prims if motion else None,
                                              **{k: p[k] for k in sref.BLEND})
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
    print(f"{g.shape[1]}x{g.shape[0]} n {n}: left out {doubt.mean():.5f}; K=0 colour max rel err {err.max():.3g}, Hw {herr.max():.3g}, "
          f"rgba8 max {d0.max()}; m1 {e1.max():.3g}, s {es.max():.3g}, Mw {emw.max():.3g}; reused {float((want_hw > n).mean()):.4f}, "
          f"with moments {float((wmw > n).mean()):.4f}")
    assert doubt.mean() <= 0.02
    assert err.max() <= TOL and herr.max() <= TOL and d0.max() <= 1
    assert e1.max() <= TOL and emw.max() <= TOL and es.max() <= TOL
    assert np.array_equal(m1[keep & (w1 == 0)], w1[keep & (w1 == 0)]) and (mom[..., 3] == 0).all()
    # the variance, from the GPU's own moments (no pixel is exempt: F is one float32 division on both sides)
    want_v, known = sref.variance(mom, n, p["min_frames"])
    ev = np.abs(v0 - want_v) / np.maximum(want_v, aref.EPS)
    frames = mom[..., 2] / F(n)
    print(f"    v: known {known.mean():.4f}, max err {ev.max():.3g} of max(v, EPS); median known v "
          f"{float(np.median(want_v[known])) if known.any() else float('nan'):.3g}")
    assert ev.max() <= TOL
    assert (v0[frames < F(p["min_frames"])] == 1.0).all() and (v0[no_history(g, prims)] == 1.0).all()
    if prev is None:
        assert (v0 == 1.0).all() and (mw == n).all() and (s == 0).all()
        assert np.array_equal(bits(mom[..., 0]), bits(acc[..., 1] / F(n)))
    assert np.array_equal(bits(rgb0[..., 3]), bits(v0))
    # the passes: 6d's filter on the GPU's own (c, v)
    rgba5, rgb5, hw5, v5, mom5 = svgf_all(r, 5, **params)
    want5, want_v5 = aref.atrous_var(rgb0[..., :3], v0, g[..., 1:4], g[..., 4:7], key, **{k: p[k] for k in sref.FILTER})
    err5 = np.abs(rgb5[..., :3] - want5) / np.maximum(1.0, np.abs(want5))
    d5 = np.abs(rgba5.astype(np.int32) - ref.to_rgba8(want5).astype(np.int32))
    ev5 = np.abs(v5 - want_v5) / np.maximum(want_v5, aref.EPS)
    print(f"    K=5 colour max rel err {err5.max():.3g}, rgba8 max {d5.max()}, variance {ev5.max():.3g}")
    assert err5.max() <= TOL and d5.max() <= 1 and ev5.max() <= VAR_TOL
    assert np.array_equal(bits(rgb5[..., 3]), bits(v5))
    assert np.array_equal(bits(hw5), bits(hw0)) and np.array_equal(bits(mom5), bits(mom))    # CURRENT stays unfiltered
    return sref.slot(rgb0, hw0, mom, g, key, frame, prims), hw0, mom, v0


def run_orbit(r, orc, ps, cams, rect=None, **params):
    size = (int(ps.camera[11]), int(ps.camera[12]))
    prev, out = None, None
    for k, cam in enumerate(cams):
        r.set_camera(cam).set_sample_offset(k * SPP).frame(SPP).sync()
        prev, *out = check_frame(r, orc, ps.primitives, cam, prev, size, rect, **params)
    return out


# ------------------------------------------------------------------ 1. the blend is crt_denoise_temporal's
def test_the_blend_is_crt_denoise_temporal_bit_for_bit(renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = orbit_cameras(ps.camera, 64)[:3]
    r = renderer

    def orbit(call):
        out = []
        for k, cam in enumerate(cams):
            r.set_camera(cam).set_sample_offset(k * SPP).frame(SPP).sync()
            rgba, rgb, hw = call()[:3]
            out.append((rgba, rgb[..., :3].copy(), hw))
        return out
    try:
        r.upload(ps).build_accel("bvh2")
        a = orbit(lambda: r.denoise_temporal(0, rgb=True, history=True))
        tidy(r)
        b = orbit(lambda: r.denoise_svgf(0, rgb=True, history=True))
        for k in range(3):
            assert same(a[k], b[k]), f"frame {k}"
        assert (a[2][2] > SPP).mean() > 0.5 and a[2][2].max() == 3 * SPP
    finally:
        tidy(r)


# ------------------------------------------------------------------ 2 + 3. moments, variance and filter against the restatement
def test_moments_variance_and_filter_match_the_reference(renderer, orc):
    """Five frames at the defaults: with min_frames 4 the variance is known from the fourth frame on."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    try:
        renderer.upload(ps).build_accel("bvh2")
        hw, mom, v = run_orbit(renderer, orc, ps, orbit_cameras(ps.camera, 64)[:5])
        # (20 up to rounding: from the fourth frame on the taps' weights are no powers of two, and sum(w Mw') / sum(w) is inexact)
        assert abs(hw.max() - 5 * SPP) <= TOL * 5 * SPP and abs(mom[..., 2].max() - 5 * SPP) <= TOL * 5 * SPP
        known = v != 1.0
        assert known.mean() > 0.4 and (mom[..., 2][known] >= 4 * SPP).all() and (mom[..., 1][known] > 0).mean() > 0.99
    finally:
        tidy(renderer)


def test_moments_variance_and_filter_match_the_reference_other_parameters(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    try:
        renderer.upload(ps).build_accel("bvh2")
        hw, mom, v = run_orbit(renderer, orc, ps, orbit_cameras(ps.camera, 64)[:3], sigma_variance=1.5, min_frames=2.0, max_history=6.0)
        assert hw.max() == 10.0 and mom[..., 2].max() == 10.0   # 4 + min(8, 6): the cap binds Mw as it binds Hw
        assert (v != 1.0).mean() > 0.5
    finally:
        tidy(renderer)


# ------------------------------------------------------------------ 4. a rectangle
def test_tile_is_filtered_on_its_own(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(128, 96)
    try:
        renderer.upload(ps).set_tile(16, 8, 76, 62).build_accel("bvh2")      # 60 x 54 inside the image
        hw, mom, v = run_orbit(renderer, orc, ps, orbit_cameras(ps.camera, 64)[:4], rect=(16, 8, 60, 54))
        assert hw.shape == (54, 60) and (mom[..., 2] > SPP).mean() > 0.5 and (v != 1.0).mean() > 0.3
    finally:
        renderer.set_tile(0, 0, 128, 96)
        tidy(renderer)


# ------------------------------------------------------------------ 5. moving geometry: k_dn_reproject<true, true>
def test_moments_follow_moving_primitives(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(100, 76)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_motion", 1)
        prev, prims = None, ps.primitives
        for k in range(3):
            if k:
                new = mref.animate(ps.primitives, k)
                send(r, new, prims)
                prims = new
            r.set_camera(ps.camera).set_sample_offset(SPP * k).frame(SPP).sync()
            prev, hw, mom, v = check_frame(r, orc, prims, ps.camera, prev, (100, 76), motion=True, min_frames=2.0)
            if k:
                # the mapped path was taken: on the moved primitives the blend looked somewhere else than at the pixel itself
                uv, g = r.read_motion(), r.read_gbuffer()
                key = ref.keys(g, prims)
                on_moved = mref.moved_mask(g) & (key != ref.MISS) & ((key >> np.uint64(24)) == 0)
                yy, xx = np.mgrid[0:76, 0:100]
                off = np.hypot(uv[..., 0] - xx, uv[..., 1] - yy)
                assert on_moved.sum() > 200 and not np.isnan(uv[on_moved]).any()
                assert (off[on_moved] > 0.25).mean() > 0.95 and np.nanmax(off[~on_moved]) < 0.1
                share = float((mom[..., 2] > SPP)[on_moved].mean())
                print(f"frame {k}: {int(on_moved.sum())} diffuse pixels on moved primitives, {share:.4f} carry moments")
                assert share >= 0.95 and (v != 1.0)[on_moved].mean() > 0.9
        assert mom[..., 2].max() == 3 * SPP
    finally:
        tidy(r)


# ------------------------------------------------------------------ 6. the slots
def _frame(r, cams, k):
    r.set_camera(cams[k]).set_sample_offset(SPP * k).frame(SPP).sync()


def test_a_temporal_slot_has_no_moments_and_twice_is_idempotent(renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd._lib import CrtError
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = orbit_cameras(ps.camera, 64)
    r = renderer

    def refused():
        with pytest.raises(CrtError, match="moments") as e:
            r.read_moments()
        assert e.value.code == -3
    try:
        r.upload(ps).build_accel("bvh2")
        _frame(r, cams, 0)
        refused()                                               # no call in this frame yet
        r.denoise_temporal()
        refused()                                               # ... and a plain crt_denoise_temporal leaves none
        _frame(r, cams, 1)
        refused()
        a = svgf_all(r)
        assert (a[2] > SPP).mean() > 0.5                        # the colour history of the temporal slot is reused ...
        assert (a[4][..., 2] == SPP).all() and (a[4][..., 1] == 0).all() and (a[3] <= 1.0).all()   # ... the moments start again
        assert same(a, svgf_all(r))                             # twice in one frame
        _frame(r, cams, 2)
        b = svgf_all(r)
        assert (b[4][..., 2] == 2 * SPP).mean() > 0.5 and b[4][..., 2].max() == 2 * SPP and b[2].max() == 3 * SPP
        r.denoise_temporal()                                    # the same frame: CURRENT loses its moments, not its colour
        refused()
        assert same(b, svgf_all(r))
        assert r._lib.crt_debug_read_moments(r._h, None) == -1 and r._lib.crt_debug_read_moments(None, None) == -1
    finally:
        tidy(r)


def test_what_drops_the_history_drops_the_moments(renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(64, 48)
    cams = orbit_cameras(ps.camera, 64)
    r = renderer

    def two_frames():
        r.temporal_reset()
        _frame(r, cams, 0)
        r.denoise_svgf()
        _frame(r, cams, 1)
    try:
        r.upload(ps).build_accel("bvh2")
        two_frames()
        _, _, hw, _, mom = svgf_all(r, min_frames=2.0)
        assert (hw > SPP).any() and (mom[..., 2] > SPP).any()   # the set-up does carry both ...
        events = {
            "temporal_reset": lambda: r.temporal_reset().reset().frame(SPP).sync(),
            "upload_scene": lambda: r.upload(ps).build_accel("bvh2").frame(SPP).sync(),
            "set_tile": lambda: r.set_tile(0, 0, 64, 48).frame(SPP).sync(),
            "set_row_bands": lambda: r.set_row_bands(8, 2, 0).set_tile(0, 0, 64, 48).frame(SPP).sync(),
            "update_primitives": lambda: (r.update_primitives(0, ps.primitives[:1]), r.refit_accel(), r.frame(SPP).sync()),
            "update_lights": lambda: r.update_lights(0, ps.lights[:1]).frame(SPP).sync(),
            "write_accum": lambda: r.write_accum(r.read_accum(), SPP),
        }
        for name, event in events.items():                      # ... and after each of these the next call is a frame 0
            two_frames()
            event()
            n = r.sample
            rgba, rgb, hw, v, mom = svgf_all(r, 0, min_frames=2.0)
            acc = r.read_accum()
            assert (hw == n).all() and (mom[..., 2] == n).all() and (mom[..., 1] == 0).all() and (v == 1.0).all(), name
            assert np.array_equal(bits(mom[..., 0]), bits(acc[..., 1] / F(n))), name
            assert np.array_equal(rgba, r.denoise(0)), name
        for name, event in {"reset": lambda: r.reset(), "build_accel": lambda: (r.build_accel("bvh2"), r.reset()),
                            "refit_accel": lambda: r.refit_accel()}.items():        # what keeps the history keeps the moments
            two_frames()
            r.denoise_svgf()
            event()
            r.set_sample_offset(2 * SPP).frame(SPP).sync()
            mom = svgf_all(r)[4]
            assert (mom[..., 2] > 2 * SPP).mean() > 0.4, f"moments lost over {name}"
    finally:
        r.set_tile(0, 0, 64, 48)
        tidy(r)


def test_denoise_svgf_refuses_what_it_cannot_do():
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError, DenoiseSvgfParams
    ps = cornell(64, 48)
    with Renderer(0) as r:
        lib, h = r._lib, r._h
        buf = np.zeros((48, 64, 4), np.uint8)

        def refused(match=None):
            with pytest.raises(CrtError, match=match) as e:
                r.denoise_svgf()
            assert e.value.code == -3
        r.upload(ps)
        refused("accel")                                        # no tree
        r.build_accel("bvh2")
        refused("no sample")                                    # sample 0
        r.frame(SPP).sync()
        r.denoise_svgf()
        assert lib.crt_denoise_svgf(h, None, None, buf.ctypes.data, None, None) == 0         # NULL = the defaults
        assert np.array_equal(buf, r.denoise_svgf())
        assert lib.crt_denoise_svgf(h, None, None, None, None, None) == 0                    # every output may be NULL
        r.set_camera(ps.camera).set_sample_offset(SPP).frame(SPP).sync()
        want = svgf_all(r, min_frames=2.0)
        good = [5, 4.0, 0.5, 0.3, 64.0, 0.5, 2.0, 2.0]
        bad = [[11] + good[1:]]
        for i in range(1, 7):
            for v in (0.0, -1.0, float("nan"), float("inf")):
                bad.append(good[:i] + [v] + good[i + 1:])
        bad += [good[:7] + [v] for v in (1.999, 0.0, -4.0, float("nan"), float("inf"))]
        for p in bad:                                           # CRT_EINVAL: context, history and moments unchanged
            assert lib.crt_denoise_svgf(h, C.byref(DenoiseSvgfParams(*p)), None, buf.ctypes.data, None, None) == -1, p
        assert same(want, svgf_all(r, min_frames=2.0)) and (want[2] > SPP).any() and (want[3] != 1.0).any()
        r.denoise_svgf(iterations=10)                           # the largest allowed
        r.update_primitives(0, ps.primitives[:1])
        r.set_sample_offset(0)
        refused("refit")                                        # a stale tree
        r.refit_accel()
        assert r.trace_adaptive(samples=4, min_samples=4) > 0
        refused("adaptive state")
        r.set_row_bands(8, 2, 1).frame(2).sync()
        refused("row-band")
        r.set_tile(0, 0, 64, 48).frame(2).sync()
        assert r.denoise_svgf().shape == (48, 64, 4)


def _failed_allocation(k, before, call, after):
    """Frame 0 under `before`, then on frame 1 the k-th device allocation of `call` fails: CRT_ENOMEM.  Returns what
    `after` gives on frame 1 and on frame 2 (k = 0: nothing is injected)."""
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(64, 48)
    cams = orbit_cameras(ps.camera, 64)
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2")
        try:
            _frame(r, cams, 0)
            before(r)
            _frame(r, cams, 1)
            if k:
                r.set_option("debug_fail_alloc", k)
                with pytest.raises(CrtError) as e:
                    call(r)
                r.set_option("debug_fail_alloc", 0)
                assert e.value.code == -4                       # CRT_ENOMEM
            out = after(r)
            _frame(r, cams, 2)
            return out + after(r)
        finally:
            r.set_option("debug_fail_alloc", 0)


@pytest.fixture(scope="module")
def uninjected():
    """The runs without a failure, once for every k."""
    return {"svgf": _failed_allocation(0, lambda r: r.denoise_temporal(), None, svgf_all),
            "temporal": _failed_allocation(0, lambda r: r.denoise(), None, lambda r: r.denoise_temporal(rgb=True, history=True))}


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_a_failed_allocation_leaves_the_slots_as_they_were(k, uninjected):
    """A context that has only called crt_denoise_temporal: crt_denoise_svgf makes six allocations (both slots' moment
    planes, the blurred variance, the variance, and the G-buffer and keys of the guide set the new frame is built into).
    The k-th of them fails: CRT_ENOMEM before any slot changes, and the next call finds PREVIOUS and CURRENT where they
    were."""
    a, b = _failed_allocation(k, lambda r: r.denoise_temporal(), lambda r: r.denoise_svgf(), svgf_all), uninjected["svgf"]
    assert same(a, b) and (a[2] > SPP).mean() > 0.5 and (a[9][..., 2] > SPP).mean() > 0.5


@pytest.mark.parametrize("k", [1, 2, 3])
def test_a_failed_allocation_of_the_first_temporal_call_leaves_the_context_as_it_was(k, uninjected):
    """A context that has only called crt_denoise: crt_denoise_temporal makes three allocations (both slots' colour
    planes and the history weights; the guide set is crt_denoise's, rebuilt in place).  The k-th of them fails:
    CRT_ENOMEM, and the next call is the one an uninjected run makes."""
    a = _failed_allocation(k, lambda r: r.denoise(), lambda r: r.denoise_temporal(), lambda r: r.denoise_temporal(rgb=True, history=True))
    b = uninjected["temporal"]
    assert same(a, b) and (a[2] == SPP).all() and (a[5] > SPP).mean() > 0.5


# ------------------------------------------------------------------ 7. read-only
def test_it_changes_nothing_a_render_depends_on(orc):
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(100, 76)
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2").frame(SPP).sync()
        before = (r.read_accum(), r.read_rgba8(), r.sample)
        r.denoise_svgf()
        svgf_all(r, 0)
        after = (r.read_accum(), r.read_rgba8(), r.sample)
        assert same(before[:2], after[:2]) and before[2] == after[2] == SPP
        r.frame(SPP).sync()
        acc = r.read_accum()
    want = orc.Scene.from_packed(ps).render(2 * SPP)[0]
    assert np.array_equal(bits(acc)[..., :3], bits(want)[..., :3])
