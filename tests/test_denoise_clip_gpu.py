"""GPU tests of clipped history (include/crt.h "Clipped history", option "temporal_clip_pct"; run with -m gpu on
an MI355X): the option is read and refuses what it cannot be; at 0 the calls are what they were, bit for bit; the box of
crt_debug_read_clip_box is the float64 restatement of tests/denoise_clip_ref.py fed the GPU's own accumulator, counts and
keys -- in the whole image, in a rectangle and in the adaptive state; the blend is the restatement given the GPU's own box,
with moving primitives too, and changes colours alone; crt_update_lights keeps the history under the option and the clip
follows a switched light sooner; and the call fails, reads and refuses by the rules of the temporal filters."""
import numpy as np
import pytest

import denoise_adaptive_ref as aref
import denoise_clip_ref as cref
import denoise_motion_ref as mref
import denoise_ref as ref
import denoise_temporal_adaptive_ref as taref
from conftest import bits
from test_adaptive_temporal_gpu import gbuffer_of, refused, rounds
from test_denoise_motion_gpu import send
from test_denoise_svgf_gpu import same, svgf_all
from test_denoise_temporal_gpu import PATH_COUNTERS, TOL, cam_frame

pytestmark = pytest.mark.gpu
F = np.float32
SPP = 4
SIZE = (100, 76)
PCT = 100
EINVAL, ESTATE, ENOMEM = -1, -3, -4


def tidy(r):
    r.set_option("temporal_clip_pct", 0)
    r.set_option("temporal_motion", 0)
    r.set_option("adaptive_temporal", 0)
    r.temporal_reset().reset().set_sample_offset(0)


def frame(r, cam, k, spp=SPP):
    r.set_camera(cam).set_sample_offset(k * spp).frame(spp).sync()


def gpu_box(r):
    """crt_debug_read_clip_box as denoise_clip_ref.box returns it: (lo, hi, N, valid), float64."""
    b = r.debug_read_clip_box()
    assert set(np.unique(b[..., 7])) <= {0.0, 1.0}
    return b[..., 0:3].astype(np.float64), b[..., 4:7].astype(np.float64), b[..., 3].astype(np.float64), b[..., 7] == 1.0


def assert_box(got, c_new, key, gamma, what):
    """Test 3: N and valid exactly, lo and hi within TOL of max(1, |want|)."""
    lo, hi, N, valid = cref.box(c_new, key, gamma)
    err = max(float((np.abs(g - w) / np.maximum(1.0, np.abs(w))).max()) for g, w in ((got[0], lo), (got[1], hi)))
    print(f"{what}: {N.shape[1]}x{N.shape[0]}: boxes {float((N > 0).mean()):.4f}, valid {float(valid.mean()):.4f}, N min "
          f"{int(N[N > 0].min())} max {int(N.max())}; lo / hi max rel err {err:.3g}")
    assert np.array_equal(got[2], N) and np.array_equal(got[3], valid)
    assert err <= TOL
    assert valid.mean() > 0.5 and (N[valid] >= 4).all() and N.max() == 49
    return lo, hi, N, valid


def check_frame(r, orc, prims, cam, prev, motion=False, svgf=False, gamma=PCT / 100.0):
    """One frame of the context against the restatement.  K = 0: the box against cref.box fed the GPU's own accumulator and
    keys, the blend against cref.blend fed `prev` (the GPU's own previous slot) and the GPU's own box; K = 5: the passes of
    the call on the GPU's own blend.  Returns the slot this frame leaves and Hw."""
    W, Hh = SIZE
    n = r.sample
    acc, g = r.read_accum(), r.read_gbuffer()
    key, fr = ref.keys(g, prims), cam_frame(orc, cam)
    c_new = ref.linear_rgb(acc, n)
    if svgf:
        rgba0, rgb0, hw0, v0, _ = svgf_all(r, 0)
    else:
        rgba0, rgb0, hw0 = r.denoise_temporal(0, rgb=True, history=True)
    bx = None
    if prev is None:
        refused(r.debug_read_clip_box, ESTATE)                  # the first frame: no PREVIOUS, no box pass
    else:
        bx = gpu_box(r)
        assert_box(bx, c_new, key, gamma, "svgf" if svgf else "temporal")
    want, want_hw, doubt = cref.blend(c_new, n, g, key, fr, prev, W, Hh, box=bx, prims_cur=prims if motion else None,
                                      prims_prev=prev["prims"] if motion and prev is not None else None)
    keep = ~doubt
    err = (np.abs(rgb0[..., :3] - want) / np.maximum(1.0, np.abs(want)))[keep]
    herr = (np.abs(hw0 - want_hw) / want_hw)[keep]
    print(f"    n {n}: left out {doubt.mean():.5f}; K=0 colour max rel err {err.max():.3g}, Hw {herr.max():.3g}; reused "
          f"{float((want_hw > n).mean()):.4f}")
    assert doubt.mean() <= 0.02
    assert err.max() <= TOL and herr.max() <= TOL
    if bx is not None:
        # the clamp did something: the restatement without the box is further from the GPU than TOL somewhere
        plain = cref.blend(c_new, n, g, key, fr, prev, W, Hh, prims_cur=prims if motion else None,
                           prims_prev=prev["prims"] if motion else None)[0]
        assert (np.abs(rgb0[..., :3] - plain) / np.maximum(1.0, np.abs(plain)))[keep].max() > 100 * TOL
    if svgf:
        rgba5, rgb5, hw5, v5, _ = svgf_all(r, 5)
        want5, _ = aref.atrous_var(rgb0[..., :3], v0, g[..., 1:4], g[..., 4:7], key, iterations=5,
                                   **{k: taref.DEFAULTS[k] for k in taref.FILTER if k != "iterations"})
    else:
        rgba5, rgb5, hw5 = r.denoise_temporal(5, rgb=True, history=True)
        want5 = ref.atrous(rgb0[..., :3], g[..., 1:4], g[..., 4:7], key, **dict(ref.DEFAULTS, iterations=5))
    err5 = np.abs(rgb5[..., :3] - want5) / np.maximum(1.0, np.abs(want5))
    d5 = np.abs(rgba5.astype(np.int32) - ref.to_rgba8(want5).astype(np.int32))
    print(f"    K=5 colour max rel err {err5.max():.3g}, rgba8 max {d5.max()}")
    assert err5.max() <= TOL and d5.max() <= 1 and np.array_equal(bits(hw5), bits(hw0))
    return mref.slot(rgb0, hw0, g, key, fr, prims), hw0


# ------------------------------------------------------------------ 1. the option
def test_the_option_is_read_and_refuses_what_it_cannot_be(renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(*SIZE)
    cams = orbit_cameras(ps.camera, 64)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_clip_pct", 150)
        frame(r, cams[0], 0)
        r.denoise_temporal()
        frame(r, cams[1], 1)
        want = r.denoise_temporal(0, rgb=True, history=True) + (r.debug_read_clip_box(),)
        for bad in (24, 10001, -1):
            refused(lambda: r.set_option("temporal_clip_pct", bad), EINVAL, "temporal_clip_pct")
            assert same(r.denoise_temporal(0, rgb=True, history=True) + (r.debug_read_clip_box(),), want)   # the option kept its value
        outs = {}
        for good in (25, 10000, 0, 150):
            r.set_option("temporal_clip_pct", good)
            outs[good] = r.denoise_temporal(0, rgb=True, history=True)
        assert same(outs[150], want[:3])
        assert not same(outs[25], outs[10000]) and not same(outs[25], outs[150]) and not same(outs[0], outs[25])
        assert all(np.array_equal(bits(outs[p][2]), bits(want[2])) for p in outs)            # Hw does not know the option
    finally:
        tidy(r)


# ------------------------------------------------------------------ 2. zero is the call as it was
def test_zero_is_the_call_as_it_was(renderer):
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(*SIZE)
    cams = orbit_cameras(ps.camera, 64)[:3]

    def orbit(r):
        out = []
        for k, cam in enumerate(cams):
            frame(r, cam, k)
            out.append(r.denoise_temporal(rgb=True, history=True) + svgf_all(r) + (r.read_motion(),))
        r.update_lights(0, ps.lights[:1])                       # with 0 this still drops the history
        frame(r, cams[2], 3)
        _, hw = r.denoise_temporal(history=True)
        assert (hw == SPP).all()
        refused(r.debug_read_clip_box, ESTATE)
        return out
    with Renderer(0) as never:
        never.upload(ps).build_accel("bvh2")
        a = orbit(never)
    try:
        renderer.upload(ps).build_accel("bvh2").set_option("temporal_clip_pct", 100).set_option("temporal_clip_pct", 0)
        b = orbit(renderer)
    finally:
        tidy(renderer)
    for k in range(3):
        assert same(a[k], b[k]), f"frame {k}"
    assert (a[2][2] > SPP).mean() > 0.5


# ------------------------------------------------------------------ 3. the box
def test_the_box_matches_the_restatement(renderer, orc):
    """Frame 2 of the orbit: whole image, then a rectangle that is no multiple of 16 and not at the origin."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(*SIZE)
    cams = orbit_cameras(ps.camera, 64)[:3]
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_clip_pct", PCT)
        for rect in (None, (13, 9, 13 + 53, 9 + 39)):
            if rect:
                r.set_tile(*rect)
            for k, cam in enumerate(cams):
                frame(r, cam, k)
                r.denoise_temporal(0)
            acc, g = r.read_accum(), r.read_gbuffer()
            key = ref.keys(g, ps.primitives)
            got = gpu_box(r)
            _, _, N, _ = assert_box(got, ref.linear_rgb(acc, SPP), key, PCT / 100.0, "rectangle" if rect else "whole image")
            assert N.shape == ((39, 53) if rect else (76, 100))
            # the corners see a 4 x 4 window at most: nothing outside the rectangle entered
            assert N[0, 0] <= 16 and N[-1, -1] <= 16 and N[0, -1] <= 16 and N[-1, 0] <= 16
            miss = key == ref.MISS
            glass = ~miss & ((key >> np.uint64(24)) == np.uint64(2))
            assert (N[miss] == 0).all() and (N[glass] == 0).all() and (N[~miss & ~glass] >= 1).all()
            # and a different gamma moves the bounds, not N
            r.set_option("temporal_clip_pct", 250)
            r.denoise_temporal(0)
            wide = gpu_box(r)
            assert_box(wide, ref.linear_rgb(acc, SPP), key, 2.5, "gamma 2.5")
            assert np.array_equal(wide[2], got[2]) and (wide[1] >= got[1]).all() and (wide[0] <= got[0]).all()
            r.set_option("temporal_clip_pct", PCT)
    finally:
        r.set_tile(0, 0, *SIZE)
        tidy(r)


def test_a_rectangle_of_three_pixels_has_no_valid_box(renderer):
    """N < 4 everywhere: the boxes are reported and not used, and the blend is P = 0's bit for bit."""
    from computeraytracer_amd import cornell
    ps = cornell(*SIZE)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_tile(48, 60, 51, 61).set_option("temporal_clip_pct", PCT)      # 3 x 1 on the floor
        for k in range(2):
            frame(r, ps.camera, k)
            clipped = r.denoise_temporal(0, rgb=True, history=True)
        lo, hi, N, valid = gpu_box(r)
        key = ref.keys(r.read_gbuffer(), ps.primitives)
        want = cref.box(ref.linear_rgb(r.read_accum(), SPP), key, PCT / 100.0)
        assert N.shape == (1, 3) and np.array_equal(N, want[2]) and N.max() >= 2 and N.max() <= 3
        assert not valid.any() and not want[3].any() and (hi > lo).any()
        assert np.abs(lo - want[0]).max() <= TOL and np.abs(hi - want[1]).max() <= TOL
        r.set_option("temporal_clip_pct", 0)
        assert same(r.denoise_temporal(0, rgb=True, history=True), clipped) and (clipped[2] > SPP).any()
    finally:
        r.set_tile(0, 0, *SIZE)
        tidy(r)


def test_the_box_in_the_adaptive_state_takes_each_tile_s_count(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(*SIZE)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("adaptive_temporal", 1).set_option("temporal_clip_pct", PCT)
        for k, cam in enumerate(orbit_cameras(ps.camera, 64)[:2]):
            r.set_camera(cam)
            g = gbuffer_of(r)
            r.set_sample_offset(8 * k)
            rounds(r, 2, 2, 8)
            r.denoise_temporal(0)
        npx = taref.pixel_counts(r.read_adaptive()[0], SIZE[1], SIZE[0])
        assert len(np.unique(npx)) >= 3, "the threshold should leave at least three distinct counts"
        c_new = (r.read_accum()[..., :3].astype(np.float64) / npx[..., None].astype(np.float64)) @ ref.M.T
        assert_box(gpu_box(r), c_new, ref.keys(g, ps.primitives), PCT / 100.0, "adaptive")
    finally:
        tidy(r)


# ------------------------------------------------------------------ 4. the blend
def test_the_blend_matches_the_restatement_given_the_gpu_s_box(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(*SIZE)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_clip_pct", PCT)
        prev = None
        for k, cam in enumerate(orbit_cameras(ps.camera, 64)[:3]):
            frame(r, cam, k)
            prev, hw = check_frame(r, orc, ps.primitives, cam, prev)
        assert hw.max() == 3 * SPP and (hw > SPP).mean() > 0.5
    finally:
        tidy(r)


def test_only_colours_differ_from_a_context_without_the_option(renderer):
    """Over the orbit Hw, the moments and crt_read_motion are bit for bit those of P = 0."""
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(*SIZE)
    cams = orbit_cameras(ps.camera, 64)[:4]

    def orbit(r):
        out = []
        for k, cam in enumerate(cams):
            frame(r, cam, k)
            _, rgb_t, hw_t = r.denoise_temporal(0, rgb=True, history=True)
            _, rgb, hw, v, mom = svgf_all(r, 0)
            assert same((rgb_t[..., :3].copy(), hw_t), (rgb[..., :3].copy(), hw))           # one blend, clipped or not
            out.append((rgb[..., :3].copy(), (hw, mom, r.read_motion(), v)))
        return out
    with Renderer(0) as off:
        off.upload(ps).build_accel("bvh2")
        a = orbit(off)
    try:
        renderer.upload(ps).build_accel("bvh2").set_option("temporal_clip_pct", PCT)
        b = orbit(renderer)
    finally:
        tidy(renderer)
    for k in range(4):
        assert same(a[k][1], b[k][1]), f"frame {k}"
        assert np.array_equal(bits(a[k][0]), bits(b[k][0])) == (k == 0), f"frame {k}"


# ------------------------------------------------------------------ 5. moving primitives: k_dn_reproject<true, true, *>
def test_the_clip_follows_moving_primitives(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(*SIZE)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_motion", 1).set_option("temporal_clip_pct", PCT)
        prev, prims = None, ps.primitives
        for k in range(3):
            if k:
                new = mref.animate(ps.primitives, k)
                send(r, new, prims)
                prims = new
            frame(r, ps.camera, k)
            prev, hw = check_frame(r, orc, prims, ps.camera, prev, motion=True, svgf=True)
            if k:
                key = ref.keys(r.read_gbuffer(), prims)
                on_moved = mref.moved_mask(r.read_gbuffer()) & (key != ref.MISS) & ((key >> np.uint64(24)) == 0)
                assert on_moved.sum() > 200 and (hw > SPP)[on_moved].mean() >= 0.95
    finally:
        tidy(r)


# ------------------------------------------------------------------ 6 + 7. lights
def _switch(r, ps, dim, pct, before=4):
    """`before` frames under the light with the option at pct, crt_update_lights to the dim rows, and the next frame traced."""
    r.upload(ps).build_accel("bvh2").set_option("temporal_clip_pct", pct)
    for k in range(before):
        frame(r, ps.camera, k)
        r.denoise_temporal()
    r.update_lights(0, dim)
    frame(r, ps.camera, before)


def test_a_light_edit_keeps_the_history_and_the_clip_follows_it(renderer):
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd.scene import PackedScene
    ps, dim = cref.with_dim_row(cornell(*SIZE))
    with Renderer(0) as t:
        t.upload(PackedScene(ps.primitives, dim, ps.camera, ps.spectra, ps.cie, ps.patches, ps.spectrum_index)).build_accel("bvh2")
        t.set_sample_offset(100000).frame(256).sync()
        truth = ref.linear_rgb(t.read_accum(), 256)
    r = renderer
    try:
        err = {}
        for pct in (0, 100, 10000):
            _switch(r, ps, dim, pct)
            acc, g = r.read_accum(), r.read_gbuffer()
            key = ref.keys(g, ps.primitives)
            diffuse = (key != ref.MISS) & ((key >> np.uint64(24)) == 0)
            _, rgb0, hw = r.denoise_temporal(0, rgb=True, history=True)
            if pct == 0:
                assert (hw == SPP).all()                        # today's behaviour: the history is gone
                refused(r.debug_read_clip_box, ESTATE)
            else:
                assert (hw[diffuse] > SPP).all() and abs(hw.max() - 5 * SPP) <= TOL * 5 * SPP    # (20 up to the rounding of sum(w Hw') / sum(w))
                lo, hi, _, valid = gpu_box(r)
                c_new = ref.linear_rgb(acc, SPP)
                used = valid & (hw > SPP)
                low, high = np.minimum(c_new, lo), np.maximum(c_new, hi)
                c = rgb0[..., :3].astype(np.float64)
                assert used.mean() > 0.5
                assert (c >= low - TOL * np.maximum(1.0, np.abs(low)))[used].all()
                assert (c <= high + TOL * np.maximum(1.0, np.abs(high)))[used].all()
            _, rgb5 = r.denoise_temporal(rgb=True)
            err[pct] = ref.mse_display(rgb5[..., :3], truth)
            tidy(r)
        print(f"first frame after the switch, MSE in display space against 256 spp of the dim scene: history dropped {err[0]:.5f}, "
              f"kept and clipped at P = 100 {err[100]:.5f}, at P = 10000 {err[10000]:.5f}; ratio {err[100] / err[10000]:.3f}")
        assert err[100] < err[10000]
    finally:
        tidy(r)


def test_back_to_zero_after_a_kept_light_edit_drops_the_history(renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps, dim = cref.with_dim_row(cornell(*SIZE))
    r = renderer
    try:
        _switch(r, ps, dim, PCT, before=2)
        r.set_option("temporal_clip_pct", 0)
        _, hw = r.denoise_temporal(history=True)
        assert (hw == SPP).all()
        tidy(r)
        # the record clears with the history: a later light edit under 0 drops, and 100 -> 0 without one does not
        r.set_option("temporal_clip_pct", PCT)
        cams = orbit_cameras(ps.camera, 64)
        frame(r, cams[0], 0)
        r.denoise_temporal()
        frame(r, cams[1], 1)                                    # a camera move alone
        r.set_option("temporal_clip_pct", 0)
        _, hw = r.denoise_temporal(history=True)
        assert (hw > SPP).mean() > 0.5
        refused(r.debug_read_clip_box, ESTATE)
    finally:
        tidy(r)


# ------------------------------------------------------------------ 8. a failed allocation
def _with_failure(k):
    """Frame 0 filtered with the option off; on frame 1 the option goes on and the k-th allocation of the call fails
    (k = 0: none).  Returns the call's outputs and boxes on frames 1 and 2."""
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(*SIZE)
    cams = orbit_cameras(ps.camera, 64)
    out = ()
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2")
        try:
            frame(r, cams[0], 0)
            r.denoise_temporal()
            frame(r, cams[1], 1)
            r.set_option("temporal_clip_pct", PCT)
            if k:
                r.set_option("debug_fail_alloc", k)
                with pytest.raises(CrtError) as e:
                    r.denoise_temporal()
                r.set_option("debug_fail_alloc", 0)
                assert e.value.code == ENOMEM
                refused(r.debug_read_clip_box, ESTATE)          # CURRENT is still frame 0's
            for j in (1, 2):
                if j == 2:
                    frame(r, cams[2], 2)
                out += r.denoise_temporal(rgb=True, history=True) + (r.debug_read_clip_box(),)
        finally:
            r.set_option("debug_fail_alloc", 0)
    return out


@pytest.fixture(scope="module")
def uninjected():
    return _with_failure(0)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_a_failed_allocation_leaves_the_slots_as_they_were(k, uninjected):
    """The call's allocations on a context that has filtered one frame without the option: the box buffer (k = 1), then
    the G-buffer and keys of the guide set the new frame is built into."""
    a = _with_failure(k)
    assert same(a, uninjected) and (a[2] > SPP).mean() > 0.5 and (a[6] > 2 * SPP).mean() > 0.5


# ------------------------------------------------------------------ 9. read-only
def test_it_changes_nothing_a_render_depends_on(orc):
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd.scene import PackedScene, orbit_cameras
    ps = cornell(*SIZE)
    cams = orbit_cameras(ps.camera, 64)

    def run(call):
        with Renderer(0) as r:
            r.upload(ps).build_accel("bvh2").enable_counters(True).set_option("temporal_clip_pct", PCT)
            frame(r, cams[0], 0)
            if call:
                r.denoise_temporal()
            r.set_camera(cams[1]).set_sample_offset(4).frame(3).sync()
            before = r.counters()
            if call:
                r.denoise_temporal()
                svgf_all(r, 0)
                assert (r.debug_read_clip_box()[..., 7] == 1).mean() > 0.5
            assert r.counters() == before
            mid = (r.read_accum(), r.read_rgba8(), r.sample, before)
            r.frame(2).sync()
            return mid + (r.read_accum(), r.read_rgba8(), r.sample, r.counters(), r.sample_offset)
    a, b = run(True), run(False)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(bits(x) if x.dtype == F else x, bits(y) if y.dtype == F else y)
        elif isinstance(x, dict):
            assert {k: x[k] for k in PATH_COUNTERS} == {k: y[k] for k in PATH_COUNTERS}
        else:
            assert x == y
    sk = PackedScene(ps.primitives, ps.lights, cams[1].copy(), ps.spectra, ps.cie, ps.patches, ps.spectrum_index)
    want = orc.Scene.from_packed(sk).render(5, first_sample=5)[0]
    assert np.array_equal(bits(a[4])[..., :3], bits(want)[..., :3])


# ------------------------------------------------------------------ 10. the hook's refusals
def test_the_hook_refuses_without_a_box_pass():
    import ctypes as C
    from computeraytracer_amd import Renderer, _lib, cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(*SIZE)
    cams = orbit_cameras(ps.camera, 64)
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2").set_option("temporal_clip_pct", PCT)
        assert r._lib.crt_debug_read_clip_box(r._h, None) == EINVAL
        frame(r, cams[0], 0)
        refused(r.debug_read_clip_box, ESTATE, "crt_debug_read_clip_box")       # before any temporal call
        r.denoise_temporal()
        refused(r.debug_read_clip_box, ESTATE)                                  # the first frame: no PREVIOUS
        frame(r, cams[1], 1)
        refused(r.debug_read_clip_box, ESTATE)                                  # no call in this frame yet
        r.denoise_svgf()
        assert r.debug_read_clip_box().shape == (76, 100, 8)
        r.set_option("temporal_clip_pct", 0)
        refused(r.debug_read_clip_box, ESTATE)                                  # the option off ...
        r.denoise_temporal()
        refused(r.debug_read_clip_box, ESTATE)                                  # ... and a call that ran without it
        r.set_option("temporal_clip_pct", PCT)
        refused(r.debug_read_clip_box, ESTATE)
        r.denoise_temporal()
        r.debug_read_clip_box()
        r.reset()
        refused(r.debug_read_clip_box, ESTATE)                                  # the accumulator was zeroed
        r.set_sample_offset(8).frame(SPP).sync()
        refused(r.debug_read_clip_box, ESTATE)
    assert _lib.load().crt_debug_read_clip_box(None, C.c_void_p()) == EINVAL
