"""GPU tests of crt_denoise_temporal (include/crt.h "Temporal reuse across camera moves"; run with -m gpu on
an MI355X): without history it is crt_denoise bit for bit; with history the blend is the float64 restatement of
tests/denoise_temporal_ref.py fed the GPU's own accumulators, G-buffers, camera frames and previous slot, and the passes
after it are denoise_ref.atrous on the GPU's own blend; the history lives and dies by the rules of the header; the call
changes nothing a render depends on; and on an orbit it beats the spatial filter by the margin of the CPU test."""
import numpy as np
import pytest

import denoise_ref as ref
import denoise_temporal_ref as tref
from conftest import bits
from test_denoise_temporal_cpu import ORBIT, assert_orbit_bounds, orbit_quality, orbit_scenes

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 1e-4                                                   # the project's bound for float64 restatements


def cam_frame(orc, cam):
    out = np.zeros(12, np.float32)
    cam = np.ascontiguousarray(cam, np.float32)
    orc.lib().orc_camera_frame(cam.ctypes.data, out.ctypes.data)
    return out


def with_camera(ps, cam):
    from computeraytracer_amd.scene import PackedScene
    return PackedScene(ps.primitives, ps.lights, np.asarray(cam, np.float32).copy(), ps.spectra, ps.cie, ps.patches, ps.spectrum_index)


def assert_equals_plain_denoise(r, n, iterations=5):
    """Test 2: no history -> crt_denoise bit for bit, and history_out == n everywhere."""
    rgba, rgb, hw = r.denoise_temporal(iterations, rgb=True, history=True)
    want_rgba, want_rgb = r.denoise(iterations, rgb=True)
    assert np.array_equal(bits(rgb[..., :3]), bits(want_rgb[..., :3])) and np.array_equal(rgba, want_rgba)
    assert (hw == n).all() and np.array_equal(bits(rgb[..., 3]), bits(hw))


def check_frame(r, orc, ps, cam, prev, rect=None, **params):
    """One frame of the context against the restatement: K = 0 (the blend) against blend() fed `prev`, K = 5 against
    denoise_ref.atrous on the GPU's own blend.  Returns (the slot this frame leaves, share of pixels left out, Hw)."""
    W, Hh = int(ps.camera[11]), int(ps.camera[12])
    x0, y0 = (rect[0], rect[1]) if rect else (0, 0)
    n = r.sample
    acc, g = r.read_accum(), r.read_gbuffer()
    key, frame = ref.keys(g, ps.primitives), cam_frame(orc, cam)
    blend_params = {k: v for k, v in params.items() if k in tref.BLEND}
    rgba0, rgb0, hw0 = r.denoise_temporal(0, rgb=True, history=True, **params)
    want, want_hw, doubt = tref.blend(ref.linear_rgb(acc, n), n, g[..., 1:4], g[..., 4:7], key, frame, prev, W, Hh, x0, y0,
                                      **dict({k: tref.DEFAULTS[k] for k in tref.BLEND}, **blend_params))
    keep = ~doubt
    err = (np.abs(rgb0[..., :3] - want) / np.maximum(1.0, np.abs(want)))[keep]
    herr = (np.abs(hw0 - want_hw) / want_hw)[keep]
    d0 = np.abs(rgba0.astype(np.int32) - ref.to_rgba8(want).astype(np.int32))[keep]
    print(f"{g.shape[1]}x{g.shape[0]} n {n}: left out {doubt.mean():.5f}; K=0 colour max rel err {err.max():.3g}, "
          f"Hw {herr.max():.3g}, rgba8 max {d0.max()}; reused {float((want_hw > n).mean()):.4f}")
    assert doubt.mean() <= 0.02
    assert err.max() <= TOL and herr.max() <= TOL and d0.max() <= 1
    assert np.array_equal(bits(rgb0[..., 3]), bits(hw0))
    # the passes after the blend: the existing filter on the GPU's own blend
    filt = {k: v for k, v in params.items() if k not in tref.BLEND}
    rgba5, rgb5, hw5 = r.denoise_temporal(5, rgb=True, history=True, **params)
    want5 = ref.atrous(rgb0[..., :3], g[..., 1:4], g[..., 4:7], key, **dict(ref.DEFAULTS, iterations=5, **filt))
    err5 = np.abs(rgb5[..., :3] - want5) / np.maximum(1.0, np.abs(want5))
    d5 = np.abs(rgba5.astype(np.int32) - ref.to_rgba8(want5).astype(np.int32))
    print(f"    K=5 colour max rel err {err5.max():.3g}, rgba8 max {d5.max()}")
    assert err5.max() <= TOL and d5.max() <= 1
    assert np.array_equal(bits(hw5), bits(hw0)) and np.array_equal(bits(rgb5[..., 3]), bits(hw0))
    return tref.slot(rgb0, hw0, g, key, frame), float(doubt.mean()), hw0


def run_orbit(r, orc, ps, cams, spp, rect=None, **params):
    prev, hw = None, None
    for k, cam in enumerate(cams):
        r.set_camera(cam).set_sample_offset(k * spp).frame(spp).sync()
        if k == 0:
            assert_equals_plain_denoise(r, spp)                 # (also makes this frame's slot)
        prev, _, hw = check_frame(r, orc, with_camera(ps, cam), cam, prev, rect, **params)
    return prev, hw


def tidy(r):
    r.temporal_reset().reset().set_sample_offset(0)


# ------------------------------------------------------------------ 2 + 3. the restatement
@pytest.mark.parametrize("frames", [2, 3])
def test_blend_matches_the_reference_cornell(renderer, orc, frames):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    try:
        renderer.upload(ps).build_accel("bvh2")
        _, hw = run_orbit(renderer, orc, ps, orbit_cameras(ps.camera, 64)[:frames], 4)
        assert hw.max() == 4 * frames and (hw > 4).mean() > 0.5
    finally:
        tidy(renderer)


def test_blend_matches_the_reference_other_parameters(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    try:
        renderer.upload(ps).build_accel("bvh2")
        _, hw = run_orbit(renderer, orc, ps, orbit_cameras(ps.camera, 64)[:3], 4, sigma_color=0.5, sigma_normal=0.25, sigma_plane=0.1,
                          max_history=6.0, normal_tol=0.1, plane_tol=0.5)
        assert hw.max() == 10.0                                # 4 + min(8, 6)
    finally:
        tidy(renderer)


def test_blend_matches_the_reference_atrium(renderer, orc):
    from computeraytracer_amd.scene import orbit_cameras
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(480, 270)
    try:
        renderer.upload(ps).build_accel("bvh2")
        run_orbit(renderer, orc, ps, orbit_cameras(ps.camera, 64)[:3], 4)
    finally:
        tidy(renderer)


def test_tile_is_filtered_on_its_own(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(128, 96)
    try:
        renderer.upload(ps).set_tile(16, 8, 76, 62).build_accel("bvh2")      # 60 x 54 inside the image
        prev, hw = run_orbit(renderer, orc, ps, orbit_cameras(ps.camera, 64)[:3], 4, rect=(16, 8, 60, 54))
        assert hw.shape == (54, 60) and (hw > 4).mean() > 0.5
    finally:
        renderer.set_tile(0, 0, 128, 96)
        tidy(renderer)


# ------------------------------------------------------------------ 4. what is reused
def test_misses_and_glass_take_no_history_and_diffuse_hits_do(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(128, 128)
    cams = orbit_cameras(ps.camera, 64)
    try:
        renderer.upload(ps).build_accel("bvh2")
        for k in range(2):
            renderer.set_camera(cams[k]).set_sample_offset(4 * k).frame(4).sync()
            _, hw = renderer.denoise_temporal(history=True)
        key = ref.keys(renderer.read_gbuffer(), ps.primitives)
        miss, material = key == ref.MISS, (key >> np.uint64(24)) & np.uint64(3)
        glass, diffuse = ~miss & (material == 2), ~miss & (material == 0)
        assert miss.any() and diffuse.any()
        assert (hw[miss] == 4).all() and (hw[glass] == 4).all()
        share = float((hw[diffuse] > 4).mean())
        print(f"reused diffuse hits after a 1/64-turn step: {share:.4f} ({int(glass.sum())} glass pixels)")
        assert share >= 0.95
        assert hw.max() <= 8.0
    finally:
        tidy(renderer)


# ------------------------------------------------------------------ 5. calls within one frame
def test_twice_is_idempotent_and_more_samples_blend_against_the_same_previous(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = orbit_cameras(ps.camera, 64)
    try:
        renderer.upload(ps).build_accel("bvh2").set_camera(cams[0]).frame(4).sync()
        prev, _, _ = check_frame(renderer, orc, with_camera(ps, cams[0]), cams[0], None)
        renderer.set_camera(cams[1]).set_sample_offset(4).frame(4).sync()
        a = renderer.denoise_temporal(rgb=True, history=True)
        b = renderer.denoise_temporal(rgb=True, history=True)
        assert all(np.array_equal(bits(x) if x.dtype == F else x, bits(y) if y.dtype == F else y) for x, y in zip(a, b))
        assert (a[2] > 4).any()
        renderer.frame(4).sync()                               # more samples, the same frame: PREVIOUS is still frame 0's slot
        assert renderer.sample == 8
        _, _, hw = check_frame(renderer, orc, with_camera(ps, cams[1]), cams[1], prev)
        assert hw.max() == 12.0
    finally:
        tidy(renderer)


# ------------------------------------------------------------------ 6. what drops the history, and what keeps it
def _two_frames(r, ps, cams, spp=4):
    """History of frame 0 in CURRENT, frame 1 rendered and not yet filtered."""
    r.temporal_reset().set_camera(cams[0]).set_sample_offset(0).frame(spp).sync()
    r.denoise_temporal()
    r.set_camera(cams[1]).set_sample_offset(spp).frame(spp).sync()


def test_dropping_events(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(64, 48)
    cams = orbit_cameras(ps.camera, 64)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2")
        _two_frames(r, ps, cams)
        _, hw = r.denoise_temporal(history=True)
        assert (hw > 4).any()                                   # the set-up does reuse history ...
        events = {
            "temporal_reset": lambda: r.temporal_reset().reset().frame(4).sync(),
            "upload_scene": lambda: r.upload(ps).build_accel("bvh2").frame(4).sync(),
            "set_tile": lambda: r.set_tile(0, 0, 64, 48).frame(4).sync(),
            "set_row_bands": lambda: r.set_row_bands(8, 2, 0).set_tile(0, 0, 64, 48).frame(4).sync(),
            "update_primitives": lambda: (r.update_primitives(0, ps.primitives[:1]), r.refit_accel(), r.frame(4).sync()),
            "update_lights": lambda: r.update_lights(0, ps.lights[:1]).frame(4).sync(),
            "write_accum": lambda: r.write_accum(r.read_accum(), 4),
        }
        for name, event in events.items():                      # ... and after each of these the next call does not
            _two_frames(r, ps, cams)
            event()
            try:
                assert_equals_plain_denoise(r, r.sample)
            except AssertionError as e:
                raise AssertionError(f"history survived {name}") from e
        # what keeps it: crt_reset + another offset + the same camera, crt_build_accel, crt_refit_accel without an update
        keeps = {"reset": lambda: r.reset(), "build_accel": lambda: (r.build_accel("bvh2"), r.reset()),
                 "refit_accel": lambda: r.refit_accel()}
        for name, event in keeps.items():
            _two_frames(r, ps, cams)
            r.denoise_temporal()                                # frame 1's slot
            event()
            r.set_sample_offset(8).frame(4).sync()
            _, hw = r.denoise_temporal(history=True)
            assert (hw > 8).mean() > 0.4, f"history lost over {name}"       # 4 new + 8 of history where the pixel found itself
    finally:
        r.set_tile(0, 0, 64, 48)
        tidy(r)


def test_comm_partition_drops_the_history():
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(64, 48)
    cams = orbit_cameras(ps.camera, 64)
    with Renderer(0) as r:
        r.comm_init(Renderer.comm_unique_id(local=True), 0, 1).upload(ps).build_accel("bvh2")
        try:
            _two_frames(r, ps, cams)
            r.comm_partition(0)                                 # one rank, contiguous strips: the whole image
            r.frame(4).sync()
            assert_equals_plain_denoise(r, 4)
        finally:
            r.comm_destroy()


def test_reset_with_the_same_camera_matches_the_reference(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(100, 76)
    try:
        renderer.upload(ps).build_accel("bvh2").frame(4).sync()
        prev, _, _ = check_frame(renderer, orc, ps, ps.camera, None)
        renderer.reset().set_sample_offset(4).frame(4).sync()
        _, _, hw = check_frame(renderer, orc, ps, ps.camera, prev)
        key = ref.keys(renderer.read_gbuffer(), ps.primitives)
        diffuse = (key != ref.MISS) & ((key >> np.uint64(24)) == 0)
        assert (hw[diffuse] == 8).mean() > 0.95                # an unchanged camera: a pixel finds itself
    finally:
        tidy(renderer)


def test_a_plain_denoise_of_a_skipped_frame_does_not_mix_up_the_guides(renderer, orc):
    """Frame 0 filtered temporally, frame 1 with crt_denoise alone (its G-buffer replaces frame 0's), frame 2 temporally
    again: PREVIOUS is frame 0's slot with frame 0's guides."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = orbit_cameras(ps.camera, 64)
    try:
        renderer.upload(ps).build_accel("bvh2").set_camera(cams[0]).frame(4).sync()
        prev, _, _ = check_frame(renderer, orc, with_camera(ps, cams[0]), cams[0], None)
        renderer.set_camera(cams[1]).set_sample_offset(4).frame(4).sync()
        renderer.denoise()
        renderer.set_camera(cams[2]).set_sample_offset(8).frame(4).sync()
        check_frame(renderer, orc, with_camera(ps, cams[2]), cams[2], prev)
    finally:
        tidy(renderer)


# ------------------------------------------------------------------ 7. read-only, and the refusals
# The counters that depend on the paths alone.  "nodes" and "prims" also depend on which walk served a ray -- the wide tree
# in the pool, or the BVH2 in k_wf_finish for the stragglers the host moved aside, a matter of timing -- and differ
# between any two runs of the same render (which is why no test compares them with the oracle either).
PATH_COUNTERS = ("rays", "paths", "bounces", "shadow", "hits", "walked")


def test_it_changes_nothing_a_render_depends_on(orc):
    """Within the context every counter is the same before and after the call; against a context that never called it
    the accumulator, rgba8, sample count, frame ring, the counters of PATH_COUNTERS and the samples traced next are equal."""
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(100, 76)

    def run(call):
        with Renderer(0) as r:
            r.upload(ps).build_accel("bvh2").enable_counters(True).set_option("frame_ring", 4)
            r.reset().set_sample_offset(4).frame(3).sync()
            before = r.counters()
            if call:
                r.denoise_temporal()
                r.denoise_temporal(0, rgb=True, history=True)
            assert r.counters() == before                      # all eight
            mid = (r.read_accum(), r.read_rgba8(), r.sample, before, r.read_sample_rgba8(3))
            r.frame(2).sync()
            before = r.counters()
            if call:
                r.denoise_temporal()
            assert r.counters() == before
            return mid + (r.read_accum(), r.read_rgba8(), r.sample, before, r.read_sample_rgba8(5), r.sample_offset)
    a, b = run(True), run(False)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(bits(x) if x.dtype == F else x, bits(y) if y.dtype == F else y)
        elif isinstance(x, dict):
            assert {k: x[k] for k in PATH_COUNTERS} == {k: y[k] for k in PATH_COUNTERS}
        else:
            assert x == y
    want = orc.Scene.from_packed(ps).render(5, first_sample=5)[0]
    assert np.array_equal(bits(a[5])[..., :3], bits(want)[..., :3])


def test_denoise_temporal_refuses_what_it_cannot_do():
    import ctypes as C
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError, DenoiseTemporalParams
    ps = cornell(64, 48)
    with Renderer(0) as r:
        lib, h = r._lib, r._h
        buf = np.zeros((48, 64, 4), np.uint8)

        def refused(match=None):
            with pytest.raises(CrtError, match=match) as e:
                r.denoise_temporal()
            assert e.value.code == -3
        r.upload(ps)
        refused("accel")                                       # no tree
        r.build_accel("bvh2")
        refused("no sample")                                   # sample 0
        r.frame(4).sync()
        r.denoise_temporal()
        assert lib.crt_denoise_temporal(h, None, None, buf.ctypes.data, None) == 0           # NULL = the defaults
        assert np.array_equal(buf, r.denoise_temporal())
        assert lib.crt_denoise_temporal(h, None, None, None, None) == 0                      # every output may be NULL
        r.set_camera(ps.camera).set_sample_offset(4).frame(4).sync()
        rgba, hw = r.denoise_temporal(history=True)
        good = [5, 1.0, 0.5, 0.3, 64.0, 0.5, 2.0]
        bad = [[11] + good[1:]]
        for i in range(1, 7):
            for v in (0.0, -1.0, float("nan"), float("inf")):
                bad.append(good[:i] + [v] + good[i + 1:])
        for p in bad:                                          # CRT_EINVAL, context and history unchanged
            assert lib.crt_denoise_temporal(h, C.byref(DenoiseTemporalParams(*p)), None, buf.ctypes.data, None) == -1, p
        rgba2, hw2 = r.denoise_temporal(history=True)
        assert np.array_equal(rgba, rgba2) and np.array_equal(bits(hw), bits(hw2)) and (hw > 4).any()
        r.denoise_temporal(iterations=10)                      # the largest allowed
        r.update_primitives(0, ps.primitives[:1])
        r.set_sample_offset(0)
        refused("refit")                                       # a stale tree
        r.refit_accel()
        assert r.trace_adaptive(samples=4, min_samples=4) > 0
        refused("adaptive state")
        r.set_row_bands(8, 2, 1).frame(2).sync()
        refused("row-band")
        r.set_tile(0, 0, 64, 48).frame(2).sync()
        assert r.denoise_temporal().shape == (48, 64, 4)


# ------------------------------------------------------------------ 8. quality on the product's own renders
def test_temporal_reuse_beats_the_filter_alone_on_the_products_orbit(renderer, orc):
    """The set-up and bounds of tests/test_denoise_temporal_cpu.py on this context's renders: the MSEs are those of
    crt_denoise_temporal and crt_denoise themselves (K = 5, the defaults) against 1024 samples of the same context."""
    scenes = orbit_scenes()
    o = ORBIT
    r = renderer

    def product(same):
        r.temporal_reset()
        for k in range(o["frames"]):
            r.set_camera(scenes[k].camera).set_sample_offset(0 if same else o["spp"] * k).frame(o["spp"]).sync()
            _, rgb, hw = r.denoise_temporal(rgb=True, history=True)
        noisy = ref.linear_rgb(r.read_accum(), o["spp"])
        _, plain = r.denoise(rgb=True)
        key = ref.keys(r.read_gbuffer(), scenes[-1].primitives)
        diffuse = (key != ref.MISS) & ((key >> np.uint64(24)) == 0)
        return noisy, plain[..., :3], rgb[..., :3], float((hw > o["spp"])[diffuse].mean())
    try:
        r.upload(scenes[0]).build_accel("bvh2")
        runs = [product(False), product(True)]
        r.set_camera(scenes[-1].camera).set_sample_offset(o["truth_first"] - 1).frame(o["truth_spp"]).sync()
        truth = ref.linear_rgb(r.read_accum(), o["truth_spp"])
        res = [(ref.mse_display(n, truth), ref.mse_display(p, truth), ref.mse_display(t, truth), share) for n, p, t, share in runs]
        assert_orbit_bounds(*res)
    finally:
        tidy(r)


def test_the_restatement_on_the_products_renders_gives_the_cpu_figures(renderer, orc):
    """orbit_quality (the float64 restatement end to end) on accumulators and G-buffers read back from the context."""
    scenes = orbit_scenes()
    o = ORBIT
    r = renderer
    try:
        r.upload(scenes[0]).build_accel("bvh2")

        def frame_of(k, first):
            r.set_camera(scenes[k].camera).set_sample_offset(first - 1).frame(o["spp"]).sync()
            g = r.read_gbuffer()
            return r.read_accum(), g, ref.keys(g, scenes[k].primitives), cam_frame(orc, scenes[k].camera)

        def truth_of(k):
            r.set_camera(scenes[k].camera).set_sample_offset(o["truth_first"] - 1).frame(o["truth_spp"]).sync()
            return ref.linear_rgb(r.read_accum(), o["truth_spp"])
        assert_orbit_bounds(orbit_quality(frame_of, truth_of, False), orbit_quality(frame_of, truth_of, True))
    finally:
        tidy(r)
