"""GPU tests of temporal reuse across primitive edits (include/crt.h option "temporal_motion" and crt_read_motion,
DESIGN.md 6f; run with -m gpu on an MI355X): the blend after crt_update_primitives is the float64 restatement of
tests/denoise_motion_ref.py fed the GPU's own accumulators, G-buffers, camera frames, previous slot and the two record
arrays; crt_read_motion is that restatement's film position rounded to float; with the option on and nothing moved every
output is bit for bit the option-off one; lights, changed spectra, the option itself and a failed allocation drop or
refuse as the header says; the calls change nothing a render depends on; and on an animated Cornell box the reuse beats
the spatial filter by the margins of the CPU test."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_motion_ref as mref
import denoise_ref as ref
import denoise_temporal_ref as tref
from conftest import ROOT, bits
from test_denoise_motion_cpu import MOTION, assert_motion_bounds
from test_denoise_temporal_gpu import PATH_COUNTERS, TOL, cam_frame

pytestmark = pytest.mark.gpu
F = np.float32
SPP = 4


def tidy(r):
    r.set_option("temporal_motion", 0)
    r.temporal_reset().reset().set_sample_offset(0)


def send(r, new, old):
    """The records of `new` that differ from `old`, one update per run of consecutive indices, then one refit."""
    changed = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(new, old)])
    for run in np.split(changed, np.flatnonzero(np.diff(changed) != 1) + 1):
        if len(run):
            r.update_primitives(int(run[0]), new[run[0]:run[-1] + 1])
    r.refit_accel()


def uv_agree(got, want_u, want_v):
    """crt_read_motion against the restatement: NaN exactly where it has no position, else within one float ulp."""
    want = np.stack([want_u, want_v], -1)
    none = np.isnan(want)
    assert np.array_equal(np.isnan(got), none)
    w32 = want.astype(F)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - w32.astype(np.float64))[~none]
        ulp = np.spacing(np.abs(w32)).astype(np.float64)[~none]
    print(f"    read_motion: {int((~none[..., 0]).sum())} positions, worst error {float((err / ulp).max()) if err.size else 0:.2f} ulp")
    assert (err <= ulp).all()


def check_frame(r, orc, cam, prims, prev, rect=None, size=None):
    """One frame of the context against the restatement (tests/test_denoise_temporal_gpu.check_frame with the map):
    K = 0 against mref.blend fed `prev` and the two record arrays, crt_read_motion against its (u, v), K = 5 against
    denoise_ref.atrous on the GPU's own blend.  Returns (the slot this frame leaves, Hw, G-buffer)."""
    W, Hh = size
    x0, y0 = (rect[0], rect[1]) if rect else (0, 0)
    n = r.sample
    acc, g = r.read_accum(), r.read_gbuffer()
    key, frame = ref.keys(g, prims), cam_frame(orc, cam)
    rgba0, rgb0, hw0 = r.denoise_temporal(0, rgb=True, history=True)
    uv = r.read_motion()
    old = prev["prims"] if prev is not None else None
    want, want_hw, doubt, u, v = mref.blend(ref.linear_rgb(acc, n), n, g, key, frame, prev, prims, old, W, Hh, x0, y0)
    keep = ~doubt
    err = (np.abs(rgb0[..., :3] - want) / np.maximum(1.0, np.abs(want)))[keep]
    herr = (np.abs(hw0 - want_hw) / want_hw)[keep]
    d0 = np.abs(rgba0.astype(np.int32) - ref.to_rgba8(want).astype(np.int32))[keep]
    print(f"{g.shape[1]}x{g.shape[0]} n {n}: left out {doubt.mean():.5f}; K=0 colour max rel err {err.max():.3g}, "
          f"Hw {herr.max():.3g}, rgba8 max {d0.max()}; reused {float((want_hw > n).mean()):.4f}")
    assert doubt.mean() <= 0.02
    assert err.max() <= TOL and herr.max() <= TOL and d0.max() <= 1
    assert np.array_equal(bits(rgb0[..., 3]), bits(hw0))
    uv_agree(uv, u, v)                                          # (pixels in doubt are not exempt here)
    rgba5, rgb5, hw5 = r.denoise_temporal(5, rgb=True, history=True)
    want5 = ref.atrous(rgb0[..., :3], g[..., 1:4], g[..., 4:7], key, **dict(ref.DEFAULTS, iterations=5))
    err5 = np.abs(rgb5[..., :3] - want5) / np.maximum(1.0, np.abs(want5))
    d5 = np.abs(rgba5.astype(np.int32) - ref.to_rgba8(want5).astype(np.int32))
    print(f"    K=5 colour max rel err {err5.max():.3g}, rgba8 max {d5.max()}")
    assert err5.max() <= TOL and d5.max() <= 1
    assert np.array_equal(bits(hw5), bits(hw0))
    assert np.array_equal(bits(r.read_motion()), bits(uv))     # the same slots: the same answer
    return mref.slot(rgb0, hw0, g, key, frame, prims), hw0, g


def run_animation(r, orc, ps, cams, frames, rect=None):
    """`frames` frames of SPP samples: before frame k > 0 the records of mref.animate(k) are sent.  Every frame is
    checked; returns the list of (Hw, G-buffer)."""
    size = (int(ps.camera[11]), int(ps.camera[12]))
    prev, prims, out = None, ps.primitives, []
    r.set_option("temporal_motion", 1)
    for k in range(frames):
        if k:
            new = mref.animate(ps.primitives, k)
            send(r, new, prims)
            prims = new
        r.set_camera(cams[k]).set_sample_offset(SPP * k).frame(SPP).sync()
        prev, hw, g = check_frame(r, orc, cams[k], prims, prev, rect, size)
        out.append((hw, g))
    return out


# ------------------------------------------------------------------ 1 + 2. the blend and the motion output
@pytest.mark.parametrize("accel", ["bvh2", "lbvh"])
@pytest.mark.parametrize("orbit", [False, True])
def test_blend_and_motion_match_the_reference(renderer, orc, orbit, accel):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = orbit_cameras(ps.camera, 64) if orbit else [ps.camera] * 3
    try:
        renderer.upload(ps).build_accel(accel)
        res = run_animation(renderer, orc, ps, cams, 3)
        hw1, g1 = res[1]
        key = ref.keys(g1, ps.primitives)
        on_moved = mref.moved_mask(g1) & (key != ref.MISS) & ((key >> np.uint64(24)) == 0)
        share = float((hw1 > SPP)[on_moved].mean())
        print(f"frame 1: {int(on_moved.sum())} diffuse pixels on moved primitives, {share:.4f} reuse history")
        assert on_moved.sum() > 200 and share >= 0.95
        assert res[2][0].max() == 3 * SPP
    finally:
        tidy(renderer)


def test_motion_with_the_option_off_is_the_camera_reprojection(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = orbit_cameras(ps.camera, 64)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2")
        for k in range(2):
            r.set_camera(cams[k]).set_sample_offset(SPP * k).frame(SPP).sync()
            r.denoise_temporal()
            uv = r.read_motion()
            if k == 0:
                assert np.isnan(uv).all()                      # no PREVIOUS slot
        g = r.read_gbuffer()
        key = ref.keys(g, ps.primitives)
        u, v, c = tref.reproject(cam_frame(orc, cams[0]), g[..., 1:4], 100, 76)
        placed = (key != ref.MISS) & ((key >> np.uint64(24)) != tref.GLASS) & (c > 0) & np.isfinite(c)
        assert placed.mean() > 0.5
        uv_agree(uv, np.where(placed, u, np.nan), np.where(placed, v, np.nan))
    finally:
        tidy(r)


# ------------------------------------------------------------------ 3. nothing moved: bit for bit the option-off run
def test_without_a_real_edit_the_option_changes_no_bit(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(100, 76)
    cams = orbit_cameras(ps.camera, 64)
    r = renderer

    def run(option, edit):
        r.temporal_reset().set_option("temporal_motion", option)
        out = []
        for k in range(3):
            if k and edit:
                r.update_primitives(0, ps.primitives[:1])
                r.refit_accel()
            r.set_camera(cams[k]).set_sample_offset(SPP * k).frame(SPP).sync()
            rgba, rgb, hw = r.denoise_temporal(rgb=True, history=True)
            out.append((rgba, bits(rgb), bits(hw), bits(r.read_motion())))
        return out
    try:
        r.upload(ps).build_accel("bvh2")
        off = run(0, False)
        assert (off[2][2].view(F) > SPP).mean() > 0.5
        for name, got in (("option on, no edit", run(1, False)), ("option on, identical records rewritten", run(1, True))):
            for k in range(3):
                for a, b in zip(off[k], got[k]):
                    assert np.array_equal(a, b), f"{name}: frame {k} differs"
    finally:
        tidy(r)


# ------------------------------------------------------------------ 4. what still drops or refuses
def _history_then_edit(r, ps, new=None):
    """Frame 0 filtered (its slot is CURRENT), then an edit and frame 1 rendered, not yet filtered."""
    r.temporal_reset().reset().set_sample_offset(0).frame(SPP).sync()
    r.denoise_temporal()
    if new is not None:
        send(r, new, ps.primitives)


def _equals_plain_denoise(r):
    rgba, rgb, hw = r.denoise_temporal(rgb=True, history=True)
    want_rgba, want_rgb = r.denoise(rgb=True)
    assert np.array_equal(bits(rgb[..., :3]), bits(want_rgb[..., :3])) and np.array_equal(rgba, want_rgba)
    assert (hw == r.sample).all()


def test_what_still_drops_or_refuses(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd._lib import CrtError
    ps = cornell(100, 76)
    moved = mref.animate(ps.primitives, 1)
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_motion", 1)
        # the set-up does keep history over an edit ...
        _history_then_edit(r, ps, moved)
        r.set_sample_offset(SPP).frame(SPP).sync()
        rgba_kept, hw_kept = r.denoise_temporal(history=True)
        assert (hw_kept > SPP).mean() > 0.5
        send(r, ps.primitives, moved)
        # ... crt_update_lights drops it in both modes
        _history_then_edit(r, ps)
        r.update_lights(0, ps.lights[:1]).set_sample_offset(SPP).frame(SPP).sync()
        _equals_plain_denoise(r)
        # the option set back to 0 after an edit drops it
        _history_then_edit(r, ps, moved)
        r.set_option("temporal_motion", 0).set_sample_offset(SPP).frame(SPP).sync()
        _equals_plain_denoise(r)
        r.set_option("temporal_motion", 1)
        send(r, ps.primitives, moved)
        # a record whose reflectance index changed takes no history on its pixels; the others do
        white = ps.primitives.copy()
        assert white[4]["data4"][1] == 2                      # the red wall ...
        white["data4"][4, 1] = 0                                # ... painted white
        _history_then_edit(r, ps, white)
        r.set_sample_offset(SPP).frame(SPP).sync()
        _, hw = r.denoise_temporal(history=True)
        uv = r.read_motion()
        idx = mref.hit_index(r.read_gbuffer())
        wall, floor = idx == 4, idx == 0
        assert wall.sum() > 100 and floor.sum() > 100
        assert (hw[wall] == SPP).all() and np.isnan(uv[wall]).all()
        assert (hw[floor] > SPP).mean() > 0.95 and not np.isnan(uv[floor]).any()
        send(r, ps.primitives, white)
        # the refusals
        with pytest.raises(CrtError) as e:
            r.set_option("temporal_motion", 2)
        assert e.value.code == -1
        r.reset().frame(SPP).sync()
        with pytest.raises(CrtError) as e:                      # no crt_denoise_temporal in this frame yet
            r.read_motion()
        assert e.value.code == -3
        assert r._lib.crt_read_motion(r._h, None) == -1 and r._lib.crt_read_motion(None, None) == -1
        # a snapshot that cannot be allocated: CRT_ENOMEM, and context, scene and history are as they were
        r.temporal_reset().reset().set_sample_offset(0).frame(SPP).sync()
        r.denoise_temporal()
        r.reset().set_sample_offset(SPP).frame(SPP).sync()
        want = r.denoise_temporal(rgb=True, history=True)
        assert (want[2] > SPP).mean() > 0.5
        r.temporal_reset().reset().set_sample_offset(0).frame(SPP).sync()
        r.denoise_temporal()
        r.set_option("debug_fail_alloc", 1)
        with pytest.raises(CrtError) as e:
            r.update_primitives(BOX0, moved[mref.BOX])
        r.set_option("debug_fail_alloc", 0)
        assert e.value.code == -4                               # CRT_ENOMEM
        r.reset().set_sample_offset(SPP).frame(SPP).sync()
        got = r.denoise_temporal(rgb=True, history=True)
        for a, b in zip(want, got):
            assert np.array_equal(bits(a) if a.dtype == F else a, bits(b) if b.dtype == F else b)
    finally:
        r.set_option("debug_fail_alloc", 0)
        tidy(r)


BOX0 = mref.BOX.start


# ------------------------------------------------------------------ 5. a rectangle
def test_a_rectangle_is_mapped_in_its_own_coordinates(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(128, 96)
    try:
        renderer.upload(ps).set_tile(16, 8, 76, 62).build_accel("bvh2")
        res = run_animation(renderer, orc, ps, [ps.camera] * 2, 2, rect=(16, 8, 60, 54))
        hw, g = res[1]
        assert hw.shape == (54, 60) and (hw > SPP).mean() > 0.5
        assert mref.moved_mask(g).sum() > 20                    # (the sphere and a corner of the box lie inside)
    finally:
        renderer.set_tile(0, 0, 128, 96)
        tidy(renderer)


# ------------------------------------------------------------------ 6. triangles
def test_a_moved_mesh_matches_the_reference(renderer, orc):
    from computeraytracer_amd import scene as S
    sc = S.load_scene(os.path.join(ROOT, "scenes", "cornell_mesh.json"))
    sc["camera"]["width"], sc["camera"]["height"] = 100, 76
    ps = S.pack_scene(sc, base_dir=os.path.join(ROOT, "scenes"))
    tri = np.flatnonzero(ps.primitives["category"] == mref.TRIANGLE)
    assert len(tri) == 8 and (np.diff(tri) == 1).all()          # the octahedron: one connected block
    block = slice(int(tri[0]), int(tri[-1]) + 1)
    R = mref.rot_y(10.0)
    centre = ps.primitives[block]["data1"].astype(np.float64).mean(0)
    new = ps.primitives.copy()
    new[block] = S.transform_records(ps.primitives[block], R, mref.about(R, centre, (-25.0, 10.0, 5.0)))
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_motion", 1)
        r.frame(SPP).sync()
        prev, _, _ = check_frame(r, orc, ps.camera, ps.primitives, None, size=(100, 76))
        send(r, new, ps.primitives)
        r.set_sample_offset(SPP).frame(SPP).sync()
        _, hw, g = check_frame(r, orc, ps.camera, new, prev, size=(100, 76))
        idx = mref.hit_index(g).astype(np.int64)
        on_mesh = (idx >= block.start) & (idx < block.stop)
        share = float((hw > SPP)[on_mesh].mean())
        print(f"{int(on_mesh.sum())} pixels on the moved mesh, {share:.4f} reuse history")
        assert on_mesh.sum() > 100 and share >= 0.9
    finally:
        tidy(r)


# ------------------------------------------------------------------ 7. read-only
def test_it_changes_nothing_a_render_depends_on(orc):
    """Against a context that never sets the option nor calls crt_read_motion: accumulator, rgba8, sample count and the
    counters of PATH_COUNTERS are equal, before and after an edit."""
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(100, 76)
    moved = mref.animate(ps.primitives, 1)

    def run(call):
        with Renderer(0) as r:
            r.upload(ps).build_accel("bvh2").enable_counters(True)
            if call:
                r.set_option("temporal_motion", 1)
            r.frame(3).sync()
            before = r.counters()
            r.denoise_temporal()
            if call:
                r.read_motion()
            assert r.counters() == before
            mid = (r.read_accum(), r.read_rgba8(), r.sample, before)
            send(r, moved, ps.primitives)
            r.set_sample_offset(3).frame(2).sync()
            before = r.counters()
            r.denoise_temporal()
            if call:
                r.read_motion()
            assert r.counters() == before
            r.frame(2).sync()
            return mid + (r.read_accum(), r.read_rgba8(), r.sample, r.counters())
    a, b = run(True), run(False)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(bits(x) if x.dtype == F else x, bits(y) if y.dtype == F else y)
        elif isinstance(x, dict):
            assert {k: x[k] for k in PATH_COUNTERS} == {k: y[k] for k in PATH_COUNTERS}
        else:
            assert x == y


# ------------------------------------------------------------------ 8. quality on the product's own renders
@pytest.mark.parametrize("orbit", [False, True])
def test_reuse_across_edits_beats_the_filter_alone_on_the_products_renders(renderer, orc, orbit):
    """The set-up and bounds of tests/test_denoise_motion_cpu.py with crt_denoise_temporal and crt_denoise themselves
    (K = 5, the defaults) against 1024 samples of the same context.  (The control of the CPU test -- history kept and
    nothing mapped -- is something the library cannot be made to do: it stays with the restatement.)"""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    m = MOTION
    ps = cornell(m["size"], m["size"])
    cams = orbit_cameras(ps.camera, m["turn"]) if orbit else [ps.camera] * m["frames"]
    r = renderer
    last = m["frames"] - 1
    try:
        r.upload(ps).build_accel("bvh2").set_option("temporal_motion", 1)
        prims = ps.primitives
        for k in range(m["frames"]):
            if k:
                new = mref.animate(ps.primitives, k)
                send(r, new, prims)
                prims = new
            r.set_camera(cams[k]).set_sample_offset(m["spp"] * k).frame(m["spp"]).sync()
            _, rgb, hw = r.denoise_temporal(rgb=True, history=True)
        _, plain = r.denoise(rgb=True)
        g = r.read_gbuffer()
        key = ref.keys(g, prims)
        on_moved = mref.moved_mask(g)
        diffuse = on_moved & (key != ref.MISS) & ((key >> np.uint64(24)) == 0)
        share = float((hw > m["spp"])[diffuse].mean())
        r.reset().set_sample_offset(m["truth_first"] - 1).frame(m["truth_spp"]).sync()
        truth = ref.linear_rgb(r.read_accum(), m["truth_spp"])
        whole = ref.mse_display(rgb[..., :3], truth) / ref.mse_display(plain[..., :3], truth)
        part = ref.mse_display(rgb[..., :3][on_moved], truth[on_moved]) / ref.mse_display(plain[..., :3][on_moved], truth[on_moved])
        assert_motion_bounds("orbit" if orbit else "fixed", whole, part, None, share)
    finally:
        tidy(r)
