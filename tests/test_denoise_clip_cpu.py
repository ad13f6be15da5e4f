"""CPU-only checks of clipped history (include/crt.h "Clipped history", option "temporal_clip_pct"): the
interface exists at every layer; without a box the restatement (tests/denoise_clip_ref.py) is 6e's and 6f's, array for
array; the box and the clamp on synthetic arrays; and the two quality tables of 6l, re-measured with the float64
restatement on oracle renders: the animated Cornell box of tests/test_denoise_motion_cpu.py, and a light switched to a
sixteenth of its emission."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_clip_ref as cref
import denoise_motion_ref as mref
import denoise_ref as ref
import denoise_temporal_ref as tref
from conftest import ROOT
from test_denoise_motion_cpu import MOTION

NODE = shutil.which("node")
F = np.float32
DIFFUSE = np.uint64(7)                                          # a key: material 0, some reflectance index

SWEEP = (0, 50, 100, 150, 200, 300)                             # 0: the control, the history kept and not clipped
# MSE in display space of the last frame of MOTION against 1024 spp, temporal + filter over the filter alone,
# on (the whole image, the pixels of the moved primitives, the static pixels), per P.
MEASURED = {
    "fixed": {0: (0.38, 0.81, 0.36), 50: (0.51, 1.00, 0.49), 100: (0.48, 0.88, 0.47), 150: (0.47, 0.84, 0.46),
              200: (0.46, 0.82, 0.45), 300: (0.45, 0.81, 0.43)},
    "orbit": {0: (0.66, 0.66, 0.66), 50: (0.63, 0.67, 0.63), 100: (0.63, 0.64, 0.63), 150: (0.63, 0.64, 0.63),
              200: (0.63, 0.64, 0.63), 300: (0.62, 0.64, 0.62)},
}
# ... and the light switch: MSE in display space of the two frames after the switch against 1024 spp of the dim scene, for
# (the history dropped, kept, kept and clipped at P = DEFAULT_PCT, the value of a bare --clip): 0.0059 / 0.0173 / 0.0050 on the
# first frame, 0.0057 / 0.0129 / 0.0057 on the second.
DEFAULT_PCT = 100
SWITCH = dict(size=64, before=4, after=2, spp=4, truth_spp=1024, truth_first=100001)


# ------------------------------------------------------------------ 1. the interface
def test_header_declares_the_hook_and_the_option_and_the_bindings_have_them():
    from test_abi import declared_symbols
    from computeraytracer_amd import _lib
    from computeraytracer_amd.renderer import Renderer
    assert "crt_debug_read_clip_box" in declared_symbols() and "crt_debug_read_clip_box" in _lib.SIGNATURES
    assert callable(Renderer.debug_read_clip_box)
    assert _lib.load().crt_debug_read_clip_box(None, None) == -1
    with open(os.path.join(ROOT, "include", "crt.h")) as f:
        assert '"temporal_clip_pct"' in f.read()


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_the_hook():
    addon = os.path.join(ROOT, "addon", "crt_napi.node")
    assert os.path.exists(addon), "build the addon first (__graft_entry__.build())"
    js = "const a=require(%r);if(typeof a.debugReadClipBox!=='function') throw new Error('debugReadClipBox');console.log('ok')" % addon
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ------------------------------------------------------------------ 2. no box: the restatements that exist
@pytest.fixture(scope="module")
def two_frames(orc):
    """Two frames of the Cornell orbit at 64 x 48, 4 spp each: (c_new, gbuf, key, camera frame) per frame, and the scene."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import PackedScene, orbit_cameras
    W, Hh = 64, 48
    ps = cornell(W, Hh)
    cams = orbit_cameras(ps.camera, 64)
    frames = []
    for k in range(2):
        sk = PackedScene(ps.primitives, ps.lights, cams[k].copy(), ps.spectra, ps.cie, ps.patches, ps.spectrum_index)
        sc = orc.Scene.from_packed(sk)
        g, _ = ref.oracle_gbuffer(orc, sk, (0, 0, W, Hh))
        frames.append((ref.linear_rgb(sc.render(4, first_sample=4 * k + 1)[0], 4), g, ref.keys(g, ps.primitives), sc.camera_frame()))
    return ps, frames


def test_without_a_box_the_blend_is_the_one_of_6e_and_6f(two_frames):
    ps, ((c0, g0, k0, f0), (c1, g1, k1, f1)) = two_frames
    Hh, W = k0.shape
    prev = tref.slot(c0, np.full((Hh, W), 4.0), g0, k0, f0)
    want = tref.blend(c1, 4, g1[..., 1:4], g1[..., 4:7], k1, f1, prev, W, Hh)
    assert (want[1] > 4).mean() > 0.5
    got = cref.blend(c1, 4, g1, k1, f1, prev, W, Hh)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    moved = mref.animate(ps.primitives, 1)                      # the slot saw frame 0's records, the frame sees frame 1's
    want = mref.blend(c1, 4, g1, k1, f1, prev, moved, ps.primitives, W, Hh)
    got = cref.blend(c1, 4, g1, k1, f1, prev, W, Hh, prims_cur=moved, prims_prev=ps.primitives)
    for a, b in zip(want[:3], got):
        assert np.array_equal(a, b)
    # and no previous slot: the frame itself
    c, hw, doubt = cref.blend(c1, 4, g1, k1, f1, None, W, Hh, box=cref.box(c1, k1, 1.0))
    assert np.array_equal(c, c1) and (hw == 4).all() and not doubt.any()


def test_a_valid_box_only_moves_colours_into_it(two_frames):
    """Hw and doubt do not depend on the box, and the clipped blend lies between c_new and the box."""
    _, ((c0, g0, k0, f0), (c1, g1, k1, f1)) = two_frames
    Hh, W = k0.shape
    prev = tref.slot(c0, np.full((Hh, W), 4.0), g0, k0, f0)
    bx = cref.box(c1, k1, 1.0)
    lo, hi, _, valid = bx
    plain = cref.blend(c1, 4, g1, k1, f1, prev, W, Hh)
    clip = cref.blend(c1, 4, g1, k1, f1, prev, W, Hh, box=bx)
    assert np.array_equal(plain[1], clip[1]) and np.array_equal(plain[2], clip[2])
    used = valid & (clip[1] > 4)
    assert used.mean() > 0.5 and not np.array_equal(plain[0], clip[0])
    assert np.array_equal(plain[0][~used], clip[0][~used])
    eps = 1e-12
    assert (clip[0][used] >= np.minimum(c1, lo)[used] - eps).all() and (clip[0][used] <= np.maximum(c1, hi)[used] + eps).all()


# ------------------------------------------------------------------ 3. the box and the clamp on synthetic arrays
def _flat(h=12, w=12, value=(0.25, 0.5, 0.75)):
    return np.broadcast_to(np.asarray(value, np.float64), (h, w, 3)).copy(), np.full((h, w), DIFFUSE)


def test_a_constant_neighbourhood_pins_the_history_to_the_frame(two_frames):
    c, key = _flat()
    lo, hi, N, valid = cref.box(c, key, 1.0)
    assert valid.all() and np.array_equal(lo, c) and np.array_equal(hi, c)
    h = np.random.default_rng(1).uniform(0, 4, c.shape)
    assert np.array_equal(cref.clamp(h, (lo, hi, N, valid)), c)             # sigma = 0: h' = mu
    # ... and through the blend: a flat frame takes nothing from any history, c = c_new
    _, ((c0, g0, k0, f0), (_, g1, k1, f1)) = two_frames
    Hh, W = k1.shape
    flat = np.broadcast_to(np.asarray([0.25, 0.5, 0.75]), (Hh, W, 3)).copy()
    prev = tref.slot(c0, np.full((Hh, W), 4.0), g0, k0, f0)
    bx = cref.box(flat, k1, 3.0)
    got, hw, _ = cref.blend(flat, 4, g1, k1, f1, prev, W, Hh, box=bx)
    used = bx[3] & (hw > 4)
    assert used.mean() > 0.5 and np.abs(got - flat)[used].max() <= 1e-15
    assert np.abs(cref.blend(flat, 4, g1, k1, f1, prev, W, Hh)[0] - flat)[used].max() > 0.01


def test_fewer_than_four_taps_leave_the_history_alone():
    c, key = _flat()
    key[5, 5] = key[5, 6] = key[6, 5] = np.uint64(9)            # an island of three pixels with a key of their own
    c[5, 5], c[5, 6], c[6, 5] = (1, 1, 1), (2, 2, 2), (3, 3, 3)
    bx = cref.box(c, key, 1.0)
    lo, hi, N, valid = bx
    assert N[5, 5] == N[5, 6] == N[6, 5] == 3 and not valid[5, 5] and not valid[5, 6] and not valid[6, 5]
    assert valid.sum() == key.size - 3
    h = np.full(c.shape, 40.0)
    out = cref.clamp(h, bx)
    assert (out[5, 5] == 40).all() and (out[0, 0] == c[0, 0]).all()
    key[6, 6] = np.uint64(9)                                    # the fourth tap makes the box
    c[6, 6] = (2, 2, 2)
    lo, hi, N, valid = cref.box(c, key, 2.0)
    assert N[5, 5] == 4 and valid[5, 5]
    sigma = np.sqrt(((np.array([1, 2, 3, 2.0]) - 2.0) ** 2).sum() / 4)
    assert np.allclose(lo[5, 5], 2 - 2 * sigma, rtol=0, atol=1e-15) and np.allclose(hi[5, 5], 2 + 2 * sigma, rtol=0, atol=1e-15)


def test_a_tap_that_is_not_finite_is_skipped_and_such_a_centre_has_no_box():
    c, key = _flat()
    c[4, 4, 1] = np.nan
    c[4, 7, 0] = np.inf
    lo, hi, N, valid = cref.box(c, key, 1.0)
    assert N[4, 4] == 0 and not valid[4, 4] and (lo[4, 4] == 0).all() and (hi[4, 4] == 0).all()
    assert N[4, 7] == 0 and not valid[4, 7]
    assert N[5, 5] == 47 and N[4, 1] == 5 * 7 - 1 and N[11, 11] == 16
    ok = np.isfinite(c).all(-1)
    assert valid[ok].all() and np.array_equal(lo[ok], c[ok]) and np.array_equal(hi[ok], c[ok])     # nothing leaked in
    # a miss and glass have none either
    key[0, 0], key[0, 1] = ref.MISS, (np.uint64(tref.GLASS) << np.uint64(24)) | np.uint64(3)
    lo, hi, N, valid = cref.box(c, key, 1.0)
    assert N[0, 0] == 0 and N[0, 1] == 0 and not valid[0, 0] and not valid[0, 1]


def test_a_key_change_bounds_the_window():
    c, key = _flat(12, 16)
    key[:, 8:] = np.uint64(11)
    c[:, 8:] = (5.0, 6.0, 7.0)
    c[3, 9] = (9.0, 9.0, 9.0)
    lo, hi, N, valid = cref.box(c, key, 1.0)
    assert valid.all()
    assert np.array_equal(lo[:, :8], c[:, :8]) and np.array_equal(hi[:, :8], c[:, :8])     # the bright side is not seen
    assert N[6, 7] == 7 * 4 and N[6, 8] == 7 * 4 and N[6, 4] == 49 and N[6, 5] == 42
    assert hi[3, 8, 0] > 5.0 and (hi[3, 13:] == c[3, 13:]).all()


def test_the_rectangle_s_edge_bounds_the_window():
    rng = np.random.default_rng(3)
    big = rng.uniform(0, 1, (20, 24, 3))
    key = np.full((20, 24), DIFFUSE)
    y0, x0, hh, ww = 3, 5, 11, 13                               # a rectangle inside: its edges are borders
    lo, hi, N, valid = cref.box(big[y0:y0 + hh, x0:x0 + ww], key[y0:y0 + hh, x0:x0 + ww], 1.5)
    assert N[0, 0] == 16 and N[0, 3] == 28 and N[3, 3] == 49 and N[hh - 1, ww - 1] == 16 and N[hh - 1, 6] == 28
    win = big[y0:y0 + 4, x0:x0 + 4].reshape(-1, 3)
    mu, sg = win.mean(0), np.sqrt(((win - win.mean(0)) ** 2).mean(0))
    assert np.allclose(lo[0, 0], mu - 1.5 * sg, rtol=0, atol=1e-14) and np.allclose(hi[0, 0], mu + 1.5 * sg, rtol=0, atol=1e-14)
    lo_b, hi_b, N_b, _ = cref.box(big, key, 1.5)
    inner = (slice(3, hh - 3), slice(3, ww - 3))
    assert np.array_equal(lo[inner], lo_b[y0 + 3:y0 + hh - 3, x0 + 3:x0 + ww - 3])          # far from the edge: the same
    assert not np.array_equal(lo[0], lo_b[y0, x0:x0 + ww])


def test_clamping_twice_is_clamping_once():
    rng = np.random.default_rng(4)
    c = rng.uniform(0, 1, (10, 10, 3))
    key = np.full((10, 10), DIFFUSE)
    key[4, 4] = np.uint64(12)                                   # (one pixel without a valid box)
    bx = cref.box(c, key, 0.5)
    h = rng.uniform(-1, 3, c.shape)
    once = cref.clamp(h, bx)
    assert np.array_equal(cref.clamp(once, bx), once)
    assert (once[bx[3]] >= bx[0][bx[3]]).all() and (once[bx[3]] <= bx[1][bx[3]]).all() and not np.array_equal(once, h)
    assert np.array_equal(once[4, 4], h[4, 4])


# ------------------------------------------------------------------ 4. quality on the animated scene
def clip_quality(frame_of, truth_of, orbit):
    """The set-up of MOTION (tests/test_denoise_motion_cpu.py) with the history kept through the map of 6f and clipped at
    each P of SWEEP.  Returns {P: (whole image, moved primitives, static pixels)}: MSE ratios of temporal + filter over the
    filter alone on the last frame."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    m = MOTION
    W = Hh = m["size"]
    ps = cornell(W, Hh)
    cams = orbit_cameras(ps.camera, m["turn"]) if orbit else [ps.camera] * m["frames"]
    prev = {P: None for P in SWEEP}
    for k in range(m["frames"]):
        prims = mref.animate(ps.primitives, k)
        acc, g, key, frame = frame_of(k, cams[k], prims)
        res = {}
        for P in SWEEP:
            out, c, hw, _ = cref.temporal(acc, m["spp"], g, key, frame, prev[P], W, Hh, gamma=P / 100.0, prims_cur=prims)
            prev[P] = mref.slot(c, hw, g, key, frame, prims)
            res[P] = out
    plain = ref.atrous(ref.linear_rgb(acc, m["spp"]), g[..., 1:4], g[..., 4:7], key, **ref.DEFAULTS)
    truth = truth_of(cams[m["frames"] - 1], prims)
    on = mref.moved_mask(g)

    def ratio(img, mask):
        return ref.mse_display(img[mask], truth[mask]) / ref.mse_display(plain[mask], truth[mask])
    return {P: (ratio(res[P], np.ones_like(on)), ratio(res[P], on), ratio(res[P], ~on)) for P in SWEEP}


@pytest.mark.parametrize("orbit", [False, True])
def test_clipped_history_on_the_animated_scene(orc, orbit):
    """The first table of DESIGN.md 6l, re-measured with the final definition on oracle renders."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import PackedScene
    m = MOTION
    size = m["size"]
    base = cornell(size, size)

    def scene(cam, prims):
        return PackedScene(prims, base.lights, np.asarray(cam, F).copy(), base.spectra, base.cie, base.patches, base.spectrum_index)

    def frame_of(k, cam, prims):
        ps = scene(cam, prims)
        sc = orc.Scene.from_packed(ps)
        g, _ = ref.oracle_gbuffer(orc, ps, (0, 0, size, size))
        return sc.render(m["spp"], first_sample=m["spp"] * k + 1)[0], g, ref.keys(g, prims), sc.camera_frame()

    def truth_of(cam, prims):
        sc = orc.Scene.from_packed(scene(cam, prims))
        return ref.linear_rgb(sc.render(m["truth_spp"], first_sample=m["truth_first"])[0], m["truth_spp"])
    name = "orbit" if orbit else "fixed"
    got = clip_quality(frame_of, truth_of, orbit)
    for P in SWEEP:
        print(f"{name}: P = {P:3d}: temporal + filter / filter alone: whole image {got[P][0]:.3f}, moved primitives "
              f"{got[P][1]:.3f}, static pixels {got[P][2]:.3f}")
    for P in SWEEP:
        for value, measured in zip(got[P], MEASURED[name][P]):
            assert value <= measured + 0.10, (name, P, got[P], MEASURED[name][P])


# ------------------------------------------------------------------ 5. the light switch
def light_switch(orc):
    """SWITCH: a static camera, four frames under the light, then two under a sixteenth of it.  Returns per frame after the
    switch the MSE in display space against the dim scene's truth for (dropped, kept, kept and clipped)."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import PackedScene
    s = SWITCH
    W = Hh = s["size"]
    ps, dim = cref.with_dim_row(cornell(W, Hh))
    dark = PackedScene(ps.primitives, dim, ps.camera, ps.spectra, ps.cie, ps.patches, ps.spectrum_index)
    g, _ = ref.oracle_gbuffer(orc, ps, (0, 0, W, Hh))
    key = ref.keys(g, ps.primitives)
    bright_sc, dark_sc = orc.Scene.from_packed(ps), orc.Scene.from_packed(dark)
    frame = bright_sc.camera_frame()
    truth = ref.linear_rgb(dark_sc.render(s["truth_spp"], first_sample=s["truth_first"])[0], s["truth_spp"])
    arms = {"dropped": 0.0, "kept": 0.0, "clipped": DEFAULT_PCT / 100.0}
    prev = {a: None for a in arms}
    errors = []
    for k in range(s["before"] + s["after"]):
        sc = bright_sc if k < s["before"] else dark_sc
        acc = sc.render(s["spp"], first_sample=s["spp"] * k + 1)[0]
        if k == s["before"]:
            prev["dropped"] = None                              # today's crt_update_lights
        row = []
        for a, gamma in arms.items():
            out, c, hw, _ = cref.temporal(acc, s["spp"], g, key, frame, prev[a], W, Hh, gamma=gamma)
            prev[a] = tref.slot(c, hw, g, key, frame)
            row.append(ref.mse_display(out, truth))
        if k >= s["before"]:
            errors.append(tuple(row))
    return errors


def test_a_switched_light_is_followed_sooner_with_the_clip(orc):
    """The second table of DESIGN.md 6l.  The direction follows from the definition: the unclipped arm keeps at least 4/5
    of its weight on a history 16 times too bright, the clipped one is bounded by the dim frame's own box."""
    got = light_switch(orc)
    for k, (dropped, kept, clipped) in enumerate(got):
        print(f"frame {k + 1} after the switch: MSE against the dim scene: history dropped {dropped:.5f}, kept {kept:.5f}, "
              f"kept and clipped at P = {DEFAULT_PCT} {clipped:.5f}")
    for k, (_, kept, clipped) in enumerate(got):
        assert clipped < kept, (k, got)
