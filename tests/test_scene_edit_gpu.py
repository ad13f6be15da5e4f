"""GPU tests of the scene edits (include/crt.h "Scene edits"; run with -m gpu on an MI355X): a moved camera,
edited primitives and lights and a refitted tree give the oracle's image of the edited buffers bit for bit, and the
same image as a fresh upload + build; stale trees, bad edits, fallbacks, denoise, pipelining, multi-GPU and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref as ref
from conftest import ROOT, bits
from denoise_ref import oracle_gbuffer

pytestmark = pytest.mark.gpu
MAXU = 0xFFFFFFFF
DEFAULTS = dict(pipeline=1, quantize=1, wf_width=4, wf_trace_form=2)
FORMS = {"form2": {}, "form1": dict(wf_trace_form=1), "pipeline0": dict(pipeline=0), "width8": dict(wf_width=8),
         "quantize0": dict(quantize=0)}


def assert_same_image(acc, rgba, acc_o, rgba_o):
    bad = (bits(acc)[..., :3] != bits(acc_o)[..., :3]).any(-1)
    assert not bad.any(), f"{int(bad.sum())} accumulator pixels differ, first at {np.argwhere(bad)[0][::-1]}"
    assert np.array_equal(rgba, rgba_o), f"{int((rgba != rgba_o).sum())} rgba8 bytes differ"


def with_camera(ps, cam):
    from computeraytracer_amd.scene import PackedScene
    return PackedScene(ps.primitives, ps.lights, np.asarray(cam, np.float32).copy(), ps.spectra, ps.cie)


def with_prims(ps, prims):
    from computeraytracer_amd.scene import PackedScene, lights_of
    return PackedScene(prims, lights_of(prims), ps.camera, ps.spectra, ps.cie)


def camera_set(ps, n=4):
    """Orbit positions, one farther away (hit_pad grows: inline refit) and one nearer."""
    from computeraytracer_amd.scene import orbit_cameras
    cams = list(orbit_cameras(ps.camera, n)[1:])
    cam = ps.camera.copy()
    look = cam[4:7].astype(np.float64)
    for f in (1.7, 0.6):
        c = cam.copy()
        c[0:3] = (look + f * (cam[0:3].astype(np.float64) - look)).astype(np.float32)
        cams.append(c)
    return cams


_ORACLE = {}


def oracle(orc, ps, spp, rect=None):
    key = (ps.primitives.tobytes(), ps.lights.tobytes(), ps.camera.tobytes(), spp, rect)
    if key not in _ORACLE:
        acc, rgba, _ = orc.Scene.from_packed(ps).render(spp, rect=rect)
        _ORACLE[key] = (acc, rgba) if rect is None else (acc[rect[1]:rect[3], rect[0]:rect[2]], rgba[rect[1]:rect[3], rect[0]:rect[2]])
    return _ORACLE[key]


def options(r, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        r.set_option(k, v)


def frame3(r):
    r.frame(2).frame(1).sync()
    return r.read_accum(), r.read_rgba8()


# ------------------------------------------------------------------ 1. camera
@pytest.mark.parametrize("mode", ["bvh2", "lbvh", "none"])
@pytest.mark.parametrize("form", list(FORMS))
def test_set_camera_matches_oracle(renderer, orc, form, mode):
    from computeraytracer_amd import cornell
    ps = cornell(96, 96)
    try:
        options(renderer, **FORMS[form])
        renderer.upload(ps).build_accel(mode)
        assert_same_image(*frame3(renderer), *oracle(orc, ps, 3))
        pad0 = renderer.debug_hit_pad
        for cam in camera_set(ps):
            renderer.set_camera(cam)
            assert renderer.sample == 0
            ed = with_camera(ps, cam)
            assert_same_image(*frame3(renderer), *oracle(orc, ed, 3))
            assert renderer.sample == 3
            assert np.float32(renderer.debug_hit_pad) == np.float32(orc.Scene.from_packed(ed).hit_pad())
        assert renderer.debug_hit_pad < pad0            # (the nearer camera was last: the pad shrank back)
    finally:
        options(renderer)


# ------------------------------------------------------------------ 2. bad camera
def test_bad_camera_is_refused_and_changes_nothing(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd._lib import CrtError
    ps = cornell(64, 48)
    renderer.upload(ps).build_accel("bvh2").frame(1).sync()
    for k in (11, 12):
        cam = camera_set(ps)[0].copy()
        cam[k] += 1
        with pytest.raises(CrtError, match="must stay 64 x 48"):
            renderer.set_camera(cam)
    assert renderer.sample == 1
    renderer.reset()
    assert_same_image(*frame3(renderer), *oracle(orc, ps, 3))


# ------------------------------------------------------------------ 3. geometry edit
def moved_cornell(ps):
    """Both spheres and the light patch moved (the light stays inside the box, below the ceiling)."""
    from computeraytracer_amd.scene import transform_records
    prims = ps.primitives.copy()
    sph = np.flatnonzero(prims["category"] == 1)
    lit = np.flatnonzero(prims["data4"][:, 2] == 1)
    assert len(sph) == 2 and len(lit) >= 1
    c, s = np.cos(0.3), np.sin(0.3)
    prims[sph[:1]] = transform_records(prims[sph[:1]], np.eye(3), [40.0, 0.0, -25.0])
    prims[sph[1:]] = transform_records(prims[sph[1:]], [[c, 0, s], [0, 1, 0], [-s, 0, c]], [30.0, 20.0, 10.0], 0.8)
    prims[lit] = transform_records(prims[lit], np.eye(3), [15.0, -1.0, 10.0])
    return prims, np.concatenate([sph, lit])


@pytest.mark.parametrize("mode", ["bvh2", "lbvh"])
def test_geometry_edit_and_refit(renderer, orc, mode):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import lights_of
    ps = cornell(96, 96)
    prims, moved = moved_cornell(ps)
    ed = with_prims(ps, prims)
    renderer.upload(ps).build_accel(mode).frame(2).sync()
    for i in moved:                                          # one call per record, then one refit
        renderer.update_primitives(int(i), prims[i:i + 1])
    renderer.update_lights(0, lights_of(prims))
    assert renderer.refit_accel() is False
    acc, rgba = frame3(renderer)
    assert_same_image(acc, rgba, *oracle(orc, ed, 3))
    for m in ("bvh2", "lbvh"):                               # = a fresh upload + build of the edited buffers
        renderer.upload(ed).build_accel(m)
        assert_same_image(acc, rgba, *frame3(renderer))


# ------------------------------------------------------------------ 4. stale guard
def test_stale_tree_is_refused_until_refit(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd._lib import CrtError
    ps = cornell(64, 64)
    prims, moved = moved_cornell(ps)
    renderer.upload(ps).build_accel("bvh2").frame(1).sync()
    renderer.update_primitives(0, prims)
    for call in (lambda: renderer.frame(1), lambda: renderer.denoise(2), lambda: renderer.read_gbuffer(),
                 lambda: renderer.debug_intersect(np.zeros((1, 3)), np.ones((1, 3)))):
        with pytest.raises(CrtError, match="crt_refit_accel"):
            call()
    renderer.update_primitives(0, prims)                     # several updates before one refit
    renderer.refit_accel()
    renderer.update_lights(0, ref_lights(prims))
    assert_same_image(*frame3(renderer), *oracle(orc, with_prims(ps, prims), 3))
    renderer.upload(ps).build_accel("none").frame(1).sync()  # no tree: nothing goes stale
    renderer.update_primitives(0, prims).update_lights(0, ref_lights(prims))
    assert_same_image(*frame3(renderer), *oracle(orc, with_prims(ps, prims), 3))
    renderer.update_primitives(0, ps.primitives)             # a full build clears the stale state too
    renderer.build_accel("bvh2").update_primitives(0, prims)
    renderer.build_accel("lbvh").update_lights(0, ref_lights(prims))
    assert_same_image(*frame3(renderer), *oracle(orc, with_prims(ps, prims), 3))


def ref_lights(prims):
    from computeraytracer_amd.scene import lights_of
    return lights_of(prims)


# ------------------------------------------------------------------ 5. invalid edits
def test_invalid_edits_change_nothing(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd._lib import CrtError
    ps = cornell(64, 64)
    n = len(ps.primitives)
    sph = int(np.flatnonzero(ps.primitives["category"] == 1)[0])
    renderer.upload(ps).build_accel("lbvh").frame(1).sync()
    bad = []
    r = ps.primitives[sph:sph + 1].copy(); r["category"] = 0; bad.append((sph, r, "category"))
    r = ps.primitives[sph:sph + 1].copy(); r["data4"][:, 2] = (r["data4"][:, 2] + 1) % 3; bad.append((sph, r, "material"))
    r = ps.primitives[sph:sph + 1].copy(); bad.append((sph + 1, r, "index"))
    r = ps.primitives[sph:sph + 1].copy(); r["data4"][:, 1] = len(ps.spectra); bad.append((sph, r, "spectrum"))
    r = ps.primitives[n - 2:].copy(); bad.append((n - 1, r, "outside"))
    for first, rec, what in bad:
        with pytest.raises(CrtError, match=what):
            renderer.update_primitives(first, rec)
    lt = ps.lights.copy(); lt["data4"][:, 0] = len(ps.spectra)
    with pytest.raises(CrtError, match="emission"):
        renderer.update_lights(0, lt)
    with pytest.raises(CrtError, match="outside"):
        renderer.update_lights(len(ps.lights), ps.lights[:1])
    assert renderer.sample == 1                              # nothing reset, nothing stale
    renderer.reset()
    assert_same_image(*frame3(renderer), *oracle(orc, ps, 3))


# ------------------------------------------------------------------ 6. S2 at 1080p, SAH and LBVH
def rigid(rng, scale=1.0):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(-0.4, 0.4)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K, rng.normal(0, 8 * scale, 3)


def rays_at(rng, prims, n, pad):
    """Rays aimed at the vertices and edge points of prims (+- pad), random and axis-parallel ones."""
    v0 = prims["data1"].astype(np.float64)
    pts = np.concatenate([v0, v0 + prims["data2"], v0 + prims["data3"], v0 + 0.5 * prims["data2"], v0 + 0.5 * prims["data3"],
                          v0 + 0.5 * (prims["data2"] + prims["data3"])])
    tgt = pts[rng.integers(0, len(pts), n)] + rng.uniform(-pad, pad, (n, 3)) * rng.integers(0, 2, (n, 1))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = n // 8
    d[:k] = 0
    d[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0], k)     # axis-parallel
    o = tgt - d * rng.uniform(1, 300, (n, 1))
    return o.astype(np.float32), d.astype(np.float32)


def check_rays(r, brute, orc_scene, o, d, spot=40):
    got = r.debug_intersect(o, d)
    want = brute.debug_intersect(o, d)
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(1).sum())} of {len(o)} rays differ"
    idx = np.linspace(0, len(o) - 1, spot).astype(int)
    for i in idx:                                            # the brute-force loop is the oracle's (spot check)
        of, ou = orc_scene.intersect(o[i], d[i])
        assert int(want[i, 7:8].view(np.uint32)[0]) == (int(ou[1]) if ou[0] else MAXU)
        if ou[0]:
            assert np.array_equal(bits(want[i, :7]), bits(of))
    return (want[:, 7].view(np.uint32) != MAXU).mean()


@pytest.mark.parametrize("mode", ["bvh2", "lbvh"])
def test_s2_rigid_move_of_a_tenth(renderer, orc, mode):
    from computeraytracer_amd import Renderer
    from computeraytracer_amd.scene import transform_records
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(1920, 1080)
    rng = np.random.default_rng(11)
    n = len(ps.primitives)
    tri = np.flatnonzero(ps.primitives["category"] == 2)
    first = int(tri[len(tri) // 3])
    cnt = n // 10
    prims = ps.primitives.copy()
    old = prims[first:first + cnt].copy()
    R, t = rigid(rng, 3.0)
    prims[first:first + cnt] = transform_records(old, R, t)
    ed = with_prims(ps, prims)
    renderer.upload(ps).build_accel(mode).frame(1)
    renderer.update_primitives(first, prims[first:first + cnt])
    assert renderer.refit_accel() is False
    pad = renderer.debug_hit_pad
    assert np.float32(pad) == np.float32(orc.Scene.from_packed(ed).hit_pad())
    o1, d1 = rays_at(rng, prims[first:first + cnt], 200_000, 4 * pad)       # at the moved geometry
    o2, d2 = rays_at(rng, old, 150_000, 4 * pad)                            # at where it was
    o3 = rng.uniform(-200, 800, (60_000, 3)).astype(np.float32)
    d3 = rng.normal(size=(60_000, 3)).astype(np.float32)
    o, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    with Renderer(0) as brute:
        brute.upload(ed).build_accel("none")
        assert 0.1 < check_rays(renderer, brute, orc.Scene.from_packed(ed), o, d)
    renderer.frame(1).sync()
    acc, rgba = renderer.read_accum(), renderer.read_rgba8()
    for rect in ((900, 500, 964, 564), (300, 700, 364, 764)):
        x0, y0, x1, y1 = rect
        assert_same_image(acc[y0:y1, x0:x1], rgba[y0:y1, x0:x1], *oracle(orc, ed, 1, rect))
    renderer.upload(ed).build_accel("lbvh").frame(1).sync()
    assert_same_image(acc, rgba, renderer.read_accum(), renderer.read_rgba8())


# ------------------------------------------------------------------ 7. repeated edits
def mixed_scene(w, h):
    """Patches + a glass and a diffuse sphere + mesh triangles + a triangle soup (~20 k primitives)."""
    from computeraytracer_amd import scene as S
    from computeraytracer_amd.scenes_synth import mesh10k
    base = mesh10k(w, h)
    idx = base.spectrum_index
    rng = np.random.default_rng(3)
    nb = len(base.primitives)
    sph = S.make_primitives([1, 1], [[120, 90, 150], [430, 110, 180]], [[60] * 3, [75] * 3], [[0] * 3] * 2,
                            [idx["dark"]] * 2, [idx["red"], idx["white"]], [0, 2], first_index=nb)
    m = 9000
    v0 = rng.uniform([20, 20, -200], [530, 530, 500], (m, 3))
    soup = S.make_primitives(np.full(m, 2), v0, rng.normal(0, 6, (m, 3)), rng.normal(0, 6, (m, 3)), [idx["dark"]] * m,
                             [idx["white"]] * m, [0] * m, first_index=nb + 2)
    prims = np.zeros(nb + 2 + m, S.PRIM_DTYPE)
    prims[:nb], prims[nb:nb + 2], prims[nb + 2:] = base.primitives, sph, soup
    return S.PackedScene(prims, S.lights_of(prims), base.camera, base.spectra, base.cie)


@pytest.mark.parametrize("mode", ["bvh2", "lbvh"])
def test_repeated_random_rigid_moves(renderer, orc, mode):
    from computeraytracer_amd import Renderer
    from computeraytracer_amd.scene import transform_records
    ps = mixed_scene(96, 54)
    prims = ps.primitives.copy()
    n = len(prims)
    rng = np.random.default_rng(7)
    renderer.upload(ps).build_accel(mode)
    with Renderer(0) as brute:
        brute.upload(ps).build_accel("none")
        for step in range(16):
            first = int(rng.integers(0, n - 1))
            cnt = int(rng.integers(1, min(3000, n - first) + 1))
            R, t = rigid(rng, 2.0)
            prims[first:first + cnt] = transform_records(prims[first:first + cnt], R, t, float(rng.uniform(0.8, 1.25)))
            renderer.update_primitives(first, prims[first:first + cnt])
            brute.update_primitives(first, prims[first:first + cnt])
            assert renderer.refit_accel() is False, step
            o, d = rays_at(rng, prims[first:first + cnt], 40_000, 4 * renderer.debug_hit_pad)
            sc = orc.Scene(prims, ps.lights, ps.spectra, ps.cie, ps.camera)
            check_rays(renderer, brute, sc, o, d, spot=8)
    renderer.update_lights(0, ref_lights(prims))
    assert_same_image(*frame3(renderer), *oracle(orc, with_prims(ps, prims), 3))


# ------------------------------------------------------------------ 8. fallbacks
def test_refit_falls_back_to_a_rebuild(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import transform_records
    ps = cornell(64, 64)
    sph = int(np.flatnonzero(ps.primitives["category"] == 1)[0])
    for mode in ("bvh2", "lbvh"):
        renderer.upload(ps).build_accel(mode)
        assert renderer.accel_stats()["bytes_per_box"] == 16            # a quantised tree
        # the scene pushed far from the origin (camera too): its 16-bit grid would lose the slack (quantize_bvh4's rule)
        T = np.float32([2.0e5, 0.0, 0.0])
        far = transform_records(ps.primitives, np.eye(3), T)
        cam = ps.camera.copy()
        cam[0:3] += T
        cam[4:7] += T
        renderer.set_camera(cam)                                         # (a larger pad: refitted inline, still quantisable)
        assert renderer.accel_stats()["bytes_per_box"] == 16
        renderer.update_primitives(0, far).update_lights(0, ref_lights(far))
        assert renderer.refit_accel() is True
        assert renderer.accel_stats()["bytes_per_box"] == 32             # rebuilt the way a fresh build does it
        assert_same_image(*frame3(renderer), *oracle(orc, with_prims(with_camera(ps, cam), far), 3))
        renderer.upload(ps).build_accel(mode)
        small = ps.primitives.copy()
        small[sph:sph + 1] = transform_records(small[sph:sph + 1], np.eye(3), [3.0, 0.0, 2.0])
        renderer.update_primitives(sph, small[sph:sph + 1])
        assert renderer.refit_accel() is False
        assert_same_image(*frame3(renderer), *oracle(orc, with_prims(ps, small), 3))
    try:
        options(renderer, wf_width=8)
        renderer.upload(ps).build_accel("bvh2")
        assert renderer.accel_stats()["width"] == 8
        renderer.update_primitives(sph, small[sph:sph + 1])
        assert renderer.refit_accel() is True
        assert renderer.accel_stats()["width"] == 8
        assert_same_image(*frame3(renderer), *oracle(orc, with_prims(ps, small), 3))
    finally:
        options(renderer)


# ------------------------------------------------------------------ 9. denoise
def test_denoise_after_edits(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(64, 64)
    renderer.upload(ps).build_accel("bvh2").frame(4).sync()
    renderer.read_gbuffer()
    cam = camera_set(ps)[0]
    prims, _ = moved_cornell(ps)
    for step in ("camera", "edit"):
        if step == "camera":
            renderer.set_camera(cam)
            ed = with_camera(ps, cam)
        else:
            renderer.update_primitives(0, prims).refit_accel()
            renderer.update_lights(0, ref_lights(prims))
            ed = with_prims(with_camera(ps, cam), prims)
        renderer.frame(4).sync()
        g = renderer.read_gbuffer()
        want, hit = oracle_gbuffer(orc, ed, (0, 0, 64, 64))
        assert np.array_equal(bits(g[..., 7]), bits(want[..., 7]))
        assert np.array_equal(bits(g[hit][:, :7]), bits(want[hit][:, :7]))
        rgba, rgb = renderer.denoise(3, rgb=True)
        rgb_o, rgba_o = orc.Scene.from_packed(ed).denoise(renderer.read_accum(), 4, g, 3)
        assert np.array_equal(bits(rgb), bits(rgb_o)) and np.array_equal(rgba, rgba_o)
        assert (ref.keys(g, ed.primitives) != ref.MISS).any()


# ------------------------------------------------------------------ 10. pipelining
def test_set_camera_with_calls_in_flight(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd._lib import CrtError
    ps = cornell(128, 96)
    cam = camera_set(ps)[1]
    try:
        renderer.set_option("frame_ring", 8)
        renderer.upload(ps).build_accel("bvh2")
        for _ in range(6):
            renderer.frame(1)                                 # in flight (merged / pipelined batches)
        renderer.set_camera(cam)
        assert renderer.sample == 0
        with pytest.raises(CrtError):
            renderer.read_sample_rgba8(3)                     # a frame from before the edit is gone
        renderer.frame(1).frame(1).frame(1)
        assert np.array_equal(renderer.read_sample_rgba8(2), oracle(orc, with_camera(ps, cam), 2)[1])
        assert_same_image(renderer.read_accum(), renderer.read_rgba8(), *oracle(orc, with_camera(ps, cam), 3))
    finally:
        renderer.set_option("frame_ring", 0)


# ------------------------------------------------------------------ 11. multi-GPU
def test_partitioned_ranks_set_camera(orc):
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(72, 61)
    cam = camera_set(ps)[2]
    cid = Renderer.comm_unique_id(local=True)
    rs = [Renderer(0) for _ in range(2)]
    try:
        for k, r in enumerate(rs):
            r.comm_init(cid, k, 2).upload(ps).comm_partition(8).build_accel("bvh2")
        for r in rs:
            r.frame(2)
        for r in rs:
            r.set_camera(cam)
        for r in rs:
            r.frame(3).sync().gather(rgba8=True, accum=True)
        for r in rs:
            assert_same_image(r.read_frame_accum(), r.read_frame_rgba8(), *oracle(orc, with_camera(ps, cam), 3))
    finally:
        for r in rs:
            r.close()


# ------------------------------------------------------------------ 12. CLI
def test_cli_orbit(orc, tmp_path):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    subprocess.run([sys.executable, "-m", "computeraytracer_amd", "--width", "32", "--height", "32", "--spp", "2",
                    "--orbit", "2", "--out", str(tmp_path / "o.ppm")], cwd=ROOT, check=True, capture_output=True)
    ps = cornell(32, 32)
    for k, cam in enumerate(orbit_cameras(ps.camera, 2)):
        ppm = (tmp_path / f"o_{k:03d}.ppm").read_bytes()
        assert ppm.startswith(b"P6\n32 32\n255\n")
        img = np.frombuffer(ppm[13:], np.uint8).reshape(32, 32, 3)
        assert np.array_equal(img, oracle(orc, with_camera(ps, cam), 2)[1][..., :3])
