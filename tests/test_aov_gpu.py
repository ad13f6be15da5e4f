"""GPU tests of the feature planes (include/crt.h "Feature planes"; run with -m gpu on an MI355X):
crt_render_aovs is the restatement of tests/aov_ref.py bit for bit -- the oracle's camera rays, float32 sums in sample
order -- under every tree, a sample offset, a tile, the adaptive state and scene edits, and it leaves the renderer's
state alone."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref
import aov_ref as ref
from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

NODE = shutil.which("node")
EINVAL, ESTATE, ENOMEM = -1, -3, -4
_CACHE = {}


def cornell_truth(orc, w, h, n, offset=0):
    """(scene, planes, index) of the whole Cornell box at w x h: computed once, shared, never written."""
    from computeraytracer_amd import cornell
    key = (w, h, n, offset)
    if key not in _CACHE:
        ps = cornell(w, h)
        want, index = ref.oracle_aovs(orc, ps, (0, 0, w, h), n, offset)
        for a in list(want.values()) + [index]:
            a.setflags(write=False)
        _CACHE[key] = (ps, want, index)
    return _CACHE[key]


def raw(r, n, planes_ptr):
    return r._lib.crt_render_aovs(r._h, n, planes_ptr)


def state(r):
    """Accumulator, rgba8, sample and the counters that count what the paths did.  (`nodes` and `prims` count what the
    traversal kernels visited, which depends on the order rays shrink their t_max in and differs between two contexts
    that made the same calls: those two are compared on one context, before and after the call.)"""
    c = r.counters()
    return (r.read_accum().tobytes(), r.read_rgba8().tobytes(), r.sample, tuple((k, c[k]) for k in sorted(c) if k not in ("nodes", "prims")))


# ------------------------------------------------------------------ 1. against the oracle, every tree
def test_cornell_equals_the_oracle_under_every_tree(renderer, orc):
    n = 17                                                   # sample % 16 wraps
    ps, want, index = cornell_truth(orc, 32, 32, n)
    h = want["hits"]
    assert int(((h > 0) & (h < n)).sum()) >= 50, "too few fractional pixels for the test to mean anything"
    assert int((ref.distinct_primitives(index) >= 2).sum()) >= 100, "too few pixels that see two primitives"
    table = ref.albedo_table(ps.spectra, ps.cie)
    for mode in ("none", "bvh2", "lbvh", "ploc"):
        renderer.upload(ps).build_accel(mode)
        got = renderer.render_aovs(n)                        # at sample 0: an explicit n needs nothing traced
        assert set(got) == set(ref.PLANES)
        ref.assert_planes(got, want, mode)
        assert np.array_equal(bits(renderer.albedo_table()), bits(table)), mode
    from computeraytracer_amd import spectrum_rgb
    rows = np.asarray(ps.spectra, np.float32).reshape(-1, 301)
    assert all(np.array_equal(bits(spectrum_rgb(rows[i], ps.cie)), bits(table[i])) for i in range(len(rows)))
    assert (got["normal"][..., 3] == 0).all() and (got["albedo"][..., 3] == 0).all()
    assert not np.signbit(got["normal"][..., 3]).any() and not np.signbit(got["albedo"][..., 3]).any()


# ------------------------------------------------------------------ 2. sample offset
def test_sample_offset(renderer, orc):
    ps, want, _ = cornell_truth(orc, 48, 32, 5, offset=100)
    h = want["hits"]
    assert int(((h > 0) & (h < 5)).sum()) >= 10
    renderer.upload(ps).build_accel("bvh2").set_sample_offset(100)
    ref.assert_planes(renderer.render_aovs(5), want, "offset 100")
    # n_samples = 0 under the offset: the very rays the accumulator was averaged over
    renderer.frame(5)
    ref.assert_planes(renderer.render_aovs(0), want, "offset 100, n = 0")


# ------------------------------------------------------------------ 3. one sample is the G-buffer's ray
def test_one_sample_at_offset_7_is_the_gbuffer(renderer):
    from computeraytracer_amd import cornell
    renderer.upload(cornell(48, 32)).build_accel("bvh2").set_sample_offset(7)
    renderer.frame(1).sync()                                 # (crt_read_gbuffer wants a sample in the accumulator)
    g = renderer.read_gbuffer()
    got = renderer.render_aovs(1)
    hit = bits(g[..., 7]) != ref.MISS
    assert hit.mean() > 0.3
    assert np.array_equal(got["hits"], hit.astype(np.uint32))
    assert np.array_equal(bits(got["alpha"]), bits(hit.astype(np.float32)))
    assert np.array_equal(bits(got["depth"])[hit], bits(g[..., 0])[hit])
    assert (bits(got["depth"])[~hit] == bits(ref.INF)).all()
    # the normal is (+0 + n) / 1: the G-buffer's, but for a component of -0, which the sum from +0 turns into +0
    assert np.array_equal(bits(got["normal"][..., :3]), bits(np.float32(0) + g[..., 4:7]))
    assert np.array_equal(got["normal"][..., :3], g[..., 4:7])


# ------------------------------------------------------------------ 4. a tile is the crop of the frame
def test_tile_equals_the_crop(renderer, orc):
    ps, want, _ = cornell_truth(orc, 32, 32, 17)
    renderer.upload(ps).build_accel("bvh2").set_tile(5, 3, 18, 14)            # 13 x 11: partial blocks on both edges
    got = renderer.render_aovs(17)
    assert got["hits"].shape == (11, 13) and got["normal"].shape == (11, 13, 4)
    ref.assert_planes(got, {p: a[3:14, 5:18] for p, a in want.items()}, "tile")


# ------------------------------------------------------------------ 5. a large scene
def test_atrium_crop_equals_the_oracle(renderer, orc):
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(480, 270)
    x0, y0, w, h = rect = (200, 120, 16, 16)
    want, _ = ref.oracle_aovs(orc, ps, rect, 3, full_log=False)
    assert want["hits"].any()
    for mode in ("bvh2", "lbvh"):
        renderer.upload(ps).set_tile(x0, y0, x0 + w, y0 + h).build_accel(mode)
        ref.assert_planes(renderer.render_aovs(3), want, mode)


# ------------------------------------------------------------------ 6. n_samples = 0, and the state stays
def test_zero_means_what_the_accumulator_holds_and_nothing_changes(renderer):
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError
    ps = cornell(64, 48)
    renderer.upload(ps).build_accel("bvh2").enable_counters(True).reset_counters()
    try:
        with pytest.raises(CrtError) as e:
            renderer.render_aovs(0)
        assert e.value.code == ESTATE                        # sample 0: the accumulator holds nothing
        renderer.frame(3)                                    # no sync: the call is a sync point
        held = renderer.render_aovs(0)
        counted = renderer.counters()
        ref.assert_planes(held, renderer.render_aovs(3), "n = 0 after frame(3)")
        assert held["hits"].max() == 3
        assert renderer.counters() == counted                # every counter, nodes and prims included
        with Renderer(0) as other:                           # a context that never makes the call
            other.upload(ps).build_accel("bvh2").enable_counters(True).reset_counters()
            other.frame(3).sync()
            assert state(renderer) == state(other)
            renderer.frame(2).sync()
            other.frame(2).sync()
            assert renderer.sample == 5 and state(renderer) == state(other)
    finally:
        renderer.enable_counters(False)


# ------------------------------------------------------------------ 7. the adaptive state: every tile its own count
def test_adaptive_state_takes_each_tiles_count(renderer):
    from computeraytracer_amd import cornell
    renderer.upload(cornell(64, 64)).build_accel("bvh2")
    rule = dict(samples=8, min_samples=8, max_samples=40)
    try:
        renderer.trace_adaptive(threshold=0.0, **rule)
        counts, errors = renderer.read_adaptive()
        thr = float(np.float32(np.median(errors[np.isfinite(errors)])))
        for _ in range(4):
            if renderer.trace_adaptive(threshold=thr, **rule) == 0 or len(np.unique(renderer.read_adaptive()[0])) >= 2:
                break
        counts, errors = renderer.read_adaptive()
        distinct = [int(v) for v in np.unique(counts)]
        assert len(distinct) >= 2, f"every tile holds {distinct} samples: the rounds did not tell the tiles apart"
        before = (renderer.read_accum().tobytes(), renderer.read_rgba8().tobytes())
        got = renderer.render_aovs(0)
        npx = adaptive_ref.pixel_counts(counts, 64, 64)
        for n in distinct:
            explicit = renderer.render_aovs(n)               # allowed in the adaptive state
            m = npx == n
            for p in ref.PLANES:
                assert np.array_equal(bits(got[p])[m], bits(explicit[p])[m]), (n, p)
        after_counts, after_errors = renderer.read_adaptive()
        assert np.array_equal(after_counts, counts) and np.array_equal(bits(after_errors), bits(errors))
        assert (renderer.read_accum().tobytes(), renderer.read_rgba8().tobytes()) == before
        want_active = adaptive_ref.active(counts, errors, 8, 40, np.float32(thr))
        assert renderer.trace_adaptive(threshold=thr, **rule) == int(want_active.sum())        # the next round is the rule's
        assert np.array_equal(renderer.read_adaptive()[0], counts + 8 * want_active.astype(np.uint32))
    finally:
        renderer.reset()


# ------------------------------------------------------------------ 8. scene edits
def test_planes_follow_the_camera_and_moved_primitives(renderer, orc):
    from computeraytracer_amd import Renderer, cornell, scene as S
    ps = cornell(40, 32)
    renderer.upload(ps).build_accel("bvh2")
    first = renderer.render_aovs(4)
    cam = ps.camera.copy()
    cam[0] += 40.0                                           # the eye moves; the size does not
    renderer.set_camera(cam)
    moved_cam = S.PackedScene(ps.primitives, ps.lights, cam, ps.spectra, ps.cie)
    want, _ = ref.oracle_aovs(orc, moved_cam, (0, 0, 40, 32), 4)
    got = renderer.render_aovs(4)
    ref.assert_planes(got, want, "after set_camera")
    assert not np.array_equal(bits(got["depth"]), bits(first["depth"]))
    n = len(ps.primitives)
    shift = [1, 0, 0, 12.5, 0, 1, 0, 20.0, 0, 0, 1, -7.25]
    renderer.transform_primitives([(n - 2, 2, shift)]).refit_accel()
    records = renderer.read_primitives()
    assert records.tobytes() != np.ascontiguousarray(ps.primitives).tobytes()
    after = renderer.render_aovs(4)
    with Renderer(0) as fresh:                               # a fresh upload and build of the read-back records
        fresh.upload(S.PackedScene(records, ps.lights, cam, ps.spectra, ps.cie)).build_accel("bvh2")
        ref.assert_planes(after, fresh.render_aovs(4), "after transform_primitives + refit_accel")
    assert not np.array_equal(bits(after["depth"]), bits(got["depth"]))


# ------------------------------------------------------------------ 9. a camera at infinity
def test_non_finite_camera_takes_the_reference_loop(renderer):
    from computeraytracer_amd import cornell, scene as S
    c = cornell(48, 40)
    cam = c.camera.copy()
    cam[0] = np.inf
    ps = S.PackedScene(c.primitives, c.lights, cam, c.spectra, c.cie)
    brute = renderer.upload(ps).build_accel("none").render_aovs(3)
    assert (brute["hits"] == 3).all()                        # the reference loop ends on the last primitive, for every ray
    tree = renderer.upload(ps).build_accel("bvh2").render_aovs(3)
    ref.assert_planes(tree, brute, "bvh2 against none")


# ------------------------------------------------------------------ 10. refusals and allocation
def test_refusals(renderer):
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import AovPlanes, CrtError
    ps = cornell(32, 24)
    alpha = np.zeros((24, 32), np.float32)
    arg = AovPlanes(alpha=alpha.ctypes.data)
    with Renderer(0) as r:
        assert raw(r, 1, C.byref(arg)) == ESTATE             # no scene
        r.upload(ps)
        assert raw(r, 1, C.byref(arg)) == ESTATE             # no acceleration structure
        r.build_accel("bvh2")
        assert raw(r, 1, None) == EINVAL                     # out NULL
        assert raw(r, 1, C.byref(arg)) == 0
        r.update_primitives(0, ps.primitives[0:1])
        assert raw(r, 1, C.byref(arg)) == ESTATE             # a stale tree
        r.refit_accel()
        assert raw(r, 1, C.byref(arg)) == 0
        r.set_sample_offset(0xFFFFFFF0)
        assert raw(r, 16, C.byref(arg)) == EINVAL            # B + n = 2^32
        assert raw(r, 15, C.byref(arg)) == 0                 # 2^32 - 1 is a sample index
        r.set_sample_offset(0)
        r.set_row_bands(8, 2, 1)
        with pytest.raises(CrtError) as e:
            r.render_aovs(1)
        assert e.value.code == ESTATE                        # row bands


def test_a_failed_allocation_leaves_nothing_and_null_planes_are_skipped(renderer):
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError
    ps = cornell(32, 24)
    want = renderer.upload(ps).build_accel("bvh2").render_aovs(2)
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2").frame(2).sync()
        before = (r.read_accum().tobytes(), r.sample)
        try:
            # a plane whose pointer is NULL is not allocated: alpha alone needs two buffers, its own and the albedo table
            r.set_option("debug_fail_alloc", 3)
            only = r.render_aovs(2, planes=("alpha",))
            r.set_option("debug_fail_alloc", 0)
            assert list(only) == ["alpha"] and np.array_equal(bits(only["alpha"]), bits(want["alpha"]))
            # the other four, in the order hits, depth, normal, albedo: the k-th allocation of a call fails, the ones
            # before it stay -- hits; hits ok, depth; depth ok, normal; normal ok, albedo; albedo
            for k in (1, 2, 2, 2, 1):
                r.set_option("debug_fail_alloc", k)
                with pytest.raises(CrtError) as e:
                    r.render_aovs(2)
                r.set_option("debug_fail_alloc", 0)
                assert e.value.code == ENOMEM, k
                assert (r.read_accum().tobytes(), r.sample) == before
            ref.assert_planes(r.render_aovs(2), want, "after the failed calls")
            r.set_option("debug_fail_alloc", 1)              # nothing is left to allocate
            ref.assert_planes(r.render_aovs(2), want, "with every buffer there")
        finally:
            r.set_option("debug_fail_alloc", 0)
        ref.assert_planes(r.render_aovs(0), want, "n = 0")
    # a NULL plane is not stored either: the others do not depend on which are asked for
    some = renderer.render_aovs(2, planes=("depth", "albedo"))
    assert sorted(some) == ["albedo", "depth"]
    ref.assert_planes(some, want, "two planes")


# ------------------------------------------------------------------ 11. Node
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_planes_equal_python(tmp_path, renderer):
    from computeraytracer_amd import cornell
    pre = tmp_path / "aov"
    subprocess.run([NODE, os.path.join(ROOT, "host", "index.js"), "--width", "48", "--height", "40", "--spp", "3",
                    "--aov-out", str(pre)], capture_output=True, text=True, check=True)
    want = renderer.upload(cornell(48, 40)).build_accel("bvh2").render_aovs(3)
    for p in ref.PLANES:
        assert (tmp_path / f"aov_{p}.bin").read_bytes() == np.ascontiguousarray(want[p]).tobytes(), p
