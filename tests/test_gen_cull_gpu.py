"""GPU tests of the generate kernel's miss cull (run with -m gpu on an MI355X): k_wf_gen runs the traversal
kernel's root step on every camera ray and finishes a work chunk (the 64 pixels of one 8x8 tile of one sample) itself when
all of its rays miss the root's four child boxes -- no slot, no ray record, no shade step.  Option "wf_cull_miss" switches
it; every case renders with the cull on and off in the same process and asks for the same bits in the accumulator and the
rgba8 frame, and where it counts, for the same counters; the oracle is the third party on small frames and crops."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu
DEFAULTS = dict(pipeline=1, quantize=1, wf_width=4, wf_trace_form=2, wf_defer=1, wf_cohort=16, wf_pool=0, wf_cull_miss=1)
COUNTED = ("rays", "paths", "bounces", "shadow", "hits", "walked")
MISS = 0xFFFFFFFF


def options(r, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        r.set_option(k, v)


def same_image(a, b, what):
    (acc, rgba), (acc_o, rgba_o) = a[:2], b[:2]
    bad = (bits(acc)[..., :3] != bits(acc_o)[..., :3]).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} accumulator pixels differ, first at {np.argwhere(bad)[0][::-1]}"
    assert np.array_equal(rgba, rgba_o), f"{what}: {int((rgba != rgba_o).sum())} rgba8 bytes differ"


def on_and_off(r, prepare, run, counting=False, **opts):
    """prepare(r) and run(r) with the cull on and off: [(accum, rgba8, culled, counters)] for on, off."""
    out = []
    try:
        for cull in (1, 0):
            options(r, **opts, wf_cull_miss=cull)
            prepare(r)
            r.enable_counters(counting).reset_counters()
            run(r)
            r.sync()
            out.append((r.read_accum(), r.read_rgba8(), r.gen_culled(), r.counters() if counting else None))
    finally:
        r.enable_counters(False)
        options(r)
    return out


def scene_of(name, w, h):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scenes_synth import atrium250k, mesh10k
    return dict(cornell=cornell, mesh10k=mesh10k, atrium250k=atrium250k)[name](w, h)


def with_camera(ps, cam):
    from computeraytracer_amd.scene import PackedScene
    return PackedScene(ps.primitives, ps.lights, np.asarray(cam, np.float32), ps.spectra, ps.cie, ps.patches, ps.spectrum_index)


def looking_away(ps):
    cam = ps.camera.copy()
    cam[4:7] = 2.0 * cam[0:3] - cam[4:7]                         # look-at mirrored at the eye: the box is behind the camera
    return with_camera(ps, cam)


def first_ray_misses(sc, x0, y0, x1, y1, samples):
    """(pixel, sample) pairs of the rectangle whose camera ray hits nothing, by the oracle's transcripts."""
    n = 0
    for s in range(1, samples + 1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                n += sc.trace_pixel(x, y, s).hits[0] == MISS
    return n


# ------------------------------------------------------------------ 1. on = off = oracle, standard camera
# (scene, frame, samples, crop for the oracle or None = the whole frame): every frame is ragged in both directions or one
SHAPES = [("cornell", 100, 76, 8, None), ("mesh10k", 192, 108, 8, (0, 40, 72, 56)), ("atrium250k", 480, 270, 8, (104, 120, 120, 128))]


@pytest.mark.parametrize("mode", ["bvh2", "lbvh"])
@pytest.mark.parametrize("form", [2, 1])
@pytest.mark.parametrize("name,w,h,spp,crop", SHAPES, ids=[s[0] for s in SHAPES])
def test_on_equals_off_equals_oracle(renderer, orc, name, w, h, spp, crop, form, mode):
    ps = scene_of(name, w, h)
    x0, y0, x1, y1 = crop or (0, 0, w, h)
    with_oracle = form == 2 and mode == "bvh2"
    got = {}
    try:
        options(renderer, wf_trace_form=form)
        renderer.upload(ps).build_accel(mode)                    # one build: the option acts at the next trace call
        for counting in (True, False):                           # (the counting kernels are instantiations of their own)
            for cull in (1, 0):
                renderer.set_option("wf_cull_miss", cull).enable_counters(counting).reset().reset_counters()
                renderer.frame(spp).sync()
                got[counting, cull] = (renderer.read_accum(), renderer.read_rgba8(), renderer.gen_culled(), renderer.counters() if counting else None)
        if with_oracle:                                          # the crop alone, two samples per pixel
            renderer.set_tile(x0, y0, x1, y1)
            for cull in (1, 0):
                renderer.set_option("wf_cull_miss", cull).reset().reset_counters()
                renderer.frame(2).sync()
                got["crop", cull] = (renderer.read_accum(), renderer.read_rgba8(), renderer.gen_culled())
    finally:
        renderer.enable_counters(False)
        options(renderer)
    on, off = got[True, 1], got[True, 0]
    print(f"{name} {w}x{h} form {form} {mode}: culled {on[2]} of {w * h * spp} pixel-samples")
    same_image(on, off, "on / off")
    assert {k: on[3][k] for k in COUNTED} == {k: off[3][k] for k in COUNTED}
    assert on[3]["paths"] == w * h * spp                         # (node steps depend on the order in which lanes shrink t_max: not compared)
    assert off[2] == 0 and on[2] > 0
    same_image(got[False, 1], got[False, 0], "on / off, not counting")
    same_image(got[False, 1], on, "counting / not counting")
    assert got[False, 1][2] == on[2] and got[False, 0][2] == 0
    if with_oracle:
        sc = orc.Scene.from_packed(ps)
        acc_o, rgba_o, _ = sc.render(spp, rect=(x0, y0, x1, y1))
        same_image((on[0][y0:y1, x0:x1], on[1][y0:y1, x0:x1]), (acc_o[y0:y1, x0:x1], rgba_o[y0:y1, x0:x1]), "on / oracle")
        same_image(got["crop", 1], got["crop", 0], "crop on / off")
        # nothing is culled whose first ray the oracle sees hit something
        misses = first_ray_misses(sc, x0, y0, x1, y1, 2)
        print(f"  crop {x0},{y0}..{x1},{y1}: culled {got['crop', 1][2]}, first-ray misses {misses} of {(x1 - x0) * (y1 - y0) * 2}")
        assert got["crop", 1][2] <= misses and got["crop", 0][2] == 0


# ------------------------------------------------------------------ 2. a camera that sees nothing
@pytest.mark.parametrize("w,h", [(64, 48), (100, 76)])
def test_a_frame_that_is_culled_whole(renderer, orc, w, h):
    ps = scene_of("cornell", w, h)
    away, n = looking_away(ps), 5
    acc_a, rgba_a, _ = orc.Scene.from_packed(away).render(n)
    acc_o, rgba_o, _ = orc.Scene.from_packed(ps).render(3)
    first = []

    def run(r):
        r.frame(n).sync()                                        # no path ever enters the pool: the queues drain in gen launches alone
        first.append((r.read_accum(), r.read_rgba8(), r.gen_culled(), r.counters()))
        r.sync()
        r.set_camera(ps.camera).frame(3)                         # the pool was never fed, then is

    on, off = on_and_off(renderer, lambda r: r.upload(away).build_accel("bvh2"), run, counting=True)
    same_image(on, off, "on / off")
    same_image(on, (acc_o, rgba_o), "the second render / oracle")
    for k, what in enumerate(("on", "off")):
        same_image(first[k], (acc_a, rgba_a), f"looking away, {what} / oracle")
        assert first[k][3]["paths"] == w * h * n
    assert first[0][2] == w * h * n and first[1][2] == 0         # culled == paths
    assert {k: first[0][3][k] for k in COUNTED + ("nodes",)} == {k: first[1][3][k] for k in COUNTED + ("nodes",)}
    assert off[3]["paths"] == on[3]["paths"] == w * h * (n + 3)


def test_a_frame_that_is_culled_whole_with_several_batches_open(renderer, orc):
    """Every call is a batch of its own (wf_cohort = 1) and none is synced: the flush finds several batches open whose
    queues drain in gen launches alone, so the older ones retire through the pipes' statuses while the pipes list no rays
    (driver invariant I10: a pipe counts as drained only on its own word that every queue is dry)."""
    w, h = 100, 76
    away, calls = looking_away(scene_of("cornell", w, h)), (1, 1, 2, 1, 1, 3)
    acc_a, rgba_a, _ = orc.Scene.from_packed(away).render(sum(calls))

    def run(r):
        for n in calls:
            r.frame(n)

    on, off = on_and_off(renderer, lambda r: r.upload(away).build_accel("bvh2"), run, counting=True, wf_cohort=1)
    same_image(on, off, "on / off")
    same_image(on, (acc_a, rgba_a), "on / oracle")
    assert on[2] == w * h * sum(calls) and off[2] == 0
    assert on[3]["paths"] == off[3]["paths"] == w * h * sum(calls)
    assert {k: on[3][k] for k in COUNTED + ("nodes",)} == {k: off[3][k] for k in COUNTED + ("nodes",)}


# ------------------------------------------------------------------ 3. a camera inside the box
def test_inside_the_box_nothing_is_culled(renderer):
    ps = scene_of("cornell", 100, 76)
    cam = ps.camera.copy()
    cam[0:3], cam[4:7] = (278.0, 273.0, 100.0), (278.0, 273.0, 500.0)
    ps = with_camera(ps, cam)
    on, off = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2"), lambda r: r.frame(4))
    same_image(on, off, "on / off")
    assert on[2] == 0 and off[2] == 0


# ------------------------------------------------------------------ 4. the silhouette through tile interiors and a corner
def test_silhouette_through_tiles(renderer, orc):
    ps = scene_of("cornell", 100, 76)
    cam = ps.camera.copy()
    cam[4:7] = (cam[4] + 150.0, cam[5] + 120.0, cam[6])          # the box leaves the frame's centre: its edges cross the frame
    ps = with_camera(ps, cam)
    on, off = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2"), lambda r: r.frame(4))
    same_image(on, off, "on / off")
    acc_o, rgba_o, _ = orc.Scene.from_packed(ps).render(4)
    same_image(on, (acc_o, rgba_o), "on / oracle")
    empty = (bits(acc_o)[..., :3] == 0).all(-1)
    misses = first_ray_misses(orc.Scene.from_packed(ps), 0, 0, 100, 76, 4)
    print(f"silhouette: {int(empty.sum())} of {empty.size} pixels empty, corner pixels empty: {empty[0, 0]} {empty[0, -1]} {empty[-1, 0]} {empty[-1, -1]}, culled {on[2]}, first-ray misses {misses}")
    assert 0 < on[2] <= misses                                   # by whole tiles: fewer than the rays that miss, more than none
    corners = [empty[0, 0], empty[0, -1], empty[-1, 0], empty[-1, -1]]
    assert any(corners) and not all(corners)
    tiles = empty[:72, :96].reshape(9, 8, 12, 8).sum((1, 3))
    assert ((tiles > 0) & (tiles < 64)).sum() >= 4               # the edge crosses tile interiors


# ------------------------------------------------------------------ 5. queues that run dry inside a refill round
def test_twenty_one_sample_batches(renderer):
    ps = scene_of("cornell", 96, 64)                             # 1.5 chunks per shard and batch: steals and shortfalls

    def run(r):
        for _ in range(20):
            r.frame(1)

    on, off = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2"), run, wf_cohort=1)
    same_image(on, off, "on / off")
    assert on[2] > 0


def test_mixed_sizes_without_sync(renderer):
    ps = scene_of("atrium250k", 480, 270)

    def run(r):
        for n in (8, 1, 4, 1, 1, 16, 2):
            r.frame(n)

    on, off = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2"), run)
    same_image(on, off, "on / off")
    assert on[2] > 0


def test_small_pool(renderer):
    ps = scene_of("mesh10k", 192, 108)                           # 20 736 paths per sample through 4 096 slots: many iterations, tail mode
    on, off = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2"), lambda r: r.frame(6).frame(1), wf_pool=4096)
    same_image(on, off, "on / off")
    full = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2"), lambda r: r.frame(6).frame(1))[0]
    same_image(on, full, "small pool / automatic pool")
    assert on[2] > 0


# ------------------------------------------------------------------ 6. the frame ring and reads that do not flush
def test_frame_ring(renderer):
    ps = scene_of("cornell", 100, 76)
    frames = {}
    try:
        for cull in (1, 0):
            options(renderer, wf_cull_miss=cull, wf_cohort=1)
            renderer.upload(ps).build_accel("bvh2").set_option("frame_ring", 8)
            got = []
            for s in range(1, 7):
                renderer.frame(1)
                if s >= 2:
                    got.append(renderer.read_sample_rgba8(s - 1))    # the frame before the one in flight
            got.append(renderer.read_sample_rgba8(6))
            renderer.sync()
            frames[cull] = got + [renderer.read_rgba8()]
    finally:
        renderer.set_option("frame_ring", 0)
        options(renderer)
    assert len(frames[1]) == 7
    for k, (a, b) in enumerate(zip(frames[1], frames[0])):
        assert np.array_equal(a, b), f"frame {k + 1} of the ring differs"


# ------------------------------------------------------------------ 7. row bands
@pytest.mark.parametrize("rank", [0, 1])
def test_row_bands(renderer, rank):
    ps = scene_of("mesh10k", 192, 108)
    on, off = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2").set_row_bands(8, 2, rank), lambda r: r.frame(4))
    same_image(on, off, f"rank {rank}: on / off")
    assert on[2] > 0
    from computeraytracer_amd.partition import band_rows
    rows = band_rows(108, 2, rank, 8)
    whole = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2"), lambda r: r.frame(4))[0]
    assert np.array_equal(bits(on[0])[: len(rows), :, :3], bits(whole[0])[rows][..., :3])


# ------------------------------------------------------------------ 8. edits: the root is read from the live tree
def test_edits_move_geometry_into_an_empty_region(renderer):
    from computeraytracer_amd.scene import PackedScene, transform_records
    ps = scene_of("cornell", 100, 76)
    left = [(17, 1, [1, 0, 0, -300.0, 0, 1, 0, 0, 0, 0, 1, 0])]     # the large sphere to the frame's left edge, outside the room
    res = []
    try:
        for cull in (1, 0):
            options(renderer, wf_cull_miss=cull)
            renderer.upload(ps).build_accel("bvh2").reset_counters()
            renderer.frame(4).sync()
            img0, c0 = (renderer.read_accum(), renderer.read_rgba8()), renderer.gen_culled()
            renderer.transform_primitives(left).refit_accel()
            recs1 = renderer.read_primitives()
            renderer.reset_counters().frame(4).sync()
            img1, c1 = (renderer.read_accum(), renderer.read_rgba8()), renderer.gen_culled()
            right = transform_records(recs1[16:17], np.eye(3), [512.0, 0.0, 0.0])   # the small sphere to the right edge
            renderer.update_primitives(16, right)
            renderer.refit_accel()
            recs2 = renderer.read_primitives()
            renderer.reset_counters().frame(4).sync()
            img2, c2 = (renderer.read_accum(), renderer.read_rgba8()), renderer.gen_culled()
            res.append((img0, c0, img1, c1, img2, c2))
        fresh = []
        for recs in (recs1, recs2):
            renderer.upload(PackedScene(recs, ps.lights, ps.camera, ps.spectra, ps.cie)).build_accel("bvh2").frame(4).sync()
            fresh.append((renderer.read_accum(), renderer.read_rgba8()))
    finally:
        options(renderer)
    (img0, c0, img1, c1, img2, c2), off = res
    print(f"edits: culled {c0} -> {c1} -> {c2}")
    for k in (0, 2, 4):
        same_image(res[0][k], off[k], f"on / off after {k // 2} edits")
    same_image(img1, fresh[0], "transformed / fresh upload")
    same_image(img2, fresh[1], "updated / fresh upload")
    assert (bits(img1[0]) != bits(img0[0])).any() and (bits(img2[0]) != bits(img1[0])).any()
    assert c0 > c1 > c2 > 0 and off[1] == off[3] == off[5] == 0


# ------------------------------------------------------------------ 9. where the cull is off
def test_where_the_cull_is_off(renderer):
    from computeraytracer_amd.scene import PackedScene
    ps = scene_of("cornell", 100, 76)
    prep = lambda r: r.upload(ps).build_accel("bvh2")
    ref = on_and_off(renderer, prep, lambda r: r.frame(4))[0]
    assert ref[2] > 0
    for what, opts in (("8-wide tree", dict(wf_width=8)), ("plain boxes", dict(quantize=0))):
        on, off = on_and_off(renderer, prep, lambda r: r.frame(4), **opts)
        assert on[2] == 0 and off[2] == 0, what
        same_image(on, off, what)
        same_image(on, ref, what + " / 4-wide quantised")
    # an adaptive render
    def adaptive(r):
        r.trace_adaptive(samples=4, threshold=1e30, min_samples=4)
        r.trace_adaptive(samples=2, threshold=0.0, min_samples=4)
    try:
        on, off = on_and_off(renderer, prep, adaptive)
    finally:
        renderer.reset()
    assert on[2] == 0 and off[2] == 0
    same_image(on, off, "adaptive")
    # four primitives (a tree of one node) and none
    for n in (4, 0):
        few = PackedScene(ps.primitives[:n].copy(), ps.lights, ps.camera, ps.spectra, ps.cie)
        on, off = on_and_off(renderer, lambda r: r.upload(few).build_accel("bvh2"), lambda r: r.frame(2))
        assert on[2] == 0 and off[2] == 0, f"{n} primitives"
        same_image(on, off, f"{n} primitives")


# ------------------------------------------------------------------ 10. a camera that is not finite
def test_non_finite_camera(renderer):
    ps = scene_of("cornell", 64, 48)
    cam = ps.camera.copy()
    cam[0] = np.nan
    ps = with_camera(ps, cam)
    on, off = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2"), lambda r: r.frame(2), counting=True)
    assert on[2] == 0 and off[2] == 0                            # a ray flagged kWfNanRay is never culled
    assert np.array_equal(bits(on[0]), bits(off[0])) and np.array_equal(on[1], off[1])
    assert {k: on[3][k] for k in COUNTED} == {k: off[3][k] for k in COUNTED}
