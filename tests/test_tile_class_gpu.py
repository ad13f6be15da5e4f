"""GPU tests of the tile classes (run with -m gpu on an MI355X): at run set-up k_wf_tile_classes decides,
per 8x8 tile, whether the tile's camera rays miss the root's four child boxes -- or enter one -- for every sample, and
k_wf_gen's CULL form looks that up instead of drawing and testing every sample.  Option "wf_cull_classes" switches it; every
case renders with the classes on and off in the same process and asks for the same bits in the accumulator and the rgba8
frame, the same count of culled pixel-samples and, where it counts, the same counters.  The device table is compared with
the same definition evaluated on the CPU."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu
DEFAULTS = dict(pipeline=1, quantize=1, wf_width=4, wf_trace_form=2, wf_defer=1, wf_cohort=16, wf_pool=0, wf_cull_miss=1,
                wf_cull_classes=1)
# "nodes" is compared where k_wf_gen alone adds to it (test_counters_of_a_frame_of_miss_tiles): in a frame that traverses,
# the node steps of a walk depend on the order in which the lanes of a wave shrink t_max, and two runs with the same
# options differ in it (tests/test_gen_cull_gpu.py leaves it out for the same reason; the first test below prints it)
COUNTED = ("rays", "paths", "bounces", "shadow", "hits", "walked")
MAYBE, MISS, ENTER = 0, 1, 2


def options(r, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        r.set_option(k, v)


def same_image(a, b, what):
    (acc, rgba), (acc_o, rgba_o) = a[:2], b[:2]
    bad = (bits(acc)[..., :3] != bits(acc_o)[..., :3]).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} accumulator pixels differ, first at {np.argwhere(bad)[0][::-1]}"
    assert np.array_equal(rgba, rgba_o), f"{what}: {int((rgba != rgba_o).sum())} rgba8 bytes differ"


def scene_of(name, w, h):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scenes_synth import atrium250k, mesh10k
    return dict(cornell=cornell, mesh10k=mesh10k, atrium250k=atrium250k)[name](w, h)


def tables(r):
    """The device table, after checking it against the host's."""
    dev, host = r.tile_classes(), r.tile_classes(host=True)
    assert dev.shape == host.shape and np.array_equal(dev, host), f"{int((dev != host).sum())} of {dev.size} tile classes differ between device and host"
    return dev


def miss_tile_pixels(table, tw, th):
    """Valid pixels of the MISS tiles of a tw x th tile rectangle."""
    ys, xs = np.nonzero(table == MISS)
    return int((np.minimum(8, tw - 8 * xs) * np.minimum(8, th - 8 * ys)).sum())


def classes_on_and_off(r, run, counting=False):
    """run(r) from a reset with the classes on and off: [(accum, rgba8, culled, counters)]."""
    out = []
    for cls in (1, 0):
        r.set_option("wf_cull_classes", cls).enable_counters(counting).reset().reset_counters()
        run(r)
        r.sync()
        out.append((r.read_accum(), r.read_rgba8(), r.gen_culled(), r.counters() if counting else None))
    return out


def equal_runs(on, off, what, counting=False):
    same_image(on, off, what)
    assert on[2] == off[2], f"{what}: culled {on[2]} with the classes, {off[2]} without"
    if counting:
        assert {k: on[3][k] for k in COUNTED} == {k: off[3][k] for k in COUNTED}, what


# ------------------------------------------------------------------ 1. the table, and on = off
SHAPES = [("cornell", 100, 76, 8), ("mesh10k", 192, 108, 8), ("atrium250k", 480, 270, 8)]


@pytest.mark.parametrize("mode", ["bvh2", "lbvh"])
@pytest.mark.parametrize("form", [2, 1])
@pytest.mark.parametrize("name,w,h,spp", SHAPES, ids=[s[0] for s in SHAPES])
def test_table_and_equal_outputs(renderer, name, w, h, spp, form, mode):
    ps = scene_of(name, w, h)
    try:
        options(renderer, wf_trace_form=form)
        renderer.upload(ps).build_accel(mode)
        table = tables(renderer)
        got = {counting: classes_on_and_off(renderer, lambda r: r.frame(spp), counting) for counting in (True, False)}
        again = classes_on_and_off(renderer, lambda r: r.frame(spp), True)[1]       # the classes off, a second time
        print(f"node steps: classes on {got[True][0][3]['nodes']}, off {got[True][1][3]['nodes']}, off again {again[3]['nodes']}")
    finally:
        renderer.enable_counters(False)
        options(renderer)
    for counting in (True, False):
        equal_runs(*got[counting], f"counting {counting}: classes on / off", counting)
    same_image(got[True][0], got[False][0], "counting / not counting")
    assert got[True][0][3]["paths"] == w * h * spp
    culled = got[False][0][2]
    from_miss = miss_tile_pixels(table, w, h) * spp
    n = {k: int((table == v).sum()) for k, v in (("MISS", MISS), ("ENTER", ENTER), ("MAYBE", MAYBE))}
    print(f"{name} {w}x{h} form {form} {mode}: tiles {n}, culled {culled} of {w * h * spp} pixel-samples, "
          f"{from_miss} of them in MISS tiles: share {from_miss / max(culled, 1):.4f}")
    assert 0 < from_miss <= culled                               # a MISS tile holds only what the per-sample test culls


def test_counters_of_a_frame_of_miss_tiles(renderer):
    """A camera that looks away: every tile is MISS, no ray is ever listed, and every counter is k_wf_gen's own -- the
    counting variant adds for a MISS chunk's lanes what it adds for a chunk the per-sample test culls, node steps included."""
    ps = scene_of("cornell", 100, 76)
    cam = ps.camera.copy()
    cam[4:7] = 2.0 * cam[0:3] - cam[4:7]                         # look-at mirrored at the eye
    try:
        options(renderer)
        renderer.upload(ps).build_accel("bvh2").set_camera(cam)
        table = tables(renderer)
        on, off = classes_on_and_off(renderer, lambda r: r.frame(5), True)
    finally:
        renderer.enable_counters(False)
        options(renderer)
    assert (table == MISS).all()
    equal_runs(on, off, "looking away", True)
    assert on[3] == off[3]                                       # every counter, "nodes" included
    assert on[2] == on[3]["paths"] == 100 * 76 * 5 and on[3]["nodes"] == 4 * on[2]
    assert not bits(on[0])[..., :3].any()


# ------------------------------------------------------------------ 2. every change of the inputs makes a new table
def test_the_table_follows_its_inputs(renderer):
    from computeraytracer_amd.scene import transform_records
    ps = scene_of("cornell", 100, 76)
    seen = []

    def stage(what):
        t = tables(renderer)
        on, off = classes_on_and_off(renderer, lambda r: r.frame(4))
        equal_runs(on, off, what)
        if seen:
            assert seen[-1][1].shape != t.shape or (seen[-1][1] != t).any(), f"{what}: the table did not change"
        print(f"{what}: MISS {int((t == MISS).sum())} ENTER {int((t == ENTER).sum())} MAYBE {int((t == MAYBE).sum())}, culled {on[2]}")
        seen.append((what, t, on))

    try:
        options(renderer)
        renderer.upload(ps).build_accel("bvh2")
        stage("standard camera")
        cam = ps.camera.copy()
        cam[4:7] = (cam[4] + 150.0, cam[5] + 120.0, cam[6])      # the box leaves the frame's centre
        renderer.set_camera(cam)
        stage("set_camera")
        renderer.set_camera(ps.camera)
        stage("set_camera back")
        assert np.array_equal(seen[0][1], seen[2][1])
        same_image(seen[0][2], seen[2][2], "the first camera again")
        renderer.transform_primitives([(17, 1, [1, 0, 0, -300.0, 0, 1, 0, 0, 0, 0, 1, 0])]).refit_accel()   # the large sphere leaves the room to the left
        stage("transform_primitives + refit_accel")
        recs = renderer.read_primitives()
        renderer.update_primitives(16, transform_records(recs[16:17], np.eye(3), [512.0, 0.0, 0.0]))       # the small one to the right
        renderer.refit_accel()
        stage("update_primitives + refit_accel")
        renderer.build_accel("lbvh")
        stage("build_accel with the lbvh builder")
        renderer.set_row_bands(8, 2, 0)
        stage("row bands, part 0 of 2")
        renderer.set_row_bands(8, 2, 1)
        stage("row bands, part 1 of 2")
    finally:
        options(renderer)
    assert len(seen) == 8


def test_an_edit_ends_the_live_run(renderer):
    """Render, edit, render again with no option change, reset or sync in between (every call its own batch, left in
    flight): the edit itself has to end the run, or the next batch would be generated with the old table -- a MISS tile of the
    old camera stays black where the new one sees the box.  Compared with the classes off; every render after an edit has
    run a set-up of its own."""
    ps = scene_of("cornell", 100, 76)
    cam = ps.camera.copy()
    cam[4:7] = (cam[4] + 150.0, cam[5] + 120.0, cam[6])
    got, setups = {}, {}
    try:
        for cls in (1, 0):
            options(renderer, wf_cull_classes=cls, wf_cohort=1)
            renderer.upload(ps).build_accel("bvh2").reset_counters()
            n0, shots = renderer.tile_class_setups(), []
            renderer.frame(2)
            renderer.set_camera(cam).frame(2)
            shots.append(renderer.read_rgba8())
            renderer.frame(1)
            renderer.transform_primitives([(17, 1, [1, 0, 0, -300.0, 0, 1, 0, 0, 0, 0, 1, 0])]).refit_accel()
            renderer.frame(2)
            renderer.set_camera(ps.camera).frame(2)
            renderer.set_row_bands(8, 2, 1).frame(2)
            renderer.sync()
            got[cls] = (renderer.read_accum(), renderer.read_rgba8(), renderer.gen_culled(), shots)
            setups[cls] = renderer.tile_class_setups() - n0
    finally:
        options(renderer)
    same_image(got[1], got[0], "after the edits")
    assert np.array_equal(got[1][3][0], got[0][3][0]), "after set_camera"
    assert got[1][2] == got[0][2] > 0
    print(f"set-ups that classified: {setups[1]} with the classes, {setups[0]} without")
    assert setups[1] >= 5 and setups[0] == 0                     # the first render and one after each of the four edits (the read ends a run too)


# ------------------------------------------------------------------ 3. the frame ring and twenty one-sample batches
def test_frame_ring_and_small_batches(renderer):
    ps = scene_of("cornell", 96, 64)
    frames = {}
    try:
        for cls in (1, 0):
            options(renderer, wf_cull_classes=cls, wf_cohort=1)
            renderer.upload(ps).build_accel("bvh2").set_option("frame_ring", 32)
            renderer.reset_counters()
            for _ in range(20):
                renderer.frame(1)
            renderer.sync()
            frames[cls] = [renderer.read_sample_rgba8(s) for s in range(1, 21)] + [renderer.read_rgba8()], bits(renderer.read_accum()), renderer.gen_culled()
    finally:
        renderer.set_option("frame_ring", 0)
        options(renderer)
    for k, (a, b) in enumerate(zip(frames[1][0], frames[0][0])):
        assert np.array_equal(a, b), f"frame {k + 1} differs"
    assert np.array_equal(frames[1][1], frames[0][1])
    assert frames[1][2] == frames[0][2] > 0


# ------------------------------------------------------------------ 4. where the classes do nothing
def test_where_the_classes_do_nothing(renderer):
    from computeraytracer_amd.scene import PackedScene
    ps = scene_of("cornell", 100, 76)
    few = PackedScene(ps.primitives[:4].copy(), ps.lights, ps.camera, ps.spectra, ps.cie)

    def adaptive(r):
        r.trace_adaptive(samples=4, threshold=1e30, min_samples=4)
        r.trace_adaptive(samples=2, threshold=0.0, min_samples=4)

    cases = (("wf_cull_miss 0", ps, dict(wf_cull_miss=0), lambda r: r.frame(4)), ("adaptive", ps, {}, adaptive),
             ("8-wide tree", ps, dict(wf_width=8), lambda r: r.frame(4)), ("four primitives", few, {}, lambda r: r.frame(4)))
    try:
        for what, scene, opts, run in cases:
            options(renderer, **opts)
            renderer.upload(scene).build_accel("bvh2")
            n0 = renderer.tile_class_setups()
            on, off = classes_on_and_off(renderer, run)
            renderer.reset()
            equal_runs(on, off, what)
            assert on[2] == 0, what                              # nothing is culled there, with or without the classes
            assert renderer.tile_class_setups() == n0, f"{what}: a run set-up launched the classifier"
        options(renderer)                                        # (and where they do something, the hook moves)
        renderer.upload(ps).build_accel("bvh2")
        n0 = renderer.tile_class_setups()
        classes_on_and_off(renderer, lambda r: r.frame(4))
        assert renderer.tile_class_setups() == n0 + 1            # one run with the classes on, one with them off
    finally:
        renderer.reset()
        options(renderer)
