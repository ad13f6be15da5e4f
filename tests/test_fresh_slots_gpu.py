"""GPU tests of the fresh-slot re-arm (run with -m gpu on an MI355X): k_wf_gen starts a path with one store of the slot's
misc (kWfFresh: work id, flags, sample, seed) and the next shade step rebuilds its camera ray, RNG state and starting
throughput.  Every case compares the wavefront pipeline with the single-kernel form (pipeline 0), which shares none of
that code, bit for bit on the accumulator and on every rgba8 byte: the benchmarked shape (fresh slots evicted while their
camera rays are in flight), 1-spp cohorts, a ragged frame, adaptive rounds, a camera orbit and calls of mixed sizes that
take a pipe from tail mode back to normal mode."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu
DEFAULTS = dict(pipeline=1, quantize=1, wf_width=4, wf_trace_form=2, wf_defer=1, wf_cohort=16)


def options(r, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        r.set_option(k, v)


def assert_same_image(acc, rgba, acc_o, rgba_o):
    bad = (bits(acc)[..., :3] != bits(acc_o)[..., :3]).any(-1)
    assert not bad.any(), f"{int(bad.sum())} accumulator pixels differ, first at {np.argwhere(bad)[0][::-1]}"
    assert np.array_equal(rgba, rgba_o), f"{int((rgba != rgba_o).sum())} rgba8 bytes differ"


def both_forms(r, ps, run, mode="bvh2"):
    """run(r) under the wavefront pipeline and under the single-kernel form: the two images."""
    out = []
    try:
        for pipeline in (1, 0):
            options(r, pipeline=pipeline)
            r.upload(ps).build_accel(mode)
            run(r)
            r.sync()
            out.append((r.read_accum(), r.read_rgba8()))
    finally:
        options(r)
    return out


def test_s2_1080p_two_64_spp_calls(renderer):
    """The benchmarked shape: the first batch retires while the second one's camera rays are in flight, so fresh slots
    (traced, never shaded) are moved to the side pool and finished there."""
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(1920, 1080)
    (a, r8), (a0, r80) = both_forms(renderer, ps, lambda r: r.frame(64).frame(64))
    assert_same_image(a, r8, a0, r80)


def test_one_spp_cohort_loop(renderer):
    """Every call its own 1-sample batch, with and without a sync in between."""
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(640, 360)

    def run(r):
        r.set_option("wf_cohort", 1)
        for k in range(12):
            r.frame(1)
            if k % 4 == 3:
                r.sync()

    (a, r8), (a0, r80) = both_forms(renderer, ps, run)
    assert_same_image(a, r8, a0, r80)


def test_ragged_frame(renderer):
    """A frame that is no whole number of 8x8 tiles: items outside it start no path."""
    from computeraytracer_amd.scenes_synth import mesh10k
    ps = mesh10k(333, 217)
    (a, r8), (a0, r80) = both_forms(renderer, ps, lambda r: r.frame(5).frame(3))
    assert_same_image(a, r8, a0, r80)


def test_adaptive_rounds(renderer):
    """Adaptive batches store the full-frame id and the tile's own sample index in the fresh slot."""
    from computeraytracer_amd.scenes_synth import mesh10k
    ps = mesh10k(200, 136)

    def run(r):
        r.trace_adaptive(samples=4, threshold=1e30, min_samples=4)
        _, e = r.read_adaptive()
        thr = float(np.median(e))
        for _ in range(3):
            r.trace_adaptive(samples=3, threshold=thr, min_samples=4)

    try:
        (a, r8), (a0, r80) = both_forms(renderer, ps, run)
    finally:
        renderer.reset()
    assert_same_image(a, r8, a0, r80)


def test_camera_orbit(renderer):
    """Each set_camera runs the pool to its end first: gen and shade always see the same camera."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import orbit_cameras
    ps = cornell(256, 192)
    cams = list(orbit_cameras(ps.camera, 5)[1:])
    imgs = {}
    try:
        for pipeline in (1, 0):
            options(renderer, pipeline=pipeline)
            renderer.upload(ps).build_accel("bvh2")
            for cam in cams:                        # no sync: each set_camera flushes what the calls before it left
                renderer.set_camera(cam)
                renderer.frame(2).frame(1)
            renderer.sync()
            imgs[pipeline] = (renderer.read_accum(), renderer.read_rgba8())
            for i, cam in enumerate(cams):          # and every camera's image on its own
                renderer.set_camera(cam)
                renderer.frame(2).frame(1).sync()
                imgs[(pipeline, i)] = (renderer.read_accum(), renderer.read_rgba8())
    finally:
        options(renderer)
    assert_same_image(*imgs[1], *imgs[0])
    for i in range(len(cams)):
        assert_same_image(*imgs[(1, i)], *imgs[(0, i)])


def test_mixed_sizes_without_sync(renderer):
    """Calls of mixed sizes back to back: a pipe in tail mode (no work left, list-walking shade) is switched back to
    normal mode when the next batch is published into the live pool."""
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(480, 270)

    def run(r):
        for n in (8, 1, 4, 1, 1, 16, 2):
            r.frame(n)

    (a, r8), (a0, r80) = both_forms(renderer, ps, run)
    assert_same_image(a, r8, a0, r80)


# rays, paths, walked of the wavefront pipeline before fresh slots existed (the same samples, the same settings)
PARENT_COUNTS = (12698963, 4147200, 10556346)


def test_counters_unchanged(renderer):
    """Counting mode (batches folded on the host after each one): rays and paths equal the single-kernel form's, and
    rays, paths and walked equal what the pipeline counted before the fresh-slot re-arm."""
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(480, 270)
    got = {}
    try:
        for pipeline in (1, 0):
            options(renderer, pipeline=pipeline)
            renderer.upload(ps).build_accel("bvh2").enable_counters(True).reset_counters()
            renderer.frame(16).frame(16).sync()
            c = renderer.counters()
            got[pipeline] = (c["rays"], c["paths"], c["walked"])
    finally:
        renderer.enable_counters(False)
        options(renderer)
    print("counters", got)
    assert got[1][:2] == got[0][:2]
    assert got[1] == PARENT_COUNTS
