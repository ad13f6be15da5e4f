"""GPU tests of the deferred NEE term (run with -m gpu on an MI355X): a path that Russian roulette ends
while its NEE shadow ray is still pending finishes in that shade step and frees its slot; the term is added to the sample's
staging cell by the next shade launch of the pipe, if the ray was visible.  Option "wf_defer_nee" switches it; every case
renders with it on and off in the same process and asks for the same bits in the accumulator and in the rgba8 frame and,
where it counts, for the same counters.  crt_debug_deferred_nee says how many paths took the new route, so that no case
passes without it.

A path can be deferred only in a launch behind which slots are re-armed, that is while the host still sees work in a queue.
The frames here are small, so the pools are held smaller than a batch's work (option "wf_pool"): the work then lasts many
iterations, as it does on the benchmarked frame with the automatic pool."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu
DEFAULTS = dict(pipeline=1, quantize=1, wf_width=4, wf_trace_form=2, wf_defer=1, wf_cohort=16, wf_pool=0, wf_pipes=2,
                wf_finish_at=32768, wf_flush_at=4096, wf_tail_walk=1, wf_ring=32, frame_ring=0, time_kernels=0, wf_defer_nee=1)
COUNTED = ("rays", "paths", "bounces", "shadow", "hits", "walked")
# (scene, frame, samples, pool): ragged frames; the atrium's pool is the smallest that runs as two pipes
SHAPES = [("cornell", 100, 76, 8, 4096), ("mesh10k", 192, 108, 8, 16384), ("atrium250k", 480, 270, 16, 1 << 19)]
SHAPE = {s[0]: s for s in SHAPES}


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


def on_and_off(r, prepare, run, counting=False, **opts):
    """prepare(r) and run(r) with the option on and off: [(accum, rgba8, deferred, counters, what run returned)] for on, off."""
    out = []
    try:
        for d in (1, 0):
            options(r, **opts, wf_defer_nee=d)
            prepare(r)
            r.enable_counters(counting).reset_counters()
            extra = run(r)
            r.sync()
            out.append((r.read_accum(), r.read_rgba8(), r.deferred_nee(), r.counters() if counting else None, extra))
    finally:
        r.enable_counters(False)
        options(r)
    return out


def uploaded(name):
    _, w, h, _, _ = SHAPE[name]
    ps = scene_of(name, w, h)
    return lambda r: r.upload(ps).build_accel("bvh2")


# ------------------------------------------------------------------ 1. on = off, images and counters
@pytest.mark.parametrize("mode", ["bvh2", "lbvh"])
@pytest.mark.parametrize("form", [2, 1])
@pytest.mark.parametrize("name,w,h,spp,pool", SHAPES, ids=[s[0] for s in SHAPES])
def test_on_equals_off(renderer, name, w, h, spp, pool, form, mode):
    ps = scene_of(name, w, h)
    got = {}
    try:
        options(renderer, wf_trace_form=form, wf_pool=pool)
        renderer.upload(ps).build_accel(mode)                    # one build: the option acts at the next trace call
        for counting in (True, False):                           # (the counting kernels are instantiations of their own)
            for d in (1, 0):
                renderer.set_option("wf_defer_nee", d).enable_counters(counting).reset().reset_counters()
                renderer.frame(spp).sync()
                got[counting, d] = (renderer.read_accum(), renderer.read_rgba8(), renderer.deferred_nee(), renderer.counters() if counting else None)
        renderer.enable_counters(False).set_option("wf_pool", 0).set_option("wf_defer_nee", 1).reset().reset_counters()
        renderer.frame(spp).sync()                               # the automatic pool (it may hold the whole frame at once)
        auto = (renderer.read_accum(), renderer.read_rgba8(), renderer.deferred_nee())
    finally:
        renderer.enable_counters(False)
        options(renderer)
    on, off = got[True, 1], got[True, 0]
    paths = w * h * spp
    print(f"{name} {w}x{h} x {spp} form {form} {mode}: finished at once {on[2]} of {paths} paths = {on[2] / paths:.4f} per path "
          f"(not counting: {got[False, 1][2] / paths:.4f}; automatic pool: {auto[2] / paths:.4f})")
    same_image(on, off, "on / off")
    assert {k: on[3][k] for k in COUNTED} == {k: off[3][k] for k in COUNTED}
    assert on[3]["paths"] == paths
    assert on[2] > 0 and off[2] == 0
    same_image(got[False, 1], got[False, 0], "on / off, not counting")
    same_image(got[False, 1], on, "counting / not counting")
    assert got[False, 1][2] > 0 and got[False, 0][2] == 0
    same_image(auto, off, "automatic pool, on / small pool, off")


# ------------------------------------------------------------------ 2. several batches open: the entries count as alive
@pytest.mark.parametrize("name", ["mesh10k", "atrium250k"])
def test_pipelined_batches(renderer, name):
    _, w, h, _, pool = SHAPE[name]

    def six(r):
        for _ in range(6):
            r.frame(4)                                           # wf_cohort = 1: six batches, none synced

    on, off = on_and_off(renderer, uploaded(name), six, wf_cohort=1, wf_pool=pool)
    whole_on, whole_off = on_and_off(renderer, uploaded(name), lambda r: r.frame(24), wf_cohort=1, wf_pool=pool)
    same_image(on, off, "6 x frame(4): on / off")
    same_image(on, whole_on, "6 x frame(4) / frame(24)")
    same_image(whole_on, whole_off, "frame(24): on / off")
    print(f"{name}: 6 x frame(4) finished at once {on[2] / (w * h * 24):.4f} per path, frame(24) {whole_on[2] / (w * h * 24):.4f}")
    assert on[2] > 0 and whole_on[2] > 0 and off[2] == 0 and whole_off[2] == 0


# ------------------------------------------------------------------ 3. run ends, the tail and the side pools
def launches_of(r):
    """(launches, iterations) of the last frame() call and the sync behind it (option time_kernels: one timed traversal
    launch per iteration)."""
    r.sync()
    return r.last_trace_ms()[1], r.last_kernel_ms()[1]


@pytest.mark.parametrize("name,pool", [("cornell", 1024), ("mesh10k", 2048)])
def test_run_ends(renderer, name, pool):
    """Runs of ONE sample: the pool holds a seventh (a tenth) of a sample's paths, so that each run's work outlasts the
    three shade steps a path needs before roulette can end it."""

    def eight(r):
        for _ in range(8):
            r.frame(1).sync()

    on, off = on_and_off(renderer, uploaded(name), eight, wf_pool=pool)
    whole = on_and_off(renderer, uploaded(name), lambda r: r.frame(8), wf_pool=pool)
    same_image(on, off, "8 x (frame(1); sync): on / off")
    same_image(on, whole[0], "8 x (frame(1); sync) / frame(8)")
    same_image(whole[0], whole[1], "frame(8): on / off")
    assert on[2] > 0 and whole[0][2] > 0 and off[2] == 0


def test_tail_mode_and_side_pools(renderer):
    """mesh10k through 4 096 slots, one pipe.  (a) Nothing is ever evicted (wf_flush_at = wf_finish_at = 0): once the queue is
    dry the pipe goes on, without generate launches, until its last path has ended -- by the policy in tail mode (fewer rays
    than a quarter of the pool), behind the one sweep of the whole pool that the launches which deferred ask for.  One
    batch, no finish launch, one resolve: launches = 2 x iterations + generate launches + 1, so the iterations without a
    generate launch can be counted.  (b) With wf_flush_at = 4096 the flush sends everything alive to the side pools as soon
    as the queue is dry (a pool of 4 096 slots lists no more rays than that): the run takes fewer iterations than (a), by
    the length of the tail.  (c) Eight batches of one sample, none synced, retire by eviction under the batches behind them
    (wf_finish_at = 32768).  All of them give the image of frame(8), with the option on and off."""
    name, pool = "mesh10k", 4096
    _, w, h, _, _ = SHAPE[name]

    def one_call(r):
        r.frame(8)
        return launches_of(r)

    def eight_open(r):
        for _ in range(8):
            r.frame(1)

    tail = on_and_off(renderer, uploaded(name), one_call, wf_pool=pool, wf_flush_at=0, wf_finish_at=0, time_kernels=1)
    side = on_and_off(renderer, uploaded(name), one_call, wf_pool=pool, time_kernels=1)
    mid = on_and_off(renderer, uploaded(name), eight_open, wf_pool=pool, wf_cohort=1)
    same_image(tail[0], tail[1], "tail: on / off")
    same_image(side[0], side[1], "side pools: on / off")
    same_image(mid[0], mid[1], "eviction under the next batch: on / off")
    same_image(tail[0], side[0], "tail / side pools")
    same_image(tail[0], mid[0], "tail / eight open batches")
    for what, res in (("tail", tail), ("side pools", side)):
        for k, d in enumerate((1, 0)):
            launches, iters = res[k][4]
            print(f"{what}, wf_defer_nee {d}: {launches} launches, {iters} iterations, finished at once {res[k][2]}")
    for k in (0, 1):
        launches, iters = tail[k][4]
        gens = launches - 2 * iters - 1
        assert 0 < gens < iters, (launches, iters)
        assert iters - gens >= 3, f"{iters - gens} iterations without a generate launch: no tail"
        assert side[k][4][1] < iters, "the flush did not cut the tail short: nothing went to the side pools"
    assert tail[0][4][1] < tail[1][4][1], "fewer iterations with the slots freed early"
    assert tail[0][2] > 0 and side[0][2] > 0 and mid[0][2] > 0
    assert tail[1][2] == side[1][2] == mid[1][2] == 0


# ------------------------------------------------------------------ 4. other paths through the library
def test_frame_ring(renderer):
    name = "cornell"
    _, w, h, _, pool = SHAPE[name]
    ps = scene_of(name, w, h)
    frames = {}
    try:
        for d in (1, 0):
            options(renderer, wf_defer_nee=d, wf_cohort=1, wf_pool=pool)
            renderer.upload(ps).build_accel("bvh2").set_option("frame_ring", 8).reset_counters()
            got = []
            for s in range(1, 7):
                renderer.frame(1)
                if s >= 2:
                    got.append(renderer.read_sample_rgba8(s - 1))    # the frame before the one in flight
            got.append(renderer.read_sample_rgba8(6))
            renderer.sync()
            frames[d] = got + [renderer.read_rgba8()], renderer.deferred_nee()
    finally:
        renderer.set_option("frame_ring", 0)
        options(renderer)
    assert len(frames[1][0]) == 7
    for k, (a, b) in enumerate(zip(frames[1][0], frames[0][0])):
        assert np.array_equal(a, b), f"frame {k + 1} of the ring differs"
    assert frames[1][1] > 0 and frames[0][1] == 0


def test_write_accum_then_resume(renderer):
    name = "mesh10k"
    pool = SHAPE[name][4]

    def resume(r):
        r.frame(5).sync()
        ckpt = r.read_accum()
        r.reset()
        r.write_accum(ckpt, 5).frame(3)

    on, off = on_and_off(renderer, uploaded(name), resume, wf_pool=pool)
    whole = on_and_off(renderer, uploaded(name), lambda r: r.frame(8), wf_pool=pool)[1]
    same_image(on, off, "on / off")
    same_image(on, whole, "resumed / frame(8), off")
    assert on[2] > 0 and off[2] == 0


@pytest.mark.parametrize("rank", [0, 1])
def test_two_ranks_of_a_partition(renderer, rank):
    name = "mesh10k"
    _, w, h, _, pool = SHAPE[name]
    ps = scene_of(name, w, h)
    on, off = on_and_off(renderer, lambda r: r.upload(ps).build_accel("bvh2").set_row_bands(8, 2, rank), lambda r: r.frame(8), wf_pool=pool // 2)
    same_image(on, off, f"rank {rank}: on / off")
    assert on[2] > 0 and off[2] == 0
    from computeraytracer_amd.partition import band_rows
    rows = band_rows(h, 2, rank, 8)
    whole = on_and_off(renderer, uploaded(name), lambda r: r.frame(8), wf_pool=pool)[1]
    assert np.array_equal(bits(on[0])[: len(rows), :, :3], bits(whole[0])[rows][..., :3])


def test_adaptive_after_a_uniform_batch(renderer):
    name = "mesh10k"
    pool = SHAPE[name][4]

    def adaptive(r):
        r.frame(4)                                               # a uniform batch, not synced; reset() ends its run
        r.reset()
        r.trace_adaptive(samples=4, threshold=1e30, min_samples=4)
        r.trace_adaptive(samples=4, threshold=0.0, min_samples=4)

    try:
        on, off = on_and_off(renderer, uploaded(name), adaptive, wf_pool=pool)
    finally:
        renderer.reset()
    same_image(on, off, "on / off")
    assert on[2] > 0 and off[2] == 0


def test_an_edit_between_two_renders_without_sync(renderer):
    name = "cornell"
    _, w, h, _, pool = SHAPE[name]
    ps = scene_of(name, w, h)
    cam = ps.camera.copy()
    cam[4:7] = (cam[4] + 150.0, cam[5] + 120.0, cam[6])
    first = []

    def run(r):
        r.frame(6)
        r.set_camera(cam)                                        # ends the run in flight; the accumulation starts again
        first.append(r.deferred_nee())
        r.frame(6)

    on, off = on_and_off(renderer, uploaded(name), run, wf_pool=pool)
    moved = on_and_off(renderer, lambda r: uploaded(name)(r).set_camera(cam), lambda r: r.frame(6), wf_pool=pool)[1]
    same_image(on, off, "on / off")
    same_image(on, moved, "after the edit / a render of the moved camera alone, off")
    assert 0 < first[0] < on[2] and first[1] == 0 and off[2] == 0
