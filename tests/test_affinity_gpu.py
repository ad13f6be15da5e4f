"""GPU tests of the region-major work shards (option "wf_affinity"; run with -m gpu on an MI355X): with the
option on, shard 8 g + k of a batch's work queue hands out the tiles of image region k for the samples congruent to g
modulo 8 (csrc/crt_work_map.h) and a traversal wave starts on the ray lists of its own XCD's region.  Which path runs when
and where changes; what a path computes and where its sample is stored does not.  So every case renders with the option on
and off in the same process and asks for the same bits in the accumulator and in the rgba8 frame and, where it counts, for
the same counters; the first case also asks the oracle.  crt_debug_mapped_gen_launches says whether generate launches
handed out region-major work, so that no case passes with the option ignored; that the mapping itself is a partition of
the work is tests/host/work_map_test.cpp's.

Counters (rays, paths, shadow) are compared where check() is used.  The cohort case, the partition case and the adaptive
case compare images only: counting folds the counters on the host after every batch, which ends the merging of small
calls into cohorts and the batches in flight that the first is about, and the other two are about where frames go."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu
DEFAULTS = dict(wf_affinity=0, wf_pipes=2, wf_pool=0, wf_cohort=16)
COUNTED = ("rays", "paths", "shadow")


@pytest.fixture(scope="module")
def ctx():
    from computeraytracer_amd import Renderer
    rs = [Renderer(0) for _ in range(2)]
    yield rs
    for r in rs:
        r.close()


def options(r, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        r.set_option(k, v)


def same_image(a, b, what):
    (acc, rgba), (acc_o, rgba_o) = a[:2], b[:2]
    assert acc.shape == acc_o.shape and rgba.shape == rgba_o.shape, what
    bad = (bits(acc)[..., :3] != bits(acc_o)[..., :3]).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} accumulator pixels differ, first at {np.argwhere(bad)[0][::-1]}"
    assert np.array_equal(rgba, rgba_o), f"{what}: {int((rgba != rgba_o).sum())} rgba8 bytes differ"


def on_and_off(r, ps, run, counting=False, mapped=True, **opts):
    """The scene rendered by run(r) with the option on and off: [(accum, rgba8, counters, what run returned)] for on, off.
    So that no case passes without the mapping: with the option on, generate launches handed out region-major work
    (crt_debug_mapped_gen_launches; mapped=False: an adaptive run, which never does), with it off none did."""
    out = []
    try:
        r.upload(ps).build_accel("bvh2")
        for a in (1, 0):
            options(r, **opts, wf_affinity=a)
            r.enable_counters(counting).reset().reset_counters()
            n0 = r.mapped_gen_launches()
            extra = run(r)
            r.sync()
            n = r.mapped_gen_launches() - n0
            assert (n > 0) if (a and mapped) else (n == 0), f"wf_affinity={a}: {n} generate launches with the mapping"
            out.append((r.read_accum(), r.read_rgba8(), r.counters() if counting else None, extra))
    finally:
        r.enable_counters(False)
        options(r)
    return out


def check(r, ps, run, what, paths=None, **opts):
    on, off = on_and_off(r, ps, run, **opts)
    same_image(on, off, f"{what}: on / off")
    con, coff = on_and_off(r, ps, run, counting=True, **opts)
    same_image(con, coff, f"{what}: on / off, counting")
    same_image(con, on, f"{what}: counting / not counting")
    assert {k: con[2][k] for k in COUNTED} == {k: coff[2][k] for k in COUNTED}, what
    if paths is not None:
        assert con[2]["paths"] == paths
    return on


def test_cornell_45_tiles_against_the_oracle(ctx, orc):
    """72 x 40: 9 x 5 = 45 tiles, not a multiple of the 8 regions; 3 samples: fewer than the 8 sample groups."""
    from computeraytracer_amd import cornell
    ps = cornell(72, 40)
    on = check(ctx[0], ps, lambda r: r.frame(3), "cornell 72x40 x 3", paths=72 * 40 * 3)
    acc_o, rgba_o, _ = orc.Scene.from_packed(ps).render(3)
    same_image(on, (acc_o, rgba_o), "cornell 72x40 x 3: on / oracle")


def test_a_ragged_frame_with_a_partial_tile_row(ctx):
    """76 x 37: 10 x 5 tiles, the last column and the last row of tiles hang over the frame."""
    from computeraytracer_amd import cornell
    check(ctx[0], cornell(76, 37), lambda r: r.frame(11), "cornell 76x37 x 11", paths=76 * 37 * 11)


def test_one_tile(ctx):
    """8 x 8: one tile, seven regions are empty; 13 samples: the groups hold 2 or 1."""
    from computeraytracer_amd.scenes_synth import mesh10k
    check(ctx[0], mesh10k(8, 8), lambda r: r.frame(13), "mesh10k 8x8 x 13", paths=8 * 8 * 13)


def test_two_calls_of_64_and_5_samples(ctx):
    """200 x 120 (375 tiles), 64 samples and 5 more in a second call: two batches whose shards differ in size."""
    from computeraytracer_amd.scenes_synth import atrium250k
    check(ctx[0], atrium250k(200, 120), lambda r: r.frame(64).frame(5), "atrium250k 200x120 x 64 + 5", paths=200 * 120 * 69)


def test_cohorts_of_one_sample_calls_on_four_pipes(ctx):
    """320 one-sample calls at 96 x 64 on four pipes: cohorts of 16 samples, many batches in flight at once."""
    from computeraytracer_amd import cornell

    def run(r):
        for _ in range(320):
            r.frame(1)
    on, off = on_and_off(ctx[0], cornell(96, 64), run, wf_pipes=4, wf_pool=1 << 19, wf_cohort=2)
    same_image(on, off, "320 x 1 sample, four pipes: on / off")


def test_two_rank_partition_in_bands_of_8(ctx):
    """Two contexts as the ranks of a partition in bands of 8 rows (72 x 61: ragged): the gathered frame, on and off."""
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(72, 61)
    got = []
    try:
        for a in (1, 0):
            for r in ctx:
                r.sync()
            for r in ctx:
                r.comm_destroy()
            cid = Renderer.comm_unique_id(local=True)
            for k, r in enumerate(ctx):
                options(r, wf_affinity=a)
                r.comm_init(cid, k, 2).upload(ps).comm_partition(8).build_accel("bvh2")
            n0 = [r.mapped_gen_launches() for r in ctx]
            for r in ctx:
                r.frame(4)
            for r in ctx:
                r.gather(rgba8=True, preview=True)
            for r, n in zip(ctx, n0):
                assert (r.mapped_gen_launches() > n) if a else (r.mapped_gen_launches() == n)
            got.append([(r.read_frame_accum(), r.read_frame_rgba8()) for r in ctx])
    finally:
        for r in ctx:
            r.sync()
        for r in ctx:
            r.comm_destroy()
            options(r)
    for k in range(2):
        same_image(got[0][k], got[1][k], f"rank {k}: on / off")
    same_image(got[0][0], got[0][1], "rank 0 / rank 1")
    with Renderer(0) as one:
        one.upload(ps).build_accel("bvh2").frame(4).sync()
        same_image(got[0][0], (one.read_accum(), one.read_rgba8()), "partition / one context")


def test_an_adaptive_round_keeps_its_mapping(ctx):
    """crt_trace_adaptive's queues keep the plain ranges: two rounds, on and off."""
    from computeraytracer_amd import cornell

    def run(r):
        active = [r.trace_adaptive(samples=4, min_samples=4, threshold=0.0) for _ in range(2)]
        r.sync()
        return active, r.read_adaptive()
    on, off = on_and_off(ctx[0], cornell(72, 61), run, mapped=False)
    same_image(on, off, "adaptive rounds: on / off")
    assert on[3][0] == off[3][0] == [72, 72]
    for g, w in zip(on[3][1], off[3][1]):
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
