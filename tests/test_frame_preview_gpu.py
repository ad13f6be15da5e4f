"""GPU tests of adaptive sampling and the denoised previews across a partition (include/crt.h "The frame of a partition",
DESIGN.md 6h; run with -m gpu on an MI355X): crt_trace_adaptive under bands of a multiple of 8 rows, crt_gather with
CRT_GATHER_PREVIEW, crt_read_frame_adaptive, crt_denoise_frame and crt_denoise_adaptive_frame.

Every test runs in this process on device 0: two to four ranks of the in-process transport (one test: one rank over RCCL).
The yardstick is always one unpartitioned context after the same calls, compared bit for bit -- the kernels and their inputs
are the same, so there is no tolerance.  The unpartitioned runs are made once per module and only read afterwards."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ENOMEM = -1, -3, -4
W, H = 72, 61                                                  # neither a multiple of 8: a partial last tile row and column
TX, TY = (W + 7) // 8, (H + 7) // 8
ROUNDS, SPP = 4, 4
AS_FILTERS = [dict(), dict(iterations=0), dict(iterations=2, sigma_variance=3.0, sigma_normal=0.25, sigma_plane=0.6)]


@pytest.fixture(scope="module")
def ps():
    from computeraytracer_amd import cornell
    return cornell(W, H)


@pytest.fixture(scope="module")
def pool():
    from computeraytracer_amd import Renderer
    rs = [Renderer(0) for _ in range(4)]
    yield rs
    for r in rs:
        r.close()


@pytest.fixture(scope="module")
def ref(ps):
    """What one unpartitioned context gives: the adaptive rounds (and every filter after the last one, and one round more),
    and the uniform frames of 4 and 8 samples with their filters."""
    from computeraytracer_amd import Renderer
    out = dict(rounds=[], uniform={})
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2")
        # the threshold: the median tile error at 8 samples, so the third selection retires about half of the tiles
        for _ in range(2):
            r.trace_adaptive(samples=SPP, min_samples=SPP, threshold=0.0)
        e8 = r.read_adaptive()[1]
        assert np.isfinite(e8).all()
        out["threshold"] = thr = float(np.median(e8))
        r.reset()
        for k in range(ROUNDS + 1):
            if k == ROUNDS:
                out["filters"] = [r.denoise_adaptive(rgb=True, var=True, **kw) for kw in AS_FILTERS]
            active = r.trace_adaptive(samples=SPP, min_samples=SPP, threshold=thr)
            counts, errors = r.read_adaptive()
            out["rounds"].append(dict(active=active, counts=counts, errors=errors, accum=r.read_accum(), rgba=r.read_rgba8()))
        r.reset()
        for n in (4, 8):
            r.frame(4).sync()
            out["uniform"][n] = dict(accum=r.read_accum(), rgba=r.read_rgba8(), denoise=r.denoise(rgb=True),
                                     plain=r.denoise(iterations=0, rgb=True),
                                     other=r.denoise(iterations=2, sigma_color=0.5, sigma_normal=0.25, sigma_plane=0.6, rgb=True))
    # every tile is sampled by the first round (below min_samples); some, but not all, have retired by round 3 (index 2)
    assert out["rounds"][0]["active"] == TX * TY
    assert 0 < out["rounds"][2]["active"] < TX * TY, out["rounds"][2]["active"]
    assert out["rounds"][2]["counts"].min() < out["rounds"][2]["counts"].max()
    return out


def ranks(pool, ps, world, band, local=True, build=True):
    """The first `world` contexts of the pool as the ranks of a new communicator, partitioned with `band`."""
    from computeraytracer_amd import Renderer
    for r in pool:
        r.sync()
    for r in pool:
        r.comm_destroy()
    cid = Renderer.comm_unique_id(local=local)
    rs = pool[:world]
    for k, r in enumerate(rs):
        r.comm_init(cid, k, world).upload(ps).comm_partition(band)
        if build:
            r.build_accel("bvh2")
    return rs


def layout_rows(n, band, world, k):
    from computeraytracer_amd import _lib
    cnt, rows = C.c_uint32(), (C.c_uint32 * max(n, 1))()
    assert _lib.load().crt_layout_rows(n, band, world, k, C.byref(cnt), rows) == 0
    return np.array(rows[: cnt.value], np.int64)


def refused(fn, code, text):
    from computeraytracer_amd._lib import CrtError
    with pytest.raises(CrtError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)


def same(got, want, what):
    """Tuples of arrays, floats by their bits."""
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        if g.dtype == np.float32:
            g, w = bits(g), bits(w)
        assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} elements differ"


def gather_all(rs):
    for r in rs:
        r.gather(rgba8=True, preview=True)


def assert_frame(rs, want, what):
    for k, r in enumerate(rs):
        same(r.read_frame_accum(), want["accum"], f"{what}, rank {k}: accumulator")
        same(r.read_frame_rgba8(), want["rgba"], f"{what}, rank {k}: rgba8")


def adaptive_round(rs, ref, k, world, band):
    thr, want = ref["threshold"], ref["rounds"][k]
    active = [r.trace_adaptive(samples=SPP, min_samples=SPP, threshold=thr) for r in rs]
    gather_all(rs)
    assert sum(active) == want["active"], (k, active)
    assert_frame(rs, want, f"round {k}")
    for j, r in enumerate(rs):
        counts, errors = r.read_frame_adaptive()
        same((counts, errors), (want["counts"], want["errors"]), f"round {k}, rank {j}: read_frame_adaptive")
        mine = layout_rows(TY, band // 8, world, j)
        assert len(mine) == (r.comm_info()["rows"] + 7) // 8
        same(r.read_adaptive(), (want["counts"][mine], want["errors"][mine]), f"round {k}, rank {j}: its own read_adaptive")


# ------------------------------------------------------------------ adaptive sampling across ranks, and its filter
@pytest.mark.parametrize("world,band", [(2, 8), (3, 8), (2, 16)])
def test_adaptive_rounds_and_filter_across_ranks(pool, ps, ref, world, band):
    rs = ranks(pool, ps, world, band)
    for k in range(ROUNDS):
        adaptive_round(rs, ref, k, world, band)
    for kw, want in zip(AS_FILTERS, ref["filters"]):
        for j, r in enumerate(rs):
            same(r.denoise_adaptive_frame(rgb=True, var=True, **kw), want, f"denoise_adaptive_frame{kw}, rank {j}")
    refused(lambda: rs[0].denoise_adaptive(), ESTATE, "row-band")           # the per-context filter still refuses
    adaptive_round(rs, ref, ROUNDS, world, band)                             # the filters only read


# ------------------------------------------------------------------ the uniform state
@pytest.mark.parametrize("band", [8, 0])
def test_denoise_frame_of_a_uniform_render(pool, ps, ref, band):
    rs = ranks(pool, ps, 2, band)
    for r in rs:
        r.frame(4)
    gather_all(rs)
    want = ref["uniform"][4]
    assert_frame(rs, want, "4 samples")
    for j, r in enumerate(rs):
        same(r.denoise_frame(rgb=True), want["denoise"], f"denoise_frame, rank {j}")
        same(r.denoise_frame(iterations=2, sigma_color=0.5, sigma_normal=0.25, sigma_plane=0.6, rgb=True), want["other"], f"other sigmas, rank {j}")
        plain = r.denoise_frame(iterations=0, rgb=True)
        same(plain, want["plain"], f"iterations 0, rank {j}")
        assert np.array_equal(plain[0], r.read_frame_rgba8())
        assert r.sample == 4
    if band:
        refused(lambda: rs[0].denoise(), ESTATE, "row-band")
    for r in rs:                                                             # the filter only read
        r.frame(4)
    gather_all(rs)
    assert_frame(rs, ref["uniform"][8], "8 samples")
    same(rs[1].denoise_frame(rgb=True), ref["uniform"][8]["denoise"], "denoise_frame at 8 samples")


# ------------------------------------------------------------------ one rank over RCCL: the all-gathers of the new planes run
def test_one_rank_over_rccl(pool, ps, ref):
    r = ranks(pool, ps, 1, 8, local=False)[0]
    try:
        assert r.comm_info()["transport"] == "rccl"
        r.frame(4).gather(rgba8=True, preview=True)
        same(r.denoise_frame(rgb=True), ref["uniform"][4]["denoise"], "denoise_frame")
        r.reset()
        adaptive_round([r], ref, 0, 1, 8)
        want = pool[1]
        want.comm_destroy().upload(ps).build_accel("bvh2")
        want.trace_adaptive(samples=SPP, min_samples=SPP, threshold=ref["threshold"])
        same(r.denoise_adaptive_frame(rgb=True, var=True), want.denoise_adaptive(rgb=True, var=True), "denoise_adaptive_frame")
    finally:
        r.sync().comm_destroy()


# ------------------------------------------------------------------ refusals
def test_trace_adaptive_needs_tile_aligned_bands(pool, ps, ref):
    for band in (0, 4):
        rs = ranks(pool, ps, 2, band)
        for r in rs:
            refused(lambda: r.trace_adaptive(samples=SPP), ESTATE, "crt_comm_partition")
            refused(lambda: r.trace_adaptive(samples=SPP), ESTATE, "multiple of 8")
    rs = ranks(pool, ps, 2, 8)
    try:
        rs[0].set_sample_offset(3)
        refused(lambda: rs[0].trace_adaptive(samples=SPP), ESTATE, "sample offset")
    finally:
        rs[0].set_sample_offset(0)
    adaptive_round(rs, ref, 0, 2, 8)


def frame_calls(r):
    return dict(denoise_frame=lambda: r.denoise_frame(), denoise_adaptive_frame=lambda: r.denoise_adaptive_frame(),
                read_frame_adaptive=lambda: r.read_frame_adaptive())


def all_refuse(r, code, text):
    for name, fn in frame_calls(r).items():
        refused(fn, code, text)


def test_frame_calls_refuse(pool, ps, ref):
    from computeraytracer_amd import Renderer
    want = ref["uniform"][4]
    # no communicator
    for r in pool:
        r.sync()
    for r in pool:
        r.comm_destroy()
    pool[0].upload(ps).build_accel("bvh2").frame(4).sync()
    all_refuse(pool[0], ESTATE, "crt_comm_init")
    # no PREVIEW gather since the partition (a plain gather of the accumulator is none); at sample 0
    rs = ranks(pool, ps, 2, 8)
    for r in rs:
        r.gather(rgba8=True, accum=True)
        all_refuse(r, ESTATE, "CRT_GATHER_PREVIEW")
    gather_all(rs)
    refused(lambda: rs[0].denoise_frame(), ESTATE, "no sample")
    # a peer that has not posted
    for r in rs:
        r.frame(4)
    rs[0].gather(rgba8=True, preview=True)
    refused(lambda: rs[0].denoise_frame(), ESTATE, "has not posted")
    rs[1].gather(rgba8=True, preview=True)
    # the recorded state is not the call's
    refused(lambda: rs[0].denoise_adaptive_frame(), ESTATE, "uniform")
    refused(lambda: rs[0].read_frame_adaptive(), ESTATE, "uniform")
    # what the per-context calls reject
    refused(lambda: rs[0].denoise_frame(iterations=11), EINVAL, "iterations")
    refused(lambda: rs[0].denoise_frame(sigma_color=0.0), EINVAL, "sigma")
    refused(lambda: rs[0].denoise_frame(sigma_plane=float("inf")), EINVAL, "sigma")
    refused(lambda: rs[0].denoise_adaptive_frame(iterations=11), EINVAL, "iterations")
    refused(lambda: rs[0].denoise_adaptive_frame(sigma_variance=-1.0), EINVAL, "sigma")
    for j, r in enumerate(rs):                                               # ... and every rank still works
        same(r.denoise_frame(rgb=True), want["denoise"], f"after the refusals, rank {j}")
    # the accumulator alone gathered again (by every rank, as every gather is)
    for r in rs:
        r.gather(rgba8=False, accum=True)
    refused(lambda: rs[0].denoise_frame(), ESTATE, "gather again")
    rs[0].gather(rgba8=True, preview=True)
    refused(lambda: rs[0].denoise_frame(), ESTATE, "has not posted")
    rs[1].gather(rgba8=True, preview=True)
    same(rs[0].denoise_frame(rgb=True), want["denoise"], "gathered again")
    # the camera set between the gather and the filter: the frame state's epoch has moved
    rs[0].set_camera(ps.camera)
    refused(lambda: rs[0].denoise_frame(), ESTATE, "gather again")
    rs[1].set_camera(ps.camera)
    for r in rs:
        r.frame(4)
    gather_all(rs)
    for j, r in enumerate(rs):
        same(r.denoise_frame(rgb=True), want["denoise"], f"after set_camera and a new gather, rank {j}")
    # a stale tree
    rs[0].update_primitives(0, ps.primitives[:1])
    all_refuse(rs[0], ESTATE, "crt_refit_accel")
    rs[0].refit_accel()
    rs[1].reset()
    for r in rs:
        r.frame(4)
    gather_all(rs)
    same(rs[0].denoise_frame(rgb=True), want["denoise"], "after the refit")
    # the adaptive state, asked for the uniform filter
    for r in rs:
        r.reset()
    adaptive_round(rs, ref, 0, 2, 8)
    refused(lambda: rs[1].denoise_frame(), ESTATE, "adaptive")
    rs[1].reset()                                                            # ... and its epoch
    refused(lambda: rs[1].read_frame_adaptive(), ESTATE, "gather again")
    refused(lambda: rs[1].denoise_adaptive_frame(), ESTATE, "gather again")
    # a stale partition: nothing is written
    rs[0].set_tile(0, 0, W, 8)
    all_refuse(rs[0], ESTATE, "crt_comm_partition")
    out = np.full((H, W, 4), 0xA5, np.uint8)
    assert rs[0]._lib.crt_denoise_adaptive_frame(rs[0]._h, None, None, out.ctypes.data, None) == ESTATE
    assert (out == 0xA5).all()
    rs = ranks(pool, ps, 2, 8)
    for k in range(2):
        adaptive_round(rs, ref, k, 2, 8)


def test_ranks_that_disagree_at_the_gather(pool, ps, ref):
    rs = ranks(pool, ps, 2, 8)
    rs[0].frame(8)
    rs[1].frame(4)
    rs[0].gather(rgba8=True, preview=True)
    refused(lambda: rs[1].gather(rgba8=True, preview=True), EINVAL, "disagree")
    refused(lambda: rs[0].denoise_frame(), ESTATE, "has not posted")
    rs[1].frame(4).gather(rgba8=True, preview=True)                          # the rank catches up and gathers again
    for j, r in enumerate(rs):
        same(r.denoise_frame(rgb=True), ref["uniform"][8]["denoise"], f"rank {j}")
    # uniform against adaptive
    for r in rs:
        r.reset()
    rs[0].frame(4).gather(rgba8=True, preview=True)
    assert rs[1].trace_adaptive(samples=SPP, min_samples=SPP, threshold=ref["threshold"]) > 0
    refused(lambda: rs[1].gather(rgba8=True, preview=True), EINVAL, "disagree")
    rs[1].reset().frame(4).gather(rgba8=True, preview=True)
    for j, r in enumerate(rs):
        same(r.denoise_frame(rgb=True), ref["uniform"][4]["denoise"], f"rank {j}")


def test_a_failed_allocation_of_the_frame_buffers(ps, ref):
    """Fresh contexts: the first frame-level call allocates the G-buffer, the colour buffers and the rgba8 (5 allocations)."""
    from computeraytracer_amd import Renderer
    cid = Renderer.comm_unique_id(local=True)
    rs = [Renderer(0) for _ in range(2)]
    try:
        for k, r in enumerate(rs):
            r.comm_init(cid, k, 2).upload(ps).comm_partition(8).build_accel("bvh2").frame(4)
        gather_all(rs)
        for k in (1, 4):
            rs[0].set_option("debug_fail_alloc", k)
            try:
                refused(lambda: rs[0].denoise_frame(), ENOMEM, "")
            finally:
                rs[0].set_option("debug_fail_alloc", 0)
        for j, r in enumerate(rs):
            same(r.denoise_frame(rgb=True), ref["uniform"][4]["denoise"], f"rank {j}")
        for r in rs:
            r.frame(4)
        gather_all(rs)
        assert_frame(rs, ref["uniform"][8], "8 samples")
    finally:
        for r in rs:
            r.sync()
        for r in rs:
            r.close()
