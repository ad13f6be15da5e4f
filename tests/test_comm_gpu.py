"""GPU tests of the multi-GPU communicator off its straight line (include/crt.h "Multi-GPU"; run with -m gpu on
an MI355X): k_assemble element by element against tests/comm_ref.py at the shapes where its index arithmetic has edges,
ranks and tiles without pixels, stale partitions, re-partitioning, the refusals of crt_gather, crt_comm_destroy on a live
context, crt_frame_device_buffers, and the scene edits under a partition.

Everything runs on device 0 with the in-process transport, on at most 8 contexts that the module creates once and re-uses
(crt_comm_destroy, then crt_comm_init with a fresh id).  Every comparison is of bits."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libcrt is loaded: the two must share one HIP runtime for a torch stream to mean anything)

import comm_ref
import scene_transform_ref as xref
from conftest import bits
from test_scene_edit_gpu import assert_same_image, moved_cornell, options, oracle, ref_lights, rigid

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
H2D, D2H = 1, 2


# ------------------------------------------------------------------ the contexts, and the HIP runtime libcrt runs on
@pytest.fixture(scope="module")
def pool():
    from computeraytracer_amd import Renderer
    rs = [Renderer(0) for _ in range(8)]
    yield rs
    for r in rs:
        r.close()


def ranks(pool, world, init=True):
    """The first `world` contexts of the pool as the ranks of a new communicator; every context of the pool back to its
    defaults (no communicator, its own stream, the default options)."""
    from computeraytracer_amd import Renderer
    assert world <= len(pool)
    for r in pool:
        r.sync()                                               # (no copy of a peer's gather is in flight when a rank leaves)
    for r in pool:
        r.comm_destroy().set_stream(None)
        options(r)
    cid = Renderer.comm_unique_id(local=True)
    if init:
        for k, r in enumerate(pool[:world]):
            r.comm_init(cid, k, world)
    return pool[:world]


def hip():
    """hipMemcpy / hipDeviceSynchronize of the runtime libcrt itself is linked against (found through its handle)."""
    from computeraytracer_amd import _lib
    lib = _lib.load()
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipMemcpy.restype = C.c_int
    lib.hipDeviceSynchronize.argtypes = []
    lib.hipDeviceSynchronize.restype = C.c_int
    return lib


def to_device(ptr, a):
    a = np.ascontiguousarray(a)
    if a.nbytes:
        assert ptr and hip().hipMemcpy(ptr, a.ctypes.data, a.nbytes, H2D) == 0
    assert hip().hipDeviceSynchronize() == 0


def from_device(ptr, shape, dtype):
    out = np.zeros(shape, dtype)
    assert hip().hipDeviceSynchronize() == 0
    if out.nbytes:
        assert ptr and hip().hipMemcpy(out.ctypes.data, ptr, out.nbytes, D2H) == 0
    return out


def refused(fn, code, text):
    from computeraytracer_amd._lib import CrtError
    with pytest.raises(CrtError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)
    return str(e.value)


def gathered(rs, want):
    """Every rank posts both gathers; every rank then holds `want` = (accum, rgba8) of the whole frame."""
    for r in rs:
        r.gather(rgba8=True, accum=True)
    for r in rs:
        assert_same_image(r.read_frame_accum(), r.read_frame_rgba8(), *want)


def trace_and_gather(rs, want, spp=2):
    for r in rs:
        r.frame(spp)
    for r in rs:
        r.sync()
    gathered(rs, want)


# ------------------------------------------------------------------ a. k_assemble against the restatement, no rendering
SHAPES = [(1, 1, 1, 0), (1, 1, 3, 0), (1, 1, 3, 8),          # one pixel; two ranks own nothing
          (5, 2, 4, 0), (5, 3, 8, 1),                        # H < world
          (7, 5, 2, 64),                                     # band > H: rank 1 owns nothing
          (3, 17, 3, 1),                                     # band = 1
          (64, 9, 2, 8), (257, 13, 4, 5),                    # a ragged last band; W * H no multiple of 256, several blocks
          (136, 93, 3, 0), (136, 93, 8, 8),                  # the size of test_gpu_parity's gather test, at world = 8
          (1, 300, 5, 7)]                                    # W = 1


def accum_pattern(rows, W, rank):
    """uint32 lanes (global y, x, rank, a NaN whose payload is the pixel's index): a moved float is caught, not only a moved bit."""
    y, x = rows.astype(np.uint32)[:, None], np.arange(W, dtype=np.uint32)[None, :]
    a = np.empty((len(rows), W, 4), np.uint32)
    a[..., 0], a[..., 1], a[..., 2], a[..., 3] = y, x, rank, np.uint32(0x7FC00000) | (y * np.uint32(W) + x)
    return a


def rgba_pattern(rows, W, rank):
    y, x = rows.astype(np.uint32)[:, None], np.arange(W, dtype=np.uint32)[None, :]
    a = np.empty((len(rows), W, 4), np.uint8)
    a[..., 0], a[..., 1], a[..., 2], a[..., 3] = y & 255, x & 255, rank, y >> 8
    return a


def padded(a, rows_max, fill):
    out = np.full((max(rows_max, 1),) + a.shape[1:], fill, a.dtype)     # (the padding is poison: never part of a frame)
    out[: len(a)] = a
    return out


@pytest.mark.parametrize("W,H,world,band", SHAPES)
def test_assembly_is_the_layout_rule(pool, W, H, world, band):
    from computeraytracer_amd import cornell
    ps = cornell(W, H)
    rs = ranks(pool, world)
    rmax = comm_ref.rows_max(H, world, band)
    acc_strips, rgba_strips = [], []
    for k, r in enumerate(rs):
        r.upload(ps).comm_partition(band)                     # (no tree, no trace)
        rows = comm_ref.rows_of(H, world, band, k)
        assert r.comm_info() == dict(rank=k, world=world, transport="local", rows=len(rows))
        assert r.tile[2:] == (W, len(rows)) and (band or not len(rows) or r.tile[1] == rows[0])
        acc, rgba = accum_pattern(rows, W, k), rgba_pattern(rows, W, k)
        assert acc.shape == (len(rows), W, 4)
        r.write_accum(acc.view(np.float32), 0)
        to_device(r.device_buffers()[1], rgba)                # the bound strip
        acc_strips.append(padded(acc, rmax, 0xFFFFFFFF))
        rgba_strips.append(padded(rgba, rmax, 0xEE))
    want_acc = comm_ref.assemble(W, H, world, band, acc_strips)
    want_rgba = comm_ref.assemble(W, H, world, band, rgba_strips)
    # (what the pattern says by itself: lane 0 is the row, lane 1 the column, lane 2 the row's owner)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    assert np.array_equal(want_acc[..., 0], yy) and np.array_equal(want_acc[..., 1], xx)
    assert np.array_equal(want_acc[..., 2], np.repeat(np.uint32([p for p, _ in comm_ref.owners(H, world, band)]), W).reshape(H, W))
    for r in rs:
        r.gather(rgba8=True, accum=True)
    for k, r in enumerate(rs):
        acc, rgba = r.read_frame_accum(), r.read_frame_rgba8()
        assert acc.shape == (H, W, 4) and rgba.shape == (H, W, 4)
        bad = (bits(acc) != want_acc).any(-1)
        assert not bad.any(), f"rank {k}: {int(bad.sum())} accumulator elements misplaced, first at (x, y) = {np.argwhere(bad)[0][::-1]}"
        assert np.array_equal(rgba, want_rgba), f"rank {k}: {int((rgba != want_rgba).any(-1).sum())} rgba8 elements misplaced"


# ------------------------------------------------------------------ b. ranks and tiles without pixels do trace
@pytest.mark.parametrize("pipeline", [1, 0])
@pytest.mark.parametrize("W,H,world,band", [(5, 2, 4, 0), (7, 5, 2, 64)])
def test_ranks_without_rows_trace_and_gather(pool, orc, W, H, world, band, pipeline):
    from computeraytracer_amd import cornell
    ps = cornell(W, H)
    rs = ranks(pool, world)
    for r in rs:
        r.set_option("pipeline", pipeline)
        r.upload(ps).comm_partition(band).build_accel("bvh2")
    assert sorted(r.comm_info()["rows"] for r in rs)[0] == 0   # (that is what the shape is for)
    for r in rs:
        r.frame(2).sync()
        assert r.sample == 2
    gathered(rs, oracle(orc, ps, 2))


@pytest.mark.parametrize("pipeline", [1, 0])
def test_an_empty_tile_traces(pool, orc, pipeline):
    from computeraytracer_amd import cornell
    W, H = 7, 5
    ps = cornell(W, H)
    r = ranks(pool, 1, init=False)[0]
    r.set_option("pipeline", pipeline)
    r.upload(ps).set_tile(0, 3, W, 3).build_accel("bvh2")
    r.frame(2).sync()
    assert r.sample == 2 and r.tile == (0, 3, W, 0)
    assert r.read_accum().shape == (0, W, 4) and r.read_rgba8().shape == (0, W, 4)
    r.set_tile(0, 0, W, H).frame(2).sync()                     # ... and left nothing behind
    assert_same_image(r.read_accum(), r.read_rgba8(), *oracle(orc, ps, 2))


# ------------------------------------------------------------------ c. stale partitions
STALE = {"upload-smaller": lambda r, cornell: r.upload(cornell(32, 24)),
         "upload-larger": lambda r, cornell: r.upload(cornell(96, 64)),
         "set_tile": lambda r, cornell: r.set_tile(0, 0, 64, 8),
         "set_row_bands": lambda r, cornell: r.set_row_bands(8, 2, 0)}
SENTINEL = 0xA5


def raw_read_frame(r, accum, n_px):
    """crt_read_frame_* into a sentinel-filled array of n_px pixels: (return code, message, the array as bytes)."""
    out = np.full(n_px * (16 if accum else 4), SENTINEL, np.uint8)
    rc = (r._lib.crt_read_frame_accum if accum else r._lib.crt_read_frame_rgba8)(r._h, out.ctypes.data)
    return rc, (r._lib.crt_last_error(r._h) or b"").decode(), out


def assert_stale(r, n_px):
    refused(lambda: r.gather(rgba8=True, accum=True), ESTATE, "crt_comm_partition")
    refused(lambda: r.frame_device_buffers(), ESTATE, "crt_comm_partition")
    for accum in (True, False):
        rc, msg, out = raw_read_frame(r, accum, n_px)
        assert rc == ESTATE and "crt_comm_partition" in msg, (rc, msg)
        assert (out == SENTINEL).all(), "a refused crt_read_frame wrote to out"


@pytest.mark.parametrize("how", list(STALE))
def test_a_stale_partition_is_refused_until_partitioned_again(pool, orc, how):
    from computeraytracer_amd import cornell
    ps, small = cornell(64, 48), cornell(32, 24)
    rs = ranks(pool, 2)
    for r in rs:
        r.upload(ps).comm_partition(8).build_accel("bvh2")
    trace_and_gather(rs, oracle(orc, ps, 2))
    STALE[how](rs[0], cornell)
    assert_stale(rs[0], 96 * 64)                               # (the larger of every old and new frame of the cases)
    assert rs[0].comm_info() == dict(rank=0, world=2, transport="local", rows=24)     # crt_comm_info keeps answering
    if how == "set_tile":                                      # a stale partition is none for crt_trace_adaptive
        assert rs[0].trace_adaptive(samples=1, min_samples=1) > 0
        rs[0].reset()
    # rank 1 is still current: it may post, but the frame of that gather never comes
    rs[1].gather(rgba8=True, accum=True).sync()
    for accum in (True, False):
        rc, msg, out = raw_read_frame(rs[1], accum, 64 * 48)
        assert rc == ESTATE and ("has not posted" in msg or "crt_comm_partition" in msg), (rc, msg)
        assert (out == SENTINEL).all()
    assert_stale(rs[0], 96 * 64)                               # (a peer's gather does not freshen it)
    # a fresh crt_comm_partition makes everything work again
    for r in rs:
        r.upload(small).comm_partition(8).build_accel("bvh2")
        assert r.image_size == (32, 24)
    trace_and_gather(rs, oracle(orc, small, 2))


def test_binding_other_outputs_makes_the_partition_stale(pool, orc):
    from computeraytracer_amd import cornell
    ps = cornell(64, 48)
    rs = ranks(pool, 2)
    for r in rs:
        r.upload(ps).comm_partition(8).build_accel("bvh2")
    strips = rs[0].device_buffers()
    rs[0].bind_output(None, None)                              # the context's own buffers
    assert rs[0].device_buffers() != strips
    assert_stale(rs[0], 64 * 48)
    rs[0].bind_output(*strips)                                 # the strips again (they live until the next partition)
    trace_and_gather(rs, oracle(orc, ps, 2))
    rs[0].bind_output(None, None).comm_destroy()               # destroying a stale communicator leaves the context usable
    rs[0].reset().frame(2).sync()
    rows = comm_ref.rows_of(48, 2, 8, 0)
    assert_same_image(rs[0].read_accum(), rs[0].read_rgba8(), *(a[rows] for a in oracle(orc, ps, 2)))


# ------------------------------------------------------------------ d. re-partition, refusals, destroy
def test_partition_again_with_another_band(pool, orc):
    from computeraytracer_amd import cornell
    ps = cornell(64, 48)
    rs = ranks(pool, 2)
    for r in rs:
        r.upload(ps).comm_partition(8).build_accel("bvh2")
    trace_and_gather(rs, oracle(orc, ps, 2))
    for r in rs:
        r.comm_partition(0)                                    # no new upload; the tree stays
        assert r.sample == 0 and r.comm_info()["rows"] == 24
    assert rs[0].tile == (0, 0, 64, 24) and rs[1].tile == (0, 24, 64, 24)
    for r in rs:                                               # the gather counters start again
        refused(lambda: r.read_frame_rgba8(), ESTATE, "no crt_gather")
        refused(lambda: r.read_frame_accum(), ESTATE, "no crt_gather")
    trace_and_gather(rs, oracle(orc, ps, 3), spp=3)


def test_gather_refusals(pool, orc):
    from computeraytracer_amd import cornell
    ps = cornell(64, 48)
    rs = ranks(pool, 2)
    for r in rs:
        r.upload(ps)
    rs[0].comm_partition(4)
    refused(lambda: rs[0].gather(), ESTATE, "every rank")       # rank 1 has not partitioned
    refused(lambda: rs[1].gather(), ESTATE, "crt_comm_partition")
    rs[1].comm_partition(8)
    assert rs[0].comm_info()["rows"] == rs[1].comm_info()["rows"] == 24   # (equal strips: only the band differs)
    for r in rs:
        refused(lambda: r.gather(), EINVAL, "disagree about the partition")
    refused(lambda: rs[0].gather(rgba8=False, accum=False), EINVAL, "nothing to gather")
    refused(lambda: rs[0].comm_partition(65537), EINVAL, "band_rows")
    assert rs[0].comm_info()["rows"] == 24                     # (the refused call changed nothing)
    rs[0].comm_partition(8)
    for r in rs:
        r.build_accel("bvh2")
    trace_and_gather(rs, oracle(orc, ps, 2))
    rs[1].comm_destroy()
    refused(lambda: rs[0].gather(), ESTATE, "every rank")       # the peer has left


def test_comm_destroy_on_a_context_that_has_traced(pool, orc):
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(64, 48)
    want = oracle(orc, ps, 2)
    rs = ranks(pool, 2)
    for r in rs:
        r.upload(ps).comm_partition(8).build_accel("bvh2")
    trace_and_gather(rs, want)
    r = rs[0]
    r.comm_destroy()
    assert r.comm_info() == dict(rank=0, world=1, transport=None, rows=0)
    rows = comm_ref.rows_of(48, 2, 8, 0)
    r.reset().frame(2).sync()                                  # its own rows, into its own buffers
    assert r.tile == (0, 0, 64, len(rows))
    assert_same_image(r.read_accum(), r.read_rgba8(), want[0][rows], want[1][rows])
    refused(lambda: r.gather(), ESTATE, "crt_comm_init")
    r.comm_init(Renderer.comm_unique_id(local=True), 0, 1).comm_partition(0)
    trace_and_gather([r], want)


def test_frame_device_buffers_hold_the_assembled_frame(pool, orc):
    from computeraytracer_amd import cornell
    W, H = 64, 48
    ps = cornell(W, H)
    rs = ranks(pool, 2)
    for r in rs:
        r.upload(ps).comm_partition(8).build_accel("bvh2")
        a, g = r.frame_device_buffers()                        # before any gather: zeros
        assert not from_device(a, (H, W, 4), np.uint32).any() and not from_device(g, (H, W, 4), np.uint8).any()
    for r in rs:
        r.frame(2).sync().gather(rgba8=True, accum=False)
    for r in rs:
        a, g = r.frame_device_buffers()
        assert not from_device(a, (H, W, 4), np.uint32).any()   # (no gather of that buffer yet)
        assert np.array_equal(from_device(g, (H, W, 4), np.uint8), oracle(orc, ps, 2)[1])
        assert np.array_equal(from_device(g, (H, W, 4), np.uint8), r.read_frame_rgba8())
    for r in rs:
        r.gather(rgba8=False, accum=True)
    for r in rs:
        a, g = r.frame_device_buffers()
        assert np.array_equal(from_device(a, (H, W, 4), np.uint32), bits(r.read_frame_accum()))
        assert np.array_equal(from_device(g, (H, W, 4), np.uint8), r.read_frame_rgba8())
        assert_same_image(from_device(a, (H, W, 4), np.float32), from_device(g, (H, W, 4), np.uint8), *oracle(orc, ps, 2))


def test_stream_first_then_communicator(pool, orc):
    """The order of the benchmark: crt_set_stream, crt_comm_init, crt_upload_scene, crt_comm_partition -- two ranks on one
    torch stream, gathers in the middle of the run."""
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(64, 48)
    rs = ranks(pool, 2, init=False)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    cid = Renderer.comm_unique_id(local=True)
    try:
        for k, r in enumerate(rs):
            r.set_stream(stream.cuda_stream).comm_init(cid, k, 2).upload(ps).comm_partition(8).build_accel("bvh2")
        for i in range(3):
            for r in rs:
                r.frame(1)
                if i > 0:
                    r.gather(rgba8=True)
        for r in rs:
            r.sync()
        gathered(rs, oracle(orc, ps, 3))
    finally:
        for r in rs:
            r.comm_destroy().set_stream(None)
        torch.cuda.synchronize()


# ------------------------------------------------------------------ e. scene edits under a partition
def spheres_moved(ps):
    """Both spheres moved by update_primitives; the light patch stays, so the light records do."""
    from computeraytracer_amd.scene import transform_records
    prims = ps.primitives.copy()
    sph = np.flatnonzero(prims["category"] == 1)
    prims[sph[:1]] = transform_records(prims[sph[:1]], np.eye(3), [40.0, 0.0, -25.0])
    prims[sph[1:]] = transform_records(prims[sph[1:]], np.eye(3), [30.0, 20.0, 10.0], 0.8)
    assert ref_lights(prims).tobytes() == ps.lights.tobytes()
    return prims


def sphere_ops(ps):
    rng = np.random.default_rng(11)
    sph = np.flatnonzero(ps.primitives["category"] == 1)
    return [(int(i), 1, xref.matrix(*rigid(rng, 0.5))) for i in sph]


def with_scene(ps, prims=None, lights=None):
    from computeraytracer_amd.scene import PackedScene
    return PackedScene(ps.primitives if prims is None else prims, ps.lights if lights is None else lights, ps.camera, ps.spectra, ps.cie)


def edit_update(r, ps):
    r.update_primitives(0, spheres_moved(ps)).refit_accel()
    return with_scene(ps, prims=spheres_moved(ps))


def edit_transform(r, ps):
    r.transform_primitives(sphere_ops(ps)).refit_accel()
    return with_scene(ps, prims=xref.apply(ps.primitives, sphere_ops(ps)))


def edit_lights(r, ps):
    lights = ref_lights(moved_cornell(ps)[0])                   # the light records of a moved patch (the patch itself stays)
    assert lights.tobytes() != ps.lights.tobytes()
    r.update_lights(0, lights)
    return with_scene(ps, lights=lights)


def edit_reset(r, ps):
    r.reset()
    return ps


EDITS = {"update_primitives": edit_update, "transform_primitives": edit_transform, "update_lights": edit_lights, "reset": edit_reset}


def partitioned_pair(pool, ps):
    rs = ranks(pool, 2)
    for r in rs:
        r.upload(ps).comm_partition(8).build_accel("bvh2")
    return rs


@pytest.mark.parametrize("edit", list(EDITS))
def test_partitioned_ranks_edit_the_scene(pool, orc, edit):
    from computeraytracer_amd import cornell
    ps = cornell(72, 61)
    rs = partitioned_pair(pool, ps)
    for r in rs:
        r.frame(2)                                             # in flight
    for r in rs:
        ed = EDITS[edit](r, ps)
        assert r.sample == 0
    for r in rs:
        r.frame(3).sync().gather(rgba8=True, accum=True)
    for r in rs:
        assert_same_image(r.read_frame_accum(), r.read_frame_rgba8(), *oracle(orc, ed, 3))


def test_partitioned_ranks_resume_from_a_saved_strip(pool, orc):
    from computeraytracer_amd import cornell
    ps = cornell(72, 61)
    rs = partitioned_pair(pool, ps)
    saved = [r.frame(2).sync().read_accum() for r in rs]       # the checkpoint: each rank's strip after 2 samples
    for r in rs:
        r.frame(2)                                             # in flight
    for r, strip in zip(rs, saved):
        assert strip.shape == (r.comm_info()["rows"], 72, 4)
        r.write_accum(strip, 2)
        assert r.sample == 2
    for r in rs:
        r.frame(1).sync().gather(rgba8=True, accum=True)
    for r in rs:
        assert_same_image(r.read_frame_accum(), r.read_frame_rgba8(), *oracle(orc, ps, 3))


def test_partitioned_ranks_set_a_sample_offset(pool, orc):
    from computeraytracer_amd import cornell
    ps = cornell(72, 61)
    sc = orc.Scene.from_packed(ps)
    rs = partitioned_pair(pool, ps)
    g = pool[2].upload(ps).build_accel("bvh2").frame(1).sync().read_gbuffer()
    want_acc = sc.render(3, first_sample=6)[0]                 # the oracle's samples 6 .. 8
    want_rgba = sc.denoise(want_acc, 3, g, iterations=0)[1]     # ... tone-mapped with 3 (test_sample_offset_gpu._want)
    try:
        for r in rs:
            r.frame(2)                                         # in flight
        for r in rs:
            r.reset().set_sample_offset(5)
        for r in rs:
            r.frame(3).sync().gather(rgba8=True, accum=True)
            assert r.sample == 3 and r.sample_offset == 5
        for r in rs:
            assert_same_image(r.read_frame_accum(), r.read_frame_rgba8(), want_acc, want_rgba)
    finally:
        for r in rs:
            r.reset().set_sample_offset(0)


def test_denoise_under_a_partition(pool, orc):
    from computeraytracer_amd import cornell
    W, H = 72, 61
    ps = cornell(W, H)
    rs = partitioned_pair(pool, ps)
    for r in rs:
        r.frame(4).sync()
        refused(lambda: r.denoise(), ESTATE, "")               # row bands: local neighbours are no image neighbours
    other = pool[2]
    for k, r in enumerate(rs):
        r.comm_partition(0).frame(4).sync()
        rows = comm_ref.rows_of(H, 2, 0, k)
        assert r.tile == (0, int(rows[0]), W, len(rows))
        other.upload(ps).set_tile(0, int(rows[0]), W, int(rows[-1]) + 1).build_accel("bvh2").frame(4).sync()
        rgba, lin = r.denoise(rgb=True)
        rgba_o, lin_o = other.denoise(rgb=True)
        assert rgba.shape == (len(rows), W, 4)
        assert np.array_equal(rgba, rgba_o) and np.array_equal(bits(lin), bits(lin_o))
