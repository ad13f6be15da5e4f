"""GPU tests of the id mattes (include/crt.h "ID mattes"; run with -m gpu on an MI355X): crt_render_mattes is
the restatement of tests/matte_ref.py exactly -- the oracle's camera rays, the table, the overflow rule and the ranking in
plain Python -- under every tree, every source, a sample offset, a tile, the adaptive state and the scene edits; it leaves
the renderer's state alone, and the id table follows the edits.  Every plane is an integer plane: all comparisons are
array_equal."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref
import aov_ref
import matte_ref as ref
from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

NODE = shutil.which("node")
EINVAL, ESTATE, ENOMEM = -1, -3, -4
_CACHE = {}


def cornell_hits(orc, w, h, n, offset=0):
    """(scene, index (h, w, n)) of the whole Cornell box at w x h: the oracle's hit of every camera ray, computed once,
    shared, never written.  The first k samples of it are the hits of n = k."""
    from computeraytracer_amd import cornell
    key = (w, h, n, offset)
    if key not in _CACHE:
        ps = cornell(w, h)
        index, _, _ = aov_ref.camera_hits(orc, ps, (0, 0, w, h), n, offset)
        index.setflags(write=False)
        _CACHE[key] = (ps, index)
    return _CACHE[key]


def without_ids(ps):
    """The same scene with no object ids of its own: what upload leaves is crt_upload_scene's identity table."""
    from computeraytracer_amd.scene import PackedScene
    return PackedScene(ps.primitives, ps.lights, ps.camera, ps.spectra, ps.cie)


def raw(r, n, source, slots, planes_ptr):
    return r._lib.crt_render_mattes(r._h, n, source, slots, planes_ptr)


def state(r):
    """Accumulator, rgba8, sample and the counters that count what the paths did (tests/test_aov_gpu.py `state`: nodes and
    prims differ between two contexts that made the same calls)."""
    c = r.counters()
    return (r.read_accum().tobytes(), r.read_rgba8().tobytes(), r.sample, tuple((k, c[k]) for k in sorted(c) if k not in ("nodes", "prims")))


# ------------------------------------------------------------------ 1. Cornell against the oracle
def test_cornell_primitive_source_equals_the_oracle_under_every_tree(renderer, orc):
    ps, index = cornell_hits(orc, 32, 32, 17)
    want = {n: ref.mattes(index[..., :n], 8) for n in (16, 17)}  # 17: sample % 16 wraps
    assert int((ref.distinct(index) >= 3).sum()) >= 1, "no pixel sees three primitives"
    assert int(ref.tie_pixels(want[16]).sum()) >= 1, "no pixel where the id decides the order"
    for mode in ("none", "bvh2", "lbvh", "ploc"):
        renderer.upload(ps).build_accel(mode)
        for n in (16, 17):
            got = renderer.render_mattes(n, "primitive", 8)  # at sample 0: an explicit n needs nothing traced
            assert set(got) == set(ref.PLANES)
            ref.assert_planes(got, want[n], f"{mode} n = {n}")


def test_overflow_at_one_and_two_slots(renderer, orc):
    ps, index = cornell_hits(orc, 32, 32, 17)
    renderer.upload(ps).build_accel("bvh2")
    for slots in (1, 2):
        want = ref.mattes(index, slots)
        assert int((want["overflow"] > 0).sum()) >= 1, slots
        got = renderer.render_mattes(17, "primitive", slots)
        assert got["ids"].shape == (slots, 32, 32)
        ref.assert_planes(got, want, f"slots {slots}")
        ref.check_invariant(got)
        assert (got["hits"] <= 17).all()


def test_object_source_reads_the_id_table(renderer, orc):
    ps, index = cornell_hits(orc, 32, 32, 17)
    n = len(ps.primitives)
    renderer.upload(without_ids(ps)).build_accel("bvh2")
    # before any set_primitive_ids the table is the identity: the primitive source's planes
    assert np.array_equal(renderer.primitive_ids(), np.arange(n))
    ref.assert_planes(renderer.render_mattes(16, "object", 8), renderer.render_mattes(16, "primitive", 8), "identity")
    table = (1000 - np.arange(n) // 2).astype(np.uint32)
    ids = ref.hit_ids(ps, index[..., :16], ref.OBJECT, table)
    want = ref.mattes(ids, 8)
    assert int(ref.reordered_pixels(ids, 8).sum()) >= 1, "no pixel whose ranking differs from its insertion order"
    assert int(ref.tie_pixels(want).sum()) >= 1
    renderer.set_primitive_ids(0, table)
    assert np.array_equal(renderer.primitive_ids(), table) and np.array_equal(renderer.primitive_ids(3, 4), table[3:7])
    ref.assert_planes(renderer.render_mattes(16, "object", 8), want, "1000 - i // 2")
    renderer.set_primitive_ids(5, [77, 78])                  # a part of the table; the device copy follows
    table[5:7] = (77, 78)
    assert np.array_equal(renderer.primitive_ids(), table)
    ref.assert_planes(renderer.render_mattes(16, "object", 8), ref.mattes(ref.hit_ids(ps, index[..., :16], ref.OBJECT, table), 8), "edited")
    ref.assert_planes(renderer.render_mattes(16, "primitive", 8), ref.mattes(index[..., :16], 8), "primitive ignores the table")
    # a scene that carries object ids sets them on upload; a new upload without them is the identity again
    renderer.upload(ps)
    assert np.array_equal(renderer.primitive_ids(), ps.object_ids)
    renderer.set_primitive_ids(0, table).upload(without_ids(ps))
    assert np.array_equal(renderer.primitive_ids(), np.arange(n))


def test_material_source_is_the_filters_key(renderer, orc):
    ps, index = cornell_hits(orc, 32, 32, 17)
    ids = ref.hit_ids(ps, index[..., :16], ref.MATERIAL)
    assert int((ref.distinct(ids) >= 2).sum()) >= 1 and len(np.unique(ids)) >= 5
    for mode in ("none", "bvh2"):
        renderer.upload(ps).build_accel(mode)
        ref.assert_planes(renderer.render_mattes(16, "material", 8), ref.mattes(ids, 8), mode)


# ------------------------------------------------------------------ 2. consistency with the existing planes
def test_hits_plane_is_render_aovs_and_one_sample_is_the_gbuffer(renderer):
    from computeraytracer_amd import cornell
    renderer.upload(cornell(48, 32)).build_accel("bvh2")
    for n in (1, 6):
        m = renderer.render_mattes(n, "primitive", 4)
        assert np.array_equal(m["hits"], renderer.render_aovs(n, planes=("hits",))["hits"]), n
    renderer.set_sample_offset(7)
    renderer.frame(1).sync()                                 # (crt_read_gbuffer wants a sample in the accumulator)
    g = bits(renderer.read_gbuffer()[..., 7])
    got = renderer.render_mattes(1, "primitive", 2)
    hit = g != ref.MISS
    assert 0.3 < hit.mean() < 1.0
    assert np.array_equal(got["ids"][0], g)                  # a miss: 0xFFFFFFFF, the G-buffer's own word
    assert np.array_equal(got["counts"][0], hit.astype(np.uint32)) and np.array_equal(got["hits"], hit.astype(np.uint32))
    assert (got["ids"][1] == ref.MISS).all() and not got["counts"][1].any() and not got["overflow"].any()


# ------------------------------------------------------------------ 3. sample offset, rectangle, a large scene
def test_sample_offset(renderer, orc):
    ps, index = cornell_hits(orc, 48, 32, 5, offset=100)
    want = ref.mattes(index, 8)
    assert int((ref.distinct(index) >= 2).sum()) >= 1
    renderer.upload(ps).build_accel("bvh2").set_sample_offset(100)
    ref.assert_planes(renderer.render_mattes(5, "primitive", 8), want, "offset 100")
    renderer.frame(5)                                        # n = 0 under the offset: the very rays the accumulator holds
    ref.assert_planes(renderer.render_mattes(0, "primitive", 8), want, "offset 100, n = 0")


def test_tile_equals_the_crop(renderer, orc):
    ps, index = cornell_hits(orc, 32, 32, 17)
    want = ref.mattes(index, 3)
    renderer.upload(ps).build_accel("bvh2").set_tile(5, 3, 18, 14)            # 13 x 11: partial blocks on both edges
    got = renderer.render_mattes(17, "primitive", 3)
    assert got["ids"].shape == (3, 11, 13) and got["hits"].shape == (11, 13)
    ref.assert_planes(got, {p: a[..., 3:14, 5:18] for p, a in want.items()}, "tile")


def test_atrium_crop_equals_the_oracle(renderer, orc):
    from computeraytracer_amd.scenes_synth import atrium250k, atrium250k_object_ids
    ps = atrium250k(480, 270)
    table = atrium250k_object_ids()
    assert len(table) == len(ps.primitives)
    x0, y0, w, h = rect = (200, 120, 16, 16)
    index, _, _ = aov_ref.camera_hits(orc, ps, rect, 3, full_log=False)
    oid = ref.hit_ids(ps, index, ref.OBJECT, table)
    assert int((ref.distinct(oid) >= 2).sum()) >= 1 and len(np.unique(oid[oid != ref.MISS])) >= 2
    want_obj, want_prim = ref.mattes(oid, 8), ref.mattes(index, 2)
    assert int((ref.distinct(index) >= 3).sum()) >= 1 and int((want_prim["overflow"] > 0).sum()) >= 1
    for mode in ("bvh2", "lbvh"):
        renderer.upload(ps).set_tile(x0, y0, x0 + w, y0 + h).build_accel(mode).set_primitive_ids(0, table)
        ref.assert_planes(renderer.render_mattes(3, "object", 8), want_obj, mode)
        ref.assert_planes(renderer.render_mattes(3, "primitive", 2), want_prim, mode)


# ------------------------------------------------------------------ 4. state
def test_zero_means_what_the_accumulator_holds_and_nothing_changes(renderer):
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(64, 48)
    n = len(ps.primitives)
    renderer.upload(ps).build_accel("bvh2").enable_counters(True).reset_counters()
    try:
        renderer.frame(3)                                    # no sync: the call is a sync point
        held = renderer.render_mattes(0, "object", 4)
        counted = renderer.counters()
        ref.assert_planes(held, renderer.render_mattes(3, "object", 4), "n = 0 after frame(3)")
        assert held["hits"].max() == 3
        renderer.render_mattes(3, "material", 2)
        # set_primitive_ids touches nothing: not the sample count, not the accumulator, and the tree stays fresh
        accum = renderer.read_accum().tobytes()
        renderer.set_primitive_ids(0, np.arange(n)[::-1])
        assert renderer.sample == 3 and renderer.read_accum().tobytes() == accum
        flipped = renderer.render_mattes(0, "object", 4)     # (a stale tree would refuse)
        back = np.where(flipped["ids"] != ref.MISS, n - 1 - flipped["ids"], ref.MISS).astype(np.uint32)
        assert np.array_equal(np.sort(back, axis=0), np.sort(held["ids"], axis=0))    # (equal counts now rank the other way round)
        assert np.array_equal(flipped["counts"], held["counts"])
        assert renderer.counters() == counted                # every counter, nodes and prims included
        with Renderer(0) as other:                           # a context that never makes the matte calls
            other.upload(ps).build_accel("bvh2").enable_counters(True).reset_counters()
            other.frame(3).sync()
            assert state(renderer) == state(other)
            renderer.frame(2).sync()
            other.frame(2).sync()
            assert renderer.sample == 5 and state(renderer) == state(other)
    finally:
        renderer.enable_counters(False)


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
        got = renderer.render_mattes(0, "primitive", 4)
        npx = adaptive_ref.pixel_counts(counts, 64, 64)
        for n in distinct:
            explicit = renderer.render_mattes(n, "primitive", 4)               # allowed in the adaptive state
            m = npx == n
            for p in ref.PLANES:
                assert np.array_equal(got[p][..., m], explicit[p][..., m]), (n, p)
        after_counts, after_errors = renderer.read_adaptive()
        assert np.array_equal(after_counts, counts) and np.array_equal(bits(after_errors), bits(errors))
        assert (renderer.read_accum().tobytes(), renderer.read_rgba8().tobytes()) == before
        want_active = adaptive_ref.active(counts, errors, 8, 40, np.float32(thr))
        assert renderer.trace_adaptive(threshold=thr, **rule) == int(want_active.sum())        # the next round is the rule's
    finally:
        renderer.reset()


# ------------------------------------------------------------------ 5. the id table under the scene edits
def test_the_id_table_follows_the_edits(renderer):
    from computeraytracer_amd import Renderer, cornell, scene as S
    ps = cornell(40, 32)
    n = len(ps.primitives)
    assert n == 18 and ps.lights["data4"][:, 3].tolist() == [2]
    table = (500 + 3 * np.arange(n)).astype(np.uint32)
    renderer.upload(ps).build_accel("bvh2").set_primitive_ids(0, table)
    shift = [1, 0, 0, 12.5, 0, 1, 0, 20.0, 0, 0, 1, -7.25]
    renderer.transform_primitives([(n - 2, 2, shift)])
    assert np.array_equal(renderer.primitive_ids(), table)                    # a moved primitive keeps its id
    renderer.update_primitives(0, ps.primitives[0:1])
    assert np.array_equal(renderer.primitive_ids(), table)
    renderer.remove_primitives([(6, 3), (12, 1)])                             # middle ranges: the survivors keep their ids
    kept = np.delete(table, [6, 7, 8, 12])
    assert np.array_equal(renderer.primitive_ids(), kept)
    with pytest.raises(Exception):
        renderer.primitive_ids(0, n)                                          # the table ends where the scene ends
    rec = ps.primitives[6:8].copy()                                           # two of them come back, at the end
    rec["data4"][:, 3] = (n - 4, n - 3)
    renderer.append_primitives(rec)
    assert np.array_equal(renderer.primitive_ids(), np.concatenate([kept, [n - 4, n - 3]]))   # new primitives: their positions
    lib, h = renderer._lib, renderer._h
    whole = np.array([0, n], np.uint32)
    assert lib.crt_remove_primitives(h, whole.ctypes.data, 1, None, 0) == EINVAL              # a refused edit
    assert np.array_equal(renderer.primitive_ids(), np.concatenate([kept, [n - 4, n - 3]]))
    renderer.set_primitive_ids(n - 4, [9000, 9001])
    ids = renderer.primitive_ids()
    assert renderer.refit_accel() is True
    records = renderer.read_primitives()
    assert len(records) == n - 2 == len(ids)
    after = renderer.render_mattes(6, "object", 8)
    assert np.isin(after["ids"], np.concatenate([ids, [ref.MISS]])).all() and len(np.unique(after["ids"])) >= 4
    with Renderer(0) as fresh:                               # a fresh upload of the read-back records and the read-back ids
        fresh.upload(S.PackedScene(records, renderer.scene.lights, ps.camera, ps.spectra, ps.cie)).set_primitive_ids(0, ids).build_accel("bvh2")
        ref.assert_planes(after, fresh.render_mattes(6, "object", 8), "after the edits + refit_accel")


# ------------------------------------------------------------------ 6. edge cases and refusals
def test_non_finite_camera_takes_the_reference_loop(renderer):
    from computeraytracer_amd import cornell, scene as S
    c = cornell(48, 40)
    cam = c.camera.copy()
    cam[0] = np.inf
    ps = S.PackedScene(c.primitives, c.lights, cam, c.spectra, c.cie)
    brute = renderer.upload(ps).build_accel("none").render_mattes(3, "primitive", 2)
    assert (brute["hits"] == 3).all()                        # the reference loop ends on the last primitive, for every ray
    tree = renderer.upload(ps).build_accel("bvh2").render_mattes(3, "primitive", 2)
    ref.assert_planes(tree, brute, "bvh2 against none")


def test_refusals(renderer):
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError, MattePlanes
    ps = cornell(32, 24)
    n = len(ps.primitives)
    hits = np.zeros((24, 32), np.uint32)
    arg = MattePlanes(hits=hits.ctypes.data)
    ids = np.arange(n, dtype=np.uint32)
    with Renderer(0) as r:
        lib, h = r._lib, r._h
        assert raw(r, 1, 0, 8, C.byref(arg)) == ESTATE       # no scene
        assert lib.crt_set_primitive_ids(h, 0, 1, ids.ctypes.data) == ESTATE
        assert lib.crt_read_primitive_ids(h, 0, 1, ids.ctypes.data) == ESTATE
        r.upload(ps)
        assert raw(r, 1, 0, 8, C.byref(arg)) == ESTATE       # no acceleration structure
        r.build_accel("bvh2")
        assert raw(r, 1, 0, 8, None) == EINVAL               # out NULL
        for slots in (0, 17):
            assert raw(r, 1, 0, slots, C.byref(arg)) == EINVAL
        for source in (-1, 3):
            assert raw(r, 1, source, 8, C.byref(arg)) == EINVAL
        assert raw(r, 0, 0, 8, C.byref(arg)) == ESTATE       # n = 0 at sample 0: the accumulator holds nothing
        for slots in (1, 16):
            assert raw(r, 1, 0, slots, C.byref(arg)) == 0
        r.update_primitives(0, ps.primitives[0:1])
        assert raw(r, 1, 0, 8, C.byref(arg)) == ESTATE       # a stale tree
        r.refit_accel()
        assert raw(r, 1, 0, 8, C.byref(arg)) == 0
        r.set_sample_offset(0xFFFFFFF0)
        assert raw(r, 16, 0, 8, C.byref(arg)) == EINVAL      # B + n = 2^32
        assert raw(r, 15, 0, 8, C.byref(arg)) == 0           # 2^32 - 1 is a sample index
        r.set_sample_offset(0)
        # the table calls: nothing changes on a refusal
        bad = ids.copy()
        bad[3] = 0xFFFFFFFF
        r.set_primitive_ids(0, ids + 10)
        assert lib.crt_set_primitive_ids(h, 0, n, bad.ctypes.data) == EINVAL                  # the reserved id
        assert lib.crt_set_primitive_ids(h, 1, n, ids.ctypes.data) == EINVAL                  # past the scene
        assert lib.crt_set_primitive_ids(h, 0xFFFFFFFF, 2, ids.ctypes.data) == EINVAL         # first + count wraps in 32 bits
        assert lib.crt_set_primitive_ids(h, 0, 1, None) == EINVAL
        assert lib.crt_set_primitive_ids(h, n, 0, None) == 0                                  # an empty range at the end
        assert lib.crt_read_primitive_ids(h, 1, n, ids.ctypes.data) == EINVAL
        assert lib.crt_read_primitive_ids(h, 0, 1, None) == EINVAL
        assert np.array_equal(r.primitive_ids(), np.arange(n) + 10)
        r.set_row_bands(8, 2, 1)
        with pytest.raises(CrtError) as e:
            r.render_mattes(1)
        assert e.value.code == ESTATE                        # row bands


def test_a_failed_allocation_leaves_nothing_and_null_planes_are_skipped(renderer):
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError
    ps = cornell(32, 24)
    want = renderer.upload(ps).build_accel("bvh2").render_mattes(2, "object", 3)
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2").frame(2).sync()
        before = (r.read_accum().tobytes(), r.sample)
        try:
            # a plane whose pointer is NULL is not allocated: hits alone under source primitive needs one buffer
            r.set_option("debug_fail_alloc", 2)
            only = r.render_mattes(2, "primitive", 3, planes=("hits",))
            r.set_option("debug_fail_alloc", 0)
            assert list(only) == ["hits"] and np.array_equal(only["hits"], want["hits"])
            # source object, in the order ids, counts, overflow, the id table: the k-th allocation of a call fails, the
            # ones before it stay -- ids; ids ok, counts; counts ok, overflow; overflow ok, the table
            for k in (1, 2, 2, 2):
                r.set_option("debug_fail_alloc", k)
                with pytest.raises(CrtError) as e:
                    r.render_mattes(2, "object", 3)
                r.set_option("debug_fail_alloc", 0)
                assert e.value.code == ENOMEM, k
                assert (r.read_accum().tobytes(), r.sample) == before
            r.set_option("debug_fail_alloc", 1)              # the table again: the first buffer still to make
            with pytest.raises(CrtError) as e:
                r.render_mattes(2, "object", 3)
            assert e.value.code == ENOMEM
            r.set_option("debug_fail_alloc", 0)
            ref.assert_planes(r.render_mattes(2, "object", 3), want, "after the failed calls")
            r.set_option("debug_fail_alloc", 1)              # nothing is left to allocate
            ref.assert_planes(r.render_mattes(2, "object", 3), want, "with every buffer there")
        finally:
            r.set_option("debug_fail_alloc", 0)
        ref.assert_planes(r.render_mattes(0, "object", 3), want, "n = 0")
    # a NULL plane is not stored either: the others do not depend on which are asked for
    some = renderer.render_mattes(2, "object", 3, planes=("counts", "overflow"))
    assert sorted(some) == ["counts", "overflow"]
    ref.assert_planes(some, want, "two planes")


# ------------------------------------------------------------------ 7. the command line
def test_cli_writes_the_mattes(tmp_path, renderer, capsys):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.__main__ import main
    pre = str(tmp_path / "m")
    main(["--width", "48", "--height", "40", "--spp", "3", "--matte-out", pre, "--matte-slots", "4", "--out", str(tmp_path / "a.png")])
    want = renderer.upload(cornell(48, 40)).build_accel("bvh2").render_mattes(3, "object", 4)
    for p in ("ids", "counts", "overflow"):
        assert np.array_equal(np.load(f"{pre}_{p}.npy"), want[p]), p
    assert (tmp_path / "m_preview.png").read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    # with --adaptive every pixel's coverage is over its own tile's count
    pre = str(tmp_path / "ad")
    main(["--width", "48", "--height", "40", "--spp", "16", "--adaptive", "0.05", "--adaptive-step", "8", "--matte-out", pre,
          "--matte-source", "material", "--matte-slots", "3", "--out", str(tmp_path / "b.png")])
    ids, counts = np.load(pre + "_ids.npy"), np.load(pre + "_counts.npy")
    assert ids.shape == counts.shape == (3, 40, 48) and 8 <= counts.sum(0).max() <= 16
    assert (tmp_path / "ad_preview.png").exists()
    capsys.readouterr()


# ------------------------------------------------------------------ 8. Node
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_planes_equal_python(tmp_path, renderer):
    from computeraytracer_amd import cornell
    pre = tmp_path / "matte"
    subprocess.run([NODE, os.path.join(ROOT, "host", "index.js"), "--width", "48", "--height", "40", "--spp", "3",
                    "--matte-out", str(pre), "--matte-slots", "4"], capture_output=True, text=True, check=True)
    want = renderer.upload(cornell(48, 40)).build_accel("bvh2").render_mattes(3, "object", 4)
    for p in ref.PLANES:
        assert (tmp_path / f"matte_{p}.bin").read_bytes() == np.ascontiguousarray(want[p]).tobytes(), p
