"""CPU-only tests of the id mattes (include/crt.h "ID mattes"): the three symbols are declared, exported and
bound; the restatement of tests/matte_ref.py does what the definition says on hand-made hit lists; coverage and the
false-colour preview are deterministic; the command line takes the new arguments; the scenes carry object ids."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import matte_ref as ref
from conftest import ROOT

SYMBOLS = ("crt_render_mattes", "crt_set_primitive_ids", "crt_read_primitive_ids")
M = ref.MISS


def test_symbols_are_declared_exported_and_bound():
    from computeraytracer_amd import _lib
    text = open(os.path.join(ROOT, "include", "crt.h")).read()
    assert 0 < text.index("- Feature planes") < text.index("- ID mattes") < text.index("- Scene edits")
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/crt.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert "crt_matte_planes" in header
    assert re.search(r"enum\s*\{\s*CRT_MATTE_PRIMITIVE\s*=\s*0\s*,\s*CRT_MATTE_OBJECT\s*=\s*1\s*,\s*CRT_MATTE_MATERIAL\s*=\s*2\s*\}", header)
    assert re.search(r"#define\s+CRT_MATTE_MAX_SLOTS\s+16\b", header)
    assert [f[0] for f in _lib.MattePlanes._fields_] == list(ref.PLANES)
    assert C.sizeof(_lib.MattePlanes) == 4 * C.sizeof(C.c_void_p)
    from computeraytracer_amd.renderer import MATTE_SOURCES
    assert MATTE_SOURCES == {"primitive": ref.PRIMITIVE, "object": ref.OBJECT, "material": ref.MATERIAL}
    assert _lib.load().crt_abi_version() == 2


def test_null_context_is_einval():
    from computeraytracer_amd import _lib
    lib = _lib.load()
    ids = np.zeros(4, np.uint32)
    planes = _lib.MattePlanes(hits=ids.ctypes.data)
    assert lib.crt_render_mattes(None, 1, 0, 8, C.byref(planes)) == -1
    assert lib.crt_set_primitive_ids(None, 0, 4, ids.ctypes.data) == -1
    assert lib.crt_read_primitive_ids(None, 0, 4, ids.ctypes.data) == -1


# ------------------------------------------------------------------ the restatement on hand-made hit lists
def test_ref_insertion_and_ranking():
    inserted, ranked, h, over = ref.pixel([7, 3, 7, M, 9, 3, 7], 8)
    assert inserted == [(7, 3), (3, 2), (9, 1)] and ranked == inserted and (h, over) == (6, 0)
    inserted, ranked, h, over = ref.pixel([9, 3, 3, 7, 7, 7], 4)
    assert inserted == [(9, 1), (3, 2), (7, 3)] and ranked == [(7, 3), (3, 2), (9, 1)] and (h, over) == (6, 0)


def test_ref_overflow_at_one_and_two_slots():
    seq = [5, 6, 6, 6, 5, 8, M, 6]
    # one slot: the first id keeps it, however often another one comes
    assert ref.pixel(seq, 1) == ([(5, 2)], [(5, 2)], 7, 5)
    # two slots: 8 first appears after the table has filled and is counted in overflow only
    assert ref.pixel(seq, 2) == ([(5, 2), (6, 4)], [(6, 4), (5, 2)], 7, 1)
    assert ref.pixel(seq, 3) == ([(5, 2), (6, 4), (8, 1)], [(6, 4), (5, 2), (8, 1)], 7, 0)
    # without overflow the ranking does not depend on the sample order
    rng = np.random.default_rng(20261021)
    for _ in range(20):
        assert ref.pixel(rng.permutation(seq), 3)[1:] == ([(6, 4), (5, 2), (8, 1)], 7, 0)


def test_ref_equal_counts_are_ordered_by_id_unsigned():
    _, ranked, _, _ = ref.pixel([0x80000001, 4, 2, 0x80000001, 4, 2, 1], 8)
    assert ranked == [(2, 2), (4, 2), (0x80000001, 2), (1, 1)]


def test_ref_planes_all_miss_pixel_and_the_invariant():
    ids = np.array([[[M, M, M, M], [1, 2, 1, M]],
                    [[3, 3, 3, 3], [4, 5, 6, 7]]], np.uint32)
    for slots in (1, 2, 3, 16):
        p = ref.mattes(ids, slots)
        assert all(p[k].dtype == np.uint32 for k in ref.PLANES)
        assert p["ids"].shape == p["counts"].shape == (slots, 2, 2) and p["hits"].shape == p["overflow"].shape == (2, 2)
        assert (p["ids"][:, 0, 0] == M).all() and not p["counts"][:, 0, 0].any() and p["hits"][0, 0] == 0 and p["overflow"][0, 0] == 0
        assert np.array_equal(p["hits"], [[0, 3], [4, 4]])
        ref.check_invariant(p)
    assert np.array_equal(ref.mattes(ids, 2)["overflow"], [[0, 0], [0, 2]])
    assert np.array_equal(ref.mattes(ids, 2)["ids"][:, 0, 1], [1, 2]) and np.array_equal(ref.mattes(ids, 2)["counts"][:, 0, 1], [2, 1])
    assert np.array_equal(ref.mattes(ids, 3)["ids"][:, 1, 1], [4, 5, 6])
    assert np.array_equal(ref.distinct(ids), [[0, 2], [1, 4]])
    assert np.array_equal(ref.tie_pixels(ref.mattes(ids, 4)), [[False, False], [False, True]])
    # the adaptive state: each pixel its own n
    p = ref.mattes(ids, 4, n=np.array([[4, 1], [2, 3]]))
    assert np.array_equal(p["hits"], [[0, 1], [2, 3]]) and p["counts"][0, 1, 0] == 2


def test_ref_hit_ids_by_source():
    from computeraytracer_amd import cornell
    ps = cornell(8, 8)
    n = len(ps.primitives)
    index = np.array([[[0, n - 1, M]]], np.uint32)
    assert np.array_equal(ref.hit_ids(ps, index, ref.PRIMITIVE), index)
    assert np.array_equal(ref.hit_ids(ps, index, ref.OBJECT), index)
    assert np.array_equal(ref.hit_ids(ps, index, ref.OBJECT, 1000 - np.arange(n) // 2), [[[1000, 1000 - (n - 1) // 2, M]]])
    d4 = ps.primitives["data4"]
    assert np.array_equal(ref.hit_ids(ps, index, ref.MATERIAL), [[[(d4[0, 2] << 24) | d4[0, 1], (d4[n - 1, 2] << 24) | d4[n - 1, 1], M]]])


# ------------------------------------------------------------------ coverage and the preview
def _planes():
    ids = np.array([[[17, 3], [M, 9]], [[3, 17], [M, M]]], np.uint32)            # (slots 2, H 2, W 2)
    counts = np.array([[[5, 4], [0, 7]], [[2, 3], [0, 0]]], np.uint32)
    return dict(ids=ids, counts=counts, hits=counts.sum(0, dtype=np.uint32), overflow=np.zeros((2, 2), np.uint32))


def test_matte_coverage():
    from computeraytracer_amd import matte_coverage
    p = _planes()
    c = matte_coverage(p, 7, 17)
    assert c.dtype == np.float32 and c.shape == (2, 2)
    want = np.array([[5, 3], [0, 0]], np.float32) / np.float32(7)
    assert np.array_equal(c.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(matte_coverage(p, 7, 9), np.array([[0, 0], [0, 1]], np.float32))
    assert not matte_coverage(p, 7, 12345).any()
    # a per-pixel n, as in the adaptive state
    n = np.array([[8, 16], [8, 7]], np.uint32)
    want = np.array([[2, 4], [0, 0]], np.float32) / n.astype(np.float32)
    assert np.array_equal(matte_coverage(p, n, 3).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(matte_coverage(p, 7, 17), c) and p["ids"][0, 0, 0] == 17          # deterministic, input untouched


def test_id_preview_is_deterministic(tmp_path):
    from computeraytracer_amd import image
    p = _planes()
    a = image.id_preview(p, 7)
    assert a.shape == (2, 2, 4) and a.dtype == np.uint8 and (a[..., 3] == 255).all()
    assert np.array_equal(a, image.id_preview(p, 7))
    assert not a[1, 0, :3].any()                                             # no entry: black
    col = image.id_colour(np.array([17, 3, 9, 17], np.uint32))
    assert col.shape == (4, 3) and col.min() >= 64 and np.array_equal(col[0], col[3]) and not np.array_equal(col[0], col[1])
    assert np.array_equal(a[1, 1, :3], col[2])                               # full coverage: the id's own colour
    assert np.array_equal(a[0, 0, :3], image.unorm8(col[0].astype(np.float32) / np.float32(255) * (np.float32(5) / np.float32(7))))
    paths = image.write_mattes(str(tmp_path / "m"), p, 7)
    assert [os.path.basename(q) for q in paths] == ["m_ids.npy", "m_counts.npy", "m_overflow.npy", "m_preview.png"]
    assert np.array_equal(np.load(paths[0]), p["ids"]) and np.array_equal(np.load(paths[1]), p["counts"])
    assert open(paths[3], "rb").read()[:8] == b"\x89PNG\r\n\x1a\n"


# ------------------------------------------------------------------ the command line and the scenes
def test_the_new_arguments_parse():
    from computeraytracer_amd.__main__ import parse_args
    a = parse_args([])
    assert a.matte_out is None and a.matte_source == "object" and a.matte_slots == 8
    a = parse_args(["--matte-out", "m/f", "--matte-source", "material", "--matte-slots", "16", "--spp", "4"])
    assert (a.matte_out, a.matte_source, a.matte_slots) == ("m/f", "material", 16)
    a = parse_args(["--adaptive", "0.05", "--matte-out", "f", "--matte-source", "primitive"])
    assert a.adaptive == 0.05 and a.matte_out == "f" and a.matte_source == "primitive"
    for bad in (["--matte-out", "f", "--orbit", "2"], ["--matte-out", "f", "--matte-slots", "0"],
                ["--matte-out", "f", "--matte-slots", "17"], ["--matte-out", "f", "--matte-source", "colour"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2


def test_pack_scene_gives_one_id_per_object():
    from computeraytracer_amd import cornell, load_scene, pack_scene
    ps = cornell(16, 16)
    n = len(ps.primitives)
    assert ps.object_ids.dtype == np.uint32 and np.array_equal(ps.object_ids, np.arange(n))      # patches and spheres only
    assert ps.with_size(8, 8).object_ids is ps.object_ids
    # a mesh is one object: every triangle of it carries the id after the single primitives'
    sc = load_scene()
    sc = dict(sc, objects=dict(sc["objects"]))
    tri = dict(vertices=[[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], indices=[0, 1, 2, 1, 3, 2],
               emission=sc["objects"]["patches"][0]["emission"], reflectance=sc["objects"]["patches"][0]["reflectance"],
               type=sc["objects"]["patches"][0]["type"])
    sc["objects"]["meshes"] = [tri, dict(tri, indices=[0, 1, 2])]
    pm = pack_scene(sc)
    assert len(pm.primitives) == n + 3
    assert np.array_equal(pm.object_ids, list(range(n)) + [n, n, n + 1])
    from computeraytracer_amd.scene import PackedScene
    assert PackedScene(ps.primitives, ps.lights, ps.camera, ps.spectra, ps.cie).object_ids is None       # the last, optional field


def test_atrium_object_ids():
    from computeraytracer_amd.scenes_synth import atrium250k_object_ids
    ids = atrium250k_object_ids()
    assert ids.dtype == np.uint32 and ids.shape == (253958,)
    assert len(np.unique(ids)) == 71 and ids.max() == 70
    assert np.array_equal(ids[:6], np.arange(6)) and (ids[6:6 + 131072] == 6).all()
    cols = ids[6 + 131072:].reshape(64, 1920)
    assert (cols == (7 + np.arange(64))[:, None]).all()
