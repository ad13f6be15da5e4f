"""CPU-only checks of crt_remove_primitives / crt_append_primitives (include/crt.h "Scene edits"): the numpy
restatement's identities, the package's helpers against it, the calls at every layer, and --blink on the command line."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import scene_topology_ref as tref
from conftest import ROOT

CALLS = ("crt_remove_primitives", "crt_append_primitives")
NODE = shutil.which("node")


def small_scene():
    """The Cornell box plus 60 triangles, with a second light record on the last sphere and one that names no primitive."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd import scene as S
    from computeraytracer_amd.scenes_synth import mesh10k
    ps = cornell(32, 24)
    tri = mesh10k(32, 24).primitives[6:66].copy()
    n0 = len(ps.primitives)
    tri["data4"][:, 3] = np.arange(n0, n0 + len(tri), dtype=np.uint32)
    prims = tref.concat(ps.primitives, tri)
    lights = tref.concat(ps.lights, prims[17:18], prims[3:4])
    lights["category"] = 0
    lights["data4"][2, 3] = 5000                                 # (upload accepts it: the kernels guard include < nprim)
    return S.PackedScene(prims, lights, ps.camera, ps.spectra, ps.cie)


RANGES = [(70, 8), (0, 2), (30, 0), (20, 3), (4, 1), (23, 5)]


def test_the_restatement_removes_renumbers_and_keeps_every_other_byte():
    ps = small_scene()
    n = len(ps.primitives)
    assert n == 78 and tref.valid(RANGES, n, ps.lights["data4"][:, 3])
    out, lights = tref.remove(ps.primitives, RANGES, ps.lights)
    gone = sorted(set(range(70, 78)) | {0, 1, 4} | set(range(20, 28)))
    keep = [i for i in range(n) if i not in gone]
    assert len(out) == n - 19 and out["data4"][:, 3].tolist() == list(range(n - 19))
    a, b = out.view(np.uint8).copy().view(out.dtype), ps.primitives.view(np.uint8).reshape(n, 80)[keep].reshape(-1).view(ps.primitives.dtype)
    a["data4"][:, 3] = b["data4"][:, 3] = 0
    assert a.tobytes() == b.tobytes()                            # every other byte, the padding words included
    assert lights["data4"][:, 3].tolist() == [2 - 2, 17 - 3, 5000]
    lights["data4"][:, 3] = ps.lights["data4"][:, 3]
    assert lights.tobytes() == ps.lights.tobytes()


def test_ranges_in_any_order_and_split_ranges_give_the_same_result():
    ps = small_scene()
    want, wl = tref.remove(ps.primitives, RANGES, ps.lights)
    rng = np.random.default_rng(1)
    for _ in range(5):
        rg = [RANGES[i] for i in rng.permutation(len(RANGES))]
        got, gl = tref.remove(ps.primitives, rg, ps.lights)
        assert got.tobytes() == want.tobytes() and gl.tobytes() == wl.tobytes()
    split = [(70, 3), (73, 5), (1, 1), (0, 1), (20, 8), (4, 1)]  # touching ranges: the same primitives
    got, gl = tref.remove(ps.primitives, split, ps.lights)
    assert got.tobytes() == want.tobytes() and gl.tobytes() == wl.tobytes()


def test_remove_then_append_of_the_tail_is_the_identity():
    ps = small_scene()
    n = len(ps.primitives)
    cut, _ = tref.remove(ps.primitives, [(n - 9, 9)], ps.lights)
    assert tref.append(cut, ps.primitives[n - 9:]).tobytes() == ps.primitives.tobytes()
    grown = tref.append(ps.primitives, _renumbered(ps.primitives[:5], n))
    back, lights = tref.remove(grown, [(n, 5)], ps.lights)
    assert back.tobytes() == ps.primitives.tobytes() and lights.tobytes() == ps.lights.tobytes()
    with pytest.raises(AssertionError):
        tref.append(ps.primitives, ps.primitives[:1])            # numbered 0, not n


def _renumbered(rec, first):
    rec = rec.copy()
    rec["data4"][:, 3] = np.arange(first, first + len(rec), dtype=np.uint32)
    return rec


def test_valid_refuses_what_the_call_refuses():
    n = 78
    light = [2, 17, 5000]
    bad = {"overlap": [(0, 10), (9, 4)], "contained": [(30, 20), (35, 1)], "twice": [(7, 1), (7, 1)], "range": [(n - 1, 2)],
           "first beyond": [(n + 1, 0)], "count wraps": [(3, 0xFFFFFFFF)], "all": [(0, 40), (40, 38)], "a light's primitive": [(16, 2)]}
    for what, rg in bad.items():
        assert not tref.valid(rg, n, light), what
    assert tref.valid([(16, 2)], n, [2]) and tref.valid([], n, light) and tref.valid([(n, 0), (0, 0)], n, light)
    assert tref.valid([(3, 14), (18, 60)], n, light)


def test_the_package_helpers_equal_the_restatement():
    from computeraytracer_amd import scene as S
    ps = small_scene()
    n = len(ps.primitives)
    want, wl = tref.remove(ps.primitives, RANGES, ps.lights)
    got = S.remove_records(ps, RANGES)
    assert got.primitives.tobytes() == want.tobytes() and got.lights.tobytes() == wl.tobytes()
    assert got.camera is ps.camera and got.spectra is ps.spectra
    assert ps.primitives["data4"][:, 3].tolist() == list(range(n))        # the input is not touched
    same = S.remove_records(ps, [(5, 0)])
    assert same.primitives.tobytes() == ps.primitives.tobytes() and same.lights.tobytes() == ps.lights.tobytes()
    for rg in ([(0, 10), (9, 4)], [(n - 1, 2)], [(3, 0xFFFFFFFF)], [(0, 40), (40, 38)], [(16, 2)], [(2, 1)]):
        assert not tref.valid(rg, n, ps.lights["data4"][:, 3])
        with pytest.raises(ValueError):
            S.remove_records(ps, rg)
    kept = S.remove_records(ps, [(2, 1)], remap_lights=False)     # the caller brings the new list
    assert kept.lights.tobytes() == ps.lights.tobytes() and len(kept.primitives) == n - 1
    rec = _renumbered(ps.primitives[10:14], n)
    more = S.append_records(ps, rec)
    assert more.primitives.tobytes() == tref.append(ps.primitives, rec).tobytes() and more.lights.tobytes() == ps.lights.tobytes()
    assert S.append_records(ps, rec[:0]).primitives.tobytes() == ps.primitives.tobytes()
    with pytest.raises(ValueError):
        S.append_records(ps, ps.primitives[10:14])
    back = S.remove_records(more, [(n, 4)])
    assert back.primitives.tobytes() == ps.primitives.tobytes() and back.lights.tobytes() == ps.lights.tobytes()


def test_header_declares_both_calls_and_every_layer_has_them():
    from test_abi import declared_symbols
    from computeraytracer_amd import Renderer, _lib
    syms = declared_symbols()
    for name in CALLS:
        assert name in syms and name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t])
    text = open(os.path.join(ROOT, "include", "crt.h")).read()
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+first\s*,\s*count\s*;\s*\}\s*crt_prim_range\s*;", text)
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+2\b", text)
    assert "Out of scope: adding or removing primitives" not in text
    assert callable(Renderer.remove_primitives) and callable(Renderer.append_primitives)


def test_the_library_exports_both_calls_and_refuses_a_null_context():
    from computeraytracer_amd import _lib
    lib = _lib.load()
    assert lib.crt_abi_version() == 2
    assert lib.crt_remove_primitives(None, None, 0, None, 0) == -1
    assert lib.crt_append_primitives(None, None, 0, None, 0) == -1


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_and_host_export_the_calls():
    addon = os.path.join(ROOT, "addon", "crt_napi.node")
    assert os.path.exists(addon), "build the addon first (__graft_entry__.build())"
    js = ("const a=require(%r);for(const n of ['removePrimitives','removePrimitivesAsync','appendPrimitives','appendPrimitivesAsync'])"
          " if(typeof a[n]!=='function') throw new Error(n);"
          "const m=require(%r);console.log(Buffer.from(m.packRanges([{first:7,count:3},[0,0],[4000000000,1]])).toString('hex'))"
          % (addon, os.path.join(ROOT, "host", "main.js")))
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == np.array([[7, 3], [0, 0], [4000000000, 1]], "<u4").tobytes().hex()


def test_blink_parses_and_refuses_what_does_not_go():
    from computeraytracer_amd.__main__ import _closing_spheres, parse_args
    a = parse_args(["--orbit", "5", "--denoise", "2", "--temporal", "--blink", "2"])
    assert a.blink == 2 and a.temporal and not a.animate and not a.animate_device
    assert parse_args(["--orbit", "5", "--denoise", "2", "--temporal", "--variance", "--blink", "1"]).blink == 1
    assert parse_args(["--orbit", "5"]).blink is None
    for bad in (["--blink", "2"], ["--orbit", "5", "--blink", "2"], ["--orbit", "5", "--denoise", "2", "--blink", "2"],
                ["--orbit", "5", "--denoise", "2", "--temporal", "--blink", "0"],
                ["--orbit", "5", "--denoise", "2", "--temporal", "--animate", "--blink", "2"],
                ["--orbit", "5", "--denoise", "2", "--temporal", "--animate-device", "--blink", "2"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
    from computeraytracer_amd import cornell
    assert _closing_spheres(cornell(8, 8)) == 2 and _closing_spheres(small_scene()) == 0
