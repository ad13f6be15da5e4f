"""CPU-only checks of adaptive sampling and the previews across a partition (include/crt.h "The frame of a partition",
DESIGN.md 6h): the calls exist at every layer, their defaults need no GPU, and the tile-row identity the PREVIEW gather
relies on holds -- the tile rows of a rank's pixel rows are that rank's rows of the tile grid."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
CALLS = ("crt_read_frame_adaptive", "crt_denoise_frame", "crt_denoise_adaptive_frame")


def test_header_declares_the_calls_and_the_library_exports_them():
    from test_abi import declared_symbols
    from computeraytracer_amd import _lib
    syms = declared_symbols()
    lib = _lib.load()
    for name in CALLS:
        assert name in syms and name in _lib.SIGNATURES and hasattr(lib, name)
    text = open(os.path.join(ROOT, "include", "crt.h")).read()
    assert re.search(r"\bCRT_GATHER_PREVIEW\s*=\s*4\b", text)
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+2\b", text) or re.search(r"CRT_ABI_VERSION\s*=\s*2\b", text)
    assert lib.crt_abi_version() == 2


def test_the_calls_refuse_a_null_context_and_the_defaults_need_no_gpu():
    from computeraytracer_amd import _lib
    lib = _lib.load()
    assert lib.crt_read_frame_adaptive(None, None, None) == -1
    assert lib.crt_denoise_frame(None, None, None, None) == -1
    assert lib.crt_denoise_adaptive_frame(None, None, None, None, None) == -1
    d = _lib.denoise_adaptive_defaults()                       # NULL params of the frame calls mean the per-context defaults
    assert (d.iterations, d.sigma_variance, d.sigma_normal) == (5, 8.0, 0.5)
    assert C.sizeof(_lib.DenoiseParams) == 16


def test_renderer_has_the_frame_calls():
    import inspect
    from computeraytracer_amd.renderer import Renderer
    for name in ("read_frame_adaptive", "denoise_frame", "denoise_adaptive_frame"):
        assert callable(getattr(Renderer, name))
    assert "preview" in inspect.signature(Renderer.gather).parameters
    assert inspect.signature(Renderer.denoise_frame).parameters["iterations"].default == 5


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_the_frame_calls():
    addon = os.path.join(ROOT, "addon", "crt_napi.node")
    assert os.path.exists(addon), "build the addon first (__graft_entry__.build())"
    js = ("const a=require(%r);for(const n of ['readFrameAdaptive','denoiseFrame','denoiseFrameAsync','denoiseAdaptiveFrame',"
          "'denoiseAdaptiveFrameAsync']) if(typeof a[n]!=='function') throw new Error(n);console.log('ok')" % addon)
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
    assert "--denoise" in open(os.path.join(ROOT, "host", "multi.js")).read()


def layout_rows(n, band, world, k):
    from computeraytracer_amd import _lib
    cnt, rows = C.c_uint32(), (C.c_uint32 * max(n, 1))()
    assert _lib.load().crt_layout_rows(n, band, world, k, C.byref(cnt), rows) == 0
    return np.array(rows[: cnt.value], np.int64)


def test_tile_rows_of_a_rank_are_its_rows_of_the_tile_grid():
    """For bands of a multiple of 8 rows: the tile rows that a rank's pixel rows fall into, in local order, are
    crt_layout_rows(ceil(H/8), band/8, ...) -- and local tile row t holds exactly the local pixel rows 8t .. 8t+7."""
    for Hh in range(1, 201):
        for band in (8, 16, 24):
            for world in range(1, 6):
                seen = []
                for k in range(world):
                    rows = layout_rows(Hh, band, world, k)
                    tiles = layout_rows((Hh + 7) // 8, band // 8, world, k)
                    assert len(tiles) == (len(rows) + 7) // 8, (Hh, band, world, k)
                    assert np.array_equal(rows // 8, np.repeat(tiles, 8)[: len(rows)]), (Hh, band, world, k)
                    # within a local tile the pixel rows are consecutive image rows from a multiple of 8 on
                    assert np.array_equal(rows % 8, np.arange(len(rows)) % 8), (Hh, band, world, k)
                    seen.extend(tiles.tolist())
                assert sorted(seen) == list(range((Hh + 7) // 8))
