"""CPU-only checks of the denoised preview (include/crt.h "Denoised preview"): the interfaces exist at every layer, and
the numpy reference of the filter (tests/denoise_ref.py) has the properties DESIGN.md states."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as ref
from conftest import ROOT

NODE = shutil.which("node")


def test_header_declares_and_library_exports_the_denoise_calls():
    from test_abi import declared_symbols
    from computeraytracer_amd import _lib
    syms = declared_symbols()
    assert "crt_denoise" in syms and "crt_read_gbuffer" in syms
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "crt_denoise") and hasattr(lib, "crt_read_gbuffer")
    assert "crt_denoise" in _lib.SIGNATURES and "crt_read_gbuffer" in _lib.SIGNATURES
    assert C.sizeof(_lib.DenoiseParams) == 16


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_denoise_and_read_gbuffer():
    addon = os.path.join(ROOT, "addon", "crt_napi.node")
    assert os.path.exists(addon), "build the addon first (__graft_entry__.build())"
    js = ("const a=require(%r);for(const n of ['denoise','readGbuffer']) if(typeof a[n]!=='function') throw new Error(n);"
          "console.log('ok')" % addon)
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_renderer_has_denoise_and_read_gbuffer():
    from computeraytracer_amd.renderer import Renderer
    assert callable(Renderer.denoise) and callable(Renderer.read_gbuffer)


def _planes(h, w, depth, key, normal=(0.0, 0.0, 1.0)):
    """Pixels on planes z = depth[y, x], 0.01 apart in x and y, all facing `normal`."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    pos = np.stack([xx * 0.01, yy * 0.01, np.asarray(depth, np.float64)], -1)
    nrm = np.broadcast_to(np.asarray(normal, np.float64), (h, w, 3))
    return pos, nrm, np.asarray(key, np.uint64)


def test_reference_zero_iterations_is_the_identity():
    rng = np.random.default_rng(1)
    c = rng.uniform(0, 3, (12, 17, 3))
    pos, nrm, key = _planes(12, 17, rng.uniform(1, 2, (12, 17)), rng.integers(0, 3, (12, 17)))
    assert np.array_equal(ref.atrous(c, pos, nrm, key, iterations=0), c)


def test_reference_constant_image_is_invariant():
    rng = np.random.default_rng(2)
    h, w = 40, 33
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    pos = rng.uniform(-5, 5, (h, w, 3))
    key = rng.integers(0, 4, (h, w)).astype(np.uint64)
    key[::5, ::3] = ref.MISS
    c = np.broadcast_to(np.float64([0.3, 1.7, 0.05]), (h, w, 3))
    for guides in (True, False):
        out = ref.atrous(c, pos, n, key, iterations=6, guides=guides)
        np.testing.assert_allclose(out, c, rtol=1e-12, atol=0)


def test_reference_keys_separate_coplanar_halves():
    h, w = 24, 40
    key = np.where(np.arange(w)[None, :] < 20, 1, 2) * np.ones((h, 1), np.int64)
    pos, nrm, key = _planes(h, w, np.ones((h, w)), key)
    c = np.where(key[..., None] == 1, 0.2, 0.3) * np.ones(3)
    out = ref.atrous(c, pos, nrm, key, iterations=5)
    np.testing.assert_allclose(out, c, rtol=1e-12, atol=0)     # nothing crosses the key boundary
    blurred = ref.atrous(c, pos, nrm, key, iterations=5, guides=False)
    assert np.abs(blurred - c).max() > 0.02                     # (it would without the keys)


def test_reference_plane_weight_keeps_a_depth_step_the_guide_free_filter_blurs():
    """Two parallel planes, z = 1 and z = 2, one key, one normal: the step in colour at the step in depth survives the
    guided filter; the guide-free filter with the same sigma_color smears it."""
    h, w = 24, 40
    left = np.arange(w)[None, :] < 20
    pos, nrm, key = _planes(h, w, np.where(left, 1.0, 2.0) * np.ones((h, 1)), np.zeros((h, w), np.int64))
    c = np.where(left[..., None], 0.2, 0.3) * np.ones((h, 1, 3))
    guided = ref.atrous(c, pos, nrm, key, iterations=5)
    free = ref.atrous(c, pos, nrm, key, iterations=5, guides=False)
    err_g, err_f = np.abs(guided - c).max(), np.abs(free - c).max()
    assert err_f > 0.03
    assert err_g < 0.15 * err_f
    # and on one plane the guided filter does smooth: noise on a single plane is reduced
    rng = np.random.default_rng(3)
    noisy = 0.5 + rng.normal(0, 0.1, (h, w, 3))
    flat, _, _ = _planes(h, w, np.ones((h, w)), np.zeros((h, w)))
    assert ref.atrous(noisy, flat, nrm, key, iterations=5).std() < 0.3 * noisy.std()


def test_reference_skips_non_finite_taps():
    h, w = 9, 9
    pos, nrm, key = _planes(h, w, np.ones((h, w)), np.zeros((h, w)))
    c = np.full((h, w, 3), 0.4)
    c[4, 4] = np.nan
    out = ref.atrous(c, pos, nrm, key, iterations=2)
    fin = np.ones((h, w), bool)
    fin[4, 4] = False
    np.testing.assert_allclose(out[fin], 0.4, rtol=1e-12)        # the NaN reaches no neighbour
    assert np.isnan(out[4, 4]).all()                              # (its own centre tap always counts)


def test_reference_colour_tail_matches_the_float32_restatement():
    """to_rgba8 is tonemap_rgba8's tail: linear rgb of 0 is black, large values saturate, the G channel's linear
    segment is t * 12.92 * t (Q10)."""
    c = np.float64([[[0.0, 0.0, 0.0], [50.0, 50.0, 50.0], [0.0005, 0.0005, 0.0005]]])
    rgba = ref.to_rgba8(c)
    assert rgba[0, 0].tolist() == [0, 0, 0, 255] and rgba[0, 1].tolist() == [255, 255, 255, 255]
    t = 1 - np.exp(-0.0005 * 2.2)
    assert rgba[0, 2, 0] == int(np.floor(t * 12.92 * 255 + 0.5)) and rgba[0, 2, 1] == int(np.floor(t * 12.92 * t * 255 + 0.5))
