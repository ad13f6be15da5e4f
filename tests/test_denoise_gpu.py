"""GPU tests of the denoised preview (include/crt.h "Denoised preview", run with -m gpu on an MI355X): the G-buffer is
the oracle's first hit bit for bit, zero iterations are the plain image bit for bit, the filter is the numpy reference
of tests/denoise_ref.py, it removes noise, and it leaves the renderer's state alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as ref
from conftest import ROOT, bits
from denoise_ref import oracle_gbuffer

pytestmark = pytest.mark.gpu

NODE = shutil.which("node")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_gbuffer(g, want, hit):
    assert g.shape == want.shape
    assert np.array_equal(_u32(g[..., 7]), _u32(want[..., 7])), f"{int((_u32(g[..., 7]) != _u32(want[..., 7])).sum())} hit indices differ"
    assert 0.3 < hit.mean()
    assert np.array_equal(bits(g[hit][:, :7]), bits(want[hit][:, :7]))


def _render(r, ps, spp, mode="bvh2", tile=None):
    r.upload(ps)
    if tile is not None:
        r.set_tile(*tile)
    r.build_accel(mode).frame(spp).sync()
    return r


# ------------------------------------------------------------------ 1. the G-buffer is the oracle's first hit
def test_gbuffer_is_the_oracle_first_hit_cornell(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(256, 256)
    want, hit = oracle_gbuffer(orc, ps, (0, 0, 256, 256))
    for mode in ("none", "bvh2", "lbvh"):
        g = _render(renderer, ps, 1, mode).read_gbuffer()
        assert_gbuffer(g, want, hit)
        assert (_u32(g[~hit][:, 0]) == np.float32(2139095040.0).view(np.uint32)).all()   # t = CRT_INFINITY on a miss


def test_gbuffer_is_the_oracle_first_hit_atrium_crop(renderer, orc):
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(480, 270)
    rect = (200, 120, 64, 64)
    want, hit = oracle_gbuffer(orc, ps, rect, full_log=False)
    for mode in ("bvh2", "lbvh"):
        x0, y0, w, h = rect
        g = _render(renderer, ps, 1, mode, tile=(x0, y0, x0 + w, y0 + h)).read_gbuffer()
        assert_gbuffer(g, want, hit)


# ------------------------------------------------------------------ 2. zero iterations: the plain image, bit for bit
def _assert_k0(r):
    rgba, rgb = r.denoise(0, rgb=True)
    assert np.array_equal(rgba, r.read_rgba8())
    acc = r.read_accum()
    np.testing.assert_array_max_ulp(rgb[..., :3], ref.linear_rgb_f32(acc, r.sample), maxulp=2)


def test_zero_iterations_equal_the_framebuffer(renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scenes_synth import atrium250k
    r = _render(renderer, cornell(256, 256), 1)
    _assert_k0(r)
    r.frame(3).sync()
    assert r.sample == 4
    _assert_k0(r)
    _assert_k0(_render(renderer, atrium250k(480, 270), 2))


def test_zero_iterations_after_pipelined_frames(renderer):
    """frame(1) x 8 without a sync (batches in flight, merged into cohorts): the denoise call finishes them first."""
    from computeraytracer_amd import cornell
    renderer.upload(cornell(256, 256)).build_accel("bvh2")
    renderer.set_option("wf_defer", 1)
    for _ in range(8):
        renderer.frame(1)
    rgba = renderer.denoise(0)
    assert renderer.sample == 8
    assert np.array_equal(rgba, renderer.read_rgba8())


# ------------------------------------------------------------------ 3. the filter is the numpy reference
def _assert_filter_matches_reference(r, ps):
    acc, g = r.read_accum(), r.read_gbuffer()
    rgba, rgb = r.denoise(rgb=True)
    want = ref.atrous_gbuffer(ref.linear_rgb(acc, r.sample), g, ps.primitives)
    err = np.abs(rgb[..., :3] - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-4, f"max relative error {err.max():.3g} at {np.unravel_index(err.argmax(), err.shape)}"
    d = np.abs(rgba.astype(np.int32) - ref.to_rgba8(want).astype(np.int32))
    assert (d <= 1).all(-1).mean() >= 0.999 and d.max() <= 2
    assert (rgba[..., 3] == 255).all()


def test_filter_matches_the_reference_cornell(renderer):
    from computeraytracer_amd import cornell
    ps = cornell(256, 256)
    _assert_filter_matches_reference(_render(renderer, ps, 4), ps)


def test_filter_matches_the_reference_atrium(renderer):
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(480, 270)
    _assert_filter_matches_reference(_render(renderer, ps, 2), ps)


# ------------------------------------------------------------------ 4. it removes noise
def test_denoised_image_is_closer_to_the_converged_one(renderer):
    """Cornell 96 x 96: 4 spp denoised against 2048 spp of the same context, in display space T."""
    from computeraytracer_amd import cornell
    ps = cornell(96, 96)
    r = _render(renderer, ps, 4)
    noisy = ref.linear_rgb(r.read_accum(), 4)
    _, den = r.denoise(rgb=True)
    g = r.read_gbuffer()
    free = ref.atrous_gbuffer(noisy, g, ps.primitives, guides=False)
    r.frame(2044).sync()
    conv = ref.linear_rgb(r.read_accum(), r.sample)
    m_noisy, m_den, m_free = (ref.mse_display(x, conv) for x in (noisy, den[..., :3], free))
    print(f"MSE in T: noisy {m_noisy:.4f}, denoised {m_den:.4f}, guide-free {m_free:.4f}")
    assert m_den <= 0.35 * m_noisy
    assert m_den <= 0.75 * m_free


# ------------------------------------------------------------------ 5. state
def test_denoise_refuses_what_it_cannot_do(renderer):
    from computeraytracer_amd import cornell
    from computeraytracer_amd._lib import CrtError
    renderer.upload(cornell(64, 64)).build_accel("bvh2")
    for call in (lambda: renderer.denoise(), lambda: renderer.read_gbuffer()):
        with pytest.raises(CrtError) as e:            # sample 0
            call()
        assert e.value.code == -3
    renderer.frame(1).sync()
    for kw in (dict(iterations=11), dict(sigma_color=0.0), dict(sigma_normal=-1.0), dict(sigma_plane=float("nan")),
               dict(sigma_color=float("inf"))):
        with pytest.raises(CrtError) as e:
            renderer.denoise(**kw)
        assert e.value.code == -1, kw
    renderer.denoise(iterations=10)                    # the largest allowed
    renderer.set_row_bands(8, 2, 1).frame(1).sync()
    for call in (lambda: renderer.denoise(), lambda: renderer.read_gbuffer()):
        with pytest.raises(CrtError) as e:
            call()
        assert e.value.code == -3


def test_tile_is_filtered_on_its_own_and_gbuffer_follows_tile_and_scene(renderer, orc):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scenes_synth import mesh10k
    ps = cornell(128, 96)
    full = _render(renderer, ps, 1).read_gbuffer()
    renderer.set_tile(16, 8, 80, 72).frame(4).sync()
    g = renderer.read_gbuffer()
    assert g.shape == (64, 64, 8) and np.array_equal(bits(g), bits(full[8:72, 16:80]))
    rgba, rgb = renderer.denoise(rgb=True)
    assert rgba.shape == (64, 64, 4) and rgb.shape == (64, 64, 4)
    _assert_filter_matches_reference(renderer, ps)
    # a different scene (and size): the cached G-buffer goes with the old one
    ps2 = mesh10k(64, 48)
    g2 = _render(renderer, ps2, 1).read_gbuffer()
    want, hit = oracle_gbuffer(orc, ps2, (0, 0, 64, 48), full_log=False)
    assert_gbuffer(g2, want, hit)


def test_denoise_changes_no_renderer_state(renderer):
    from computeraytracer_amd import cornell
    renderer.upload(cornell(128, 128)).build_accel("bvh2").enable_counters(True).reset_counters()
    renderer.frame(3).sync()
    before = (renderer.read_accum(), renderer.read_rgba8(), renderer.sample, renderer.counters())
    renderer.denoise()
    renderer.denoise(0, rgb=True)
    renderer.read_gbuffer()
    after = (renderer.read_accum(), renderer.read_rgba8(), renderer.sample, renderer.counters())
    renderer.enable_counters(False)
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1])
    assert before[2:] == after[2:]
    renderer.frame(1).sync()                           # and the pass carries on from there
    assert renderer.sample == 4


# ------------------------------------------------------------------ 6. Node
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_denoise_equals_python(tmp_path, renderer):
    from computeraytracer_amd import cornell
    out = tmp_path / "dn.ppm"
    subprocess.run([NODE, os.path.join(ROOT, "host", "index.js"), "--width", "96", "--height", "72", "--spp", "4",
                    "--denoise", "5", "--out", str(out)], capture_output=True, text=True, check=True)
    rgba = _render(renderer, cornell(96, 72), 4).denoise(5)
    assert out.read_bytes() == b"P6\n96 72\n255\n" + np.ascontiguousarray(rgba[..., :3]).tobytes()
