"""GPU tests of the variance-guided preview filter (include/crt.h "Denoised preview of an adaptive render", DESIGN.md 6d;
run with -m gpu on an MI355X): zero iterations are the framebuffer and the oracle's variance bit for bit, the filter is
the float64 restatement of tests/denoise_adaptive_ref.py, it beats the plain filter on the product's own adaptive
render, and it leaves the adaptive state alone."""
import numpy as np
import pytest

import adaptive_ref as aref
import denoise_adaptive_ref as vref
import denoise_ref as ref
from conftest import bits
from test_adaptive_gpu import FORMS, _truth, options, run_rounds

pytestmark = pytest.mark.gpu
F = np.float32


def _gbuffer(r, ps, mode="bvh2", tile=None):
    """Upload, build, and the G-buffer of the rectangle (it needs one uniform sample; the reset returns to sample 0,
    where adaptive sampling starts)."""
    r.upload(ps)
    if tile is not None:
        r.set_tile(*tile)
    r.build_accel(mode).frame(1).sync()
    g = r.read_gbuffer()
    r.reset()
    return g


def _two_rounds(r, samples):
    """`samples` everywhere, then `samples` more for the tiles above the median error: mixed counts."""
    r.trace_adaptive(samples=samples, threshold=1e30, min_samples=samples, max_samples=0)
    _, errors = r.read_adaptive()
    thr = float(np.median(errors[np.isfinite(errors)]))
    n = r.trace_adaptive(samples=samples, threshold=thr, min_samples=samples, max_samples=0)
    counts, _ = r.read_adaptive()
    assert 0 < n < counts.size and len(np.unique(counts)) == 2
    return counts


# ------------------------------------------------------------------ 4. zero iterations
def test_zero_iterations_are_the_framebuffer_and_the_oracle_variance(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(100, 76)                                     # ragged tiles on both edges
    truth = _truth(orc, ps)
    try:
        renderer.upload(ps).build_accel("bvh2")
        counts, _ = run_rounds(renderer, truth, 8, 8, 40, 6)
        assert len(np.unique(counts)) >= 3
        rgba, rgb, var = renderer.denoise_adaptive(0, rgb=True, var=True)
        assert np.array_equal(rgba, renderer.read_rgba8())
        npx = aref.pixel_counts(counts, 76, 100)
        np.testing.assert_array_max_ulp(rgb[..., :3], vref.linear_rgb_f32(renderer.read_accum(), npx), maxulp=2)
        want = vref.variance(*truth.sums(counts), npx, truth.exp_)
        assert np.array_equal(bits(var), bits(want)), f"{int((bits(var) != bits(want)).sum())} variances differ from the oracle's"
        assert np.array_equal(bits(rgb[..., 3]), bits(var))
        assert np.isfinite(var).all() and (var >= 0).all() and (var > 0).mean() > 0.5
    finally:
        renderer.reset()


def test_variance_is_one_below_two_samples(renderer):
    from computeraytracer_amd import cornell
    try:
        renderer.upload(cornell(64, 48)).build_accel("bvh2")
        renderer.trace_adaptive(samples=1, threshold=1e30, min_samples=1, max_samples=1)
        rgba, var = renderer.denoise_adaptive(0, var=True)
        assert (var == 1.0).all() and np.array_equal(rgba, renderer.read_rgba8())
        rgba5, var5 = renderer.denoise_adaptive(var=True)      # and the filter runs on it
        assert np.isfinite(var5).all() and (var5 <= 1.0).all() and var5.mean() < 0.5 and (rgba5[..., 3] == 255).all()
    finally:
        renderer.reset()


# ------------------------------------------------------------------ 5. the filter is the float64 restatement
def _assert_filter_matches_reference(r, ps, g, counts, **params):
    th, tw = g.shape[:2]
    npx = aref.pixel_counts(counts, th, tw)
    acc = r.read_accum()
    _, v0 = r.denoise_adaptive(0, var=True)
    rgba, rgb, var = r.denoise_adaptive(rgb=True, var=True, **params)
    want, want_v = vref.atrous_var_gbuffer(vref.linear_rgb(acc, npx), v0, g, ps.primitives, **params)
    err = np.abs(rgb[..., :3] - want) / np.maximum(1.0, np.abs(want))
    verr = np.abs(var - want_v) / np.maximum(want_v, vref.EPS)
    d = np.abs(rgba.astype(np.int32) - ref.to_rgba8(want).astype(np.int32))
    print(f"{tw}x{th}: colour max relative error {err.max():.3g}, variance {verr.max():.3g}, "
          f"rgba8 within 1: {(d <= 1).all(-1).mean():.5f}, max {d.max()}")
    assert err.max() <= 1e-4, f"max relative error {err.max():.3g} at {np.unravel_index(err.argmax(), err.shape)}"
    assert (d <= 1).all(-1).mean() >= 0.999 and d.max() <= 2
    assert (rgba[..., 3] == 255).all()
    assert verr.max() <= 1e-3, f"variance: max relative error {verr.max():.3g} at {np.unravel_index(verr.argmax(), verr.shape)}"
    assert np.array_equal(bits(rgb[..., 3]), bits(var))


def test_filter_matches_the_reference_cornell_mixed_counts(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(100, 76)
    try:
        g = _gbuffer(renderer, ps)
        counts, _ = run_rounds(renderer, _truth(orc, ps), 8, 8, 40, 6)
        _assert_filter_matches_reference(renderer, ps, g, counts)
        _assert_filter_matches_reference(renderer, ps, g, counts, iterations=3, sigma_variance=2.0, sigma_normal=0.25, sigma_plane=0.1)
    finally:
        renderer.reset()


def test_filter_matches_the_reference_atrium(renderer):
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(480, 270)
    try:
        g = _gbuffer(renderer, ps)
        _assert_filter_matches_reference(renderer, ps, g, _two_rounds(renderer, 4))
    finally:
        renderer.reset()


def test_tile_is_filtered_on_its_own(renderer):
    from computeraytracer_amd import cornell
    ps = cornell(128, 96)
    try:
        g = _gbuffer(renderer, ps, tile=(16, 8, 76, 62))          # 60 x 54: ragged tiles inside the rectangle
        assert g.shape == (54, 60, 8)
        counts = _two_rounds(renderer, 6)
        rgba = renderer.denoise_adaptive()
        assert rgba.shape == (54, 60, 4)
        _assert_filter_matches_reference(renderer, ps, g, counts)
    finally:
        renderer.set_tile(0, 0, 128, 96)
        renderer.reset()


# ------------------------------------------------------------------ 6. it removes noise, and more of it than the plain filter
def test_variance_guided_filter_beats_the_plain_one_on_the_adaptive_render(renderer):
    """Cornell 96 x 96: four rounds of trace_adaptive(samples=16, min_samples=16, max_samples=64, threshold = median of
    the errors after the first round); MSE in display space T against 4096 samples of the same context.  The plain
    filter is denoise_ref.atrous (6a's defaults) on the same per-tile average.  The renders are the oracle's bit for
    bit, so the ratios are those of tests/test_denoise_adaptive_cpu.py (prototype: 0.46 and 0.17); asserted: <= 0.6 x
    the plain filter and <= 0.25 x the noisy image."""
    from computeraytracer_amd import cornell
    ps = cornell(96, 96)
    try:
        g = _gbuffer(renderer, ps)
        renderer.trace_adaptive(samples=16, threshold=0.0, min_samples=16, max_samples=64)
        _, errors = renderer.read_adaptive()
        thr = float(np.median(errors))
        for _ in range(3):
            renderer.trace_adaptive(samples=16, threshold=thr, min_samples=16, max_samples=64)
        counts, _ = renderer.read_adaptive()
        assert sorted(np.unique(counts).tolist()) == [16, 32, 48, 64]
        noisy = vref.linear_rgb(renderer.read_accum(), aref.pixel_counts(counts, 96, 96))
        _, guided = renderer.denoise_adaptive(rgb=True)
        plain = ref.atrous_gbuffer(noisy, g, ps.primitives)
        renderer.reset().frame(4096).sync()
        conv = ref.linear_rgb(renderer.read_accum(), renderer.sample)
        m_noisy, m_plain, m_var = (ref.mse_display(x, conv) for x in (noisy, plain, guided[..., :3]))
        print(f"MSE in T at mean {counts.mean():.1f} spp: noisy {m_noisy:.5f}, plain {m_plain:.5f}, variance-guided {m_var:.5f}")
        assert m_var <= 0.6 * m_plain
        assert m_var <= 0.25 * m_noisy
    finally:
        renderer.reset()


# ------------------------------------------------------------------ 7. state
def test_denoise_adaptive_refuses_what_it_cannot_do():
    """Every CRT_ESTATE / CRT_EINVAL case, on a context of its own."""
    import ctypes as C
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError, DenoiseAdaptiveParams
    ps = cornell(64, 48)
    with Renderer(0) as r:
        lib, h = r._lib, r._h
        buf = np.zeros((48, 64, 4), np.uint8)

        def refused(match):
            with pytest.raises(CrtError, match=match) as e:
                r.denoise_adaptive()
            assert e.value.code == -3
        r.upload(ps)
        refused("uniform state")                               # no accel structure, and uniform
        r.build_accel("bvh2")
        refused("crt_denoise filters a uniform render")        # uniform, sample 0: the message names the other filter
        r.frame(2).sync()
        refused("uniform state")                               # a uniform render
        r.reset()
        refused("uniform state")
        assert r.trace_adaptive(samples=4, min_samples=4) > 0
        r.denoise_adaptive()
        assert lib.crt_denoise_adaptive(h, None, None, buf.ctypes.data, None) == 0          # NULL = the defaults
        assert np.array_equal(buf, r.denoise_adaptive())
        assert lib.crt_denoise_adaptive(h, None, None, None, None) == 0                     # every output may be NULL
        counts, errors = r.read_adaptive()
        acc = r.read_accum()
        for p in [DenoiseAdaptiveParams(11, 8.0, 0.5, 0.3), DenoiseAdaptiveParams(5, 0.0, 0.5, 0.3),
                  DenoiseAdaptiveParams(5, -1.0, 0.5, 0.3), DenoiseAdaptiveParams(5, float("nan"), 0.5, 0.3),
                  DenoiseAdaptiveParams(5, float("inf"), 0.5, 0.3), DenoiseAdaptiveParams(5, 8.0, 0.0, 0.3),
                  DenoiseAdaptiveParams(5, 8.0, 0.5, float("nan"))]:
            assert lib.crt_denoise_adaptive(h, C.byref(p), None, buf.ctypes.data, None) == -1
        assert np.array_equal(r.read_adaptive()[0], counts) and np.array_equal(bits(acc), bits(r.read_accum()))
        r.denoise_adaptive(iterations=10)                      # the largest allowed
        r.reset()
        refused("uniform state")                               # after crt_reset
        # a stale tree (the edit also returns to the uniform state; adaptive sampling cannot start on a stale tree)
        assert r.trace_adaptive(samples=4, min_samples=4) > 0
        r.update_primitives(0, ps.primitives[:1])
        refused(None)
        with pytest.raises(CrtError, match="refit"):
            r.trace_adaptive(samples=2)
        refused(None)
        r.refit_accel()
        # under a row-band partition: adaptive sampling works, the filter refuses (rows are not neighbours)
        r.set_row_bands(8, 2, 1)
        assert r.trace_adaptive(samples=4, min_samples=4) > 0
        refused("row-band")
        r.set_tile(0, 0, 64, 48)
        assert r.trace_adaptive(samples=4, min_samples=4) > 0
        assert r.denoise_adaptive().shape == (48, 64, 4)


@pytest.mark.parametrize("form", ["wavefront-bvh2", "accel-none"])
def test_denoise_adaptive_changes_no_state_and_the_next_round_is_exact(renderer, orc, form):
    from computeraytracer_amd import cornell
    mode, opts = FORMS[form]
    ps = cornell(100, 76)
    truth = _truth(orc, ps)
    try:
        options(renderer, **opts)
        renderer.upload(ps).build_accel(mode).enable_counters(True).reset_counters()
        counts, thr = run_rounds(renderer, truth, 8, 8, 40, 3)

        def state():
            c, e = renderer.read_adaptive()
            return renderer.read_accum(), renderer.read_rgba8(), c, e, renderer.counters()
        before = state()
        a = renderer.denoise_adaptive(rgb=True, var=True)
        renderer.denoise_adaptive(0)
        b = renderer.denoise_adaptive(rgb=True, var=True)
        after = state()
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(bits(a[1]), bits(b[1]))   # repeatable
        assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1])
        assert np.array_equal(before[2], after[2]) and np.array_equal(before[3].view(np.uint32), after[3].view(np.uint32))
        assert before[4] == after[4]
        renderer.enable_counters(False)
        # the next round continues bit for bit
        want = aref.active(counts, before[3], 8, 40, thr)
        n = renderer.trace_adaptive(samples=8, threshold=float(thr), min_samples=8, max_samples=40)
        assert n == int(want.sum()) and n > 0
        grown = counts + 8 * want.astype(np.uint32)
        assert np.array_equal(renderer.read_adaptive()[0], grown)
        truth.check(renderer, grown)
    finally:
        renderer.enable_counters(False)
        renderer.reset()
        options(renderer)
