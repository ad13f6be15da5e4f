"""CPU-only checks of the variance-guided filter (include/crt.h "Denoised preview of an adaptive render"):
the interfaces exist at every layer, the numpy restatement (tests/denoise_adaptive_ref.py) has the properties the
definition states, and on oracle renders of an adaptive schedule it beats the plain filter by the margin measured."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref as aref
import denoise_adaptive_ref as vref
import denoise_ref as ref
from conftest import ROOT

NODE = shutil.which("node")
F = np.float32


# ------------------------------------------------------------------ 1. the interface
def test_defaults_need_no_gpu_and_header_declares_the_calls():
    from test_abi import declared_symbols
    from computeraytracer_amd import _lib
    syms = declared_symbols()
    assert "crt_denoise_adaptive" in syms and "crt_denoise_adaptive_defaults" in syms
    assert C.sizeof(_lib.DenoiseAdaptiveParams) == 16
    d = _lib.denoise_adaptive_defaults()
    assert (d.iterations, d.sigma_variance, d.sigma_normal, d.sigma_plane) == (5, 8.0, 0.5, F(0.3))
    assert _lib.load().crt_denoise_adaptive_defaults(None) == -1
    assert vref.DEFAULTS == dict(iterations=5, sigma_variance=8.0, sigma_normal=0.5, sigma_plane=0.3)


def test_renderer_has_denoise_adaptive():
    from computeraytracer_amd.renderer import Renderer
    assert callable(Renderer.denoise_adaptive)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_denoise_adaptive():
    addon = os.path.join(ROOT, "addon", "crt_napi.node")
    assert os.path.exists(addon), "build the addon first (__graft_entry__.build())"
    js = ("const a=require(%r);for(const n of ['denoiseAdaptive','denoiseAdaptiveAsync']) if(typeof a[n]!=='function') "
          "throw new Error(n);console.log('ok')" % addon)
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ------------------------------------------------------------------ 2. the restatement
def _planes(h, w, depth, key, normal=(0.0, 0.0, 1.0)):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    pos = np.stack([xx * 0.01, yy * 0.01, np.asarray(depth, np.float64)], -1)
    nrm = np.broadcast_to(np.asarray(normal, np.float64), (h, w, 3))
    return pos, nrm, np.asarray(key, np.uint64)


def test_reference_zero_iterations_is_the_identity():
    rng = np.random.default_rng(1)
    c, v = rng.uniform(0, 3, (12, 17, 3)), rng.uniform(0, 0.1, (12, 17))
    pos, nrm, key = _planes(12, 17, rng.uniform(1, 2, (12, 17)), rng.integers(0, 3, (12, 17)))
    c0, v0 = vref.atrous_var(c, v, pos, nrm, key, iterations=0)
    assert np.array_equal(c0, c) and np.array_equal(v0, v)


def test_reference_constant_image_stays_constant_and_its_variance_shrinks_by_the_kernel():
    h, w = 40, 33
    pos, nrm, key = _planes(h, w, np.ones((h, w)), np.zeros((h, w)))
    c = np.broadcast_to(np.float64([0.3, 1.7, 0.05]), (h, w, 3))
    v = np.full((h, w), 2.5e-3)
    c1, v1 = vref.atrous_var(c, v, pos, nrm, key, iterations=1)
    np.testing.assert_allclose(c1, c, rtol=1e-12, atol=0)
    np.testing.assert_allclose(v1[2:-2, 2:-2], 2.5e-3 * (70.0 / 256.0) ** 2, rtol=1e-12)
    assert (v1[[0, -1]] > v1[5, 5]).all() and (v1[:, [0, -1]] > v1[5, 5]).all()     # fewer taps at the borders
    c5, v5 = vref.atrous_var(c, v, pos, nrm, key, iterations=5)
    np.testing.assert_allclose(c5, c, rtol=1e-12, atol=0)
    assert (v5 < v1).all() and (v5 > 0).all()


def test_reference_variance_blur_stays_inside_the_key():
    key = np.zeros((6, 8), np.uint64)
    key[:, 4:] = 7
    v = np.where(key == 0, 1.0, 100.0)
    np.testing.assert_allclose(vref.blur_variance(v, key), v, rtol=1e-15)
    v = np.zeros((5, 5))
    v[2, 2] = 16.0
    want = np.zeros((5, 5))
    want[1:4, 1:4] = np.outer([1, 2, 1], [1, 2, 1])
    np.testing.assert_allclose(vref.blur_variance(v, np.zeros((5, 5), np.uint64)), want, rtol=1e-15)


def test_reference_converged_pixels_are_left_alone_and_noisy_ones_are_smoothed():
    """One plane, a step in colour: with a variance far below the step nothing crosses it (the colour term is in
    standard errors); with a variance as large as the step it is smoothed away."""
    h, w = 24, 40
    pos, nrm, key = _planes(h, w, np.ones((h, w)), np.zeros((h, w)))
    c = np.where(np.arange(w)[None, :, None] < 20, 0.2, 0.6) * np.ones((h, 1, 3))
    sharp, _ = vref.atrous_var(c, np.full((h, w), 1e-8), pos, nrm, key)
    blurred, _ = vref.atrous_var(c, np.full((h, w), 1e-1), pos, nrm, key)
    assert np.abs(sharp - c).max() < 1e-6
    assert np.abs(blurred - c).max() > 0.1


def test_reference_skips_non_finite_taps():
    h, w = 9, 9
    pos, nrm, key = _planes(h, w, np.ones((h, w)), np.zeros((h, w)))
    c = np.full((h, w, 3), 0.4)
    c[4, 4] = np.nan
    out, v = vref.atrous_var(c, np.full((h, w), 1e-3), pos, nrm, key, iterations=2)
    fin = np.ones((h, w), bool)
    fin[4, 4] = False
    np.testing.assert_allclose(out[fin], 0.4, rtol=1e-12)        # the NaN reaches no neighbour
    assert np.isnan(out[4, 4]).all()                              # (its own centre tap always counts)
    assert np.isfinite(v[fin]).all()


def test_reference_variance_is_one_where_nothing_is_known(orc):
    exp_ = lambda x: orc.math_eval("exp", np.asarray(x, F))    # noqa: E731
    S = F([[1.0, 2.0, 2.0, np.nan, 1e30]])
    Q = F([[1.0, 2.0, 3.0, 1.0, np.inf]])
    v = vref.variance(S, Q, np.uint32([[1, 2, 2, 4, 4]]), exp_)
    assert v.dtype == np.float32
    assert v[0, 0] == 1.0                                        # one sample
    assert v[0, 1] == 0.0                                        # two equal samples of 1: no spread
    e = aref.pixel_error(F([2.0]), F([3.0]), np.uint32([2]), exp_)
    assert v[0, 2] == (e * e).astype(F)[0] and v[0, 2] > 0
    assert v[0, 3] == 1.0 and v[0, 4] == 1.0                     # NaN, inf
    assert np.isfinite(v).all() and (v >= 0).all()


# ------------------------------------------------------------------ 3. quality on oracle renders
def adaptive_schedule(S, Q, exp_, first=16, step=16, rounds=3, max_samples=64):
    """`first` samples everywhere, then `rounds` rounds of `step` for the tiles above the median error of the first
    round (adaptive_ref's rule).  S, Q: (n + 1, H, W) running sums.  Returns the tile counts."""
    hh, ww = S.shape[1:]
    counts = np.full(((hh + 7) // 8, (ww + 7) // 8), first, np.uint32)
    ii, jj = np.indices((hh, ww))
    thr = None
    for _ in range(rounds):
        npx = aref.pixel_counts(counts, hh, ww)
        E = aref.tile_errors(S[npx, ii, jj], Q[npx, ii, jj], counts, exp_)
        if thr is None:
            thr = F(np.median(E))
        counts = counts + np.uint32(step) * aref.active(counts, E, first, max_samples, thr).astype(np.uint32)
    return counts


def test_variance_guided_filter_beats_the_plain_one_on_an_adaptive_oracle_render(orc):
    """Cornell 96 x 96: 16 samples everywhere, then 3 rounds of 16 for the tiles above the median error; MSE in display
    space T against 4096 oracle samples.  Measured with the float64 prototype: noisy 0.00667, plain filter 0.00242,
    variance-guided 0.00111 (ratios 0.46 and 0.17); asserted: <= 0.6 x the plain filter and <= 0.25 x the noisy image."""
    from computeraytracer_amd import cornell
    W = Hh = 96
    ps = cornell(W, Hh)
    sc = orc.Scene.from_packed(ps)
    exp_ = lambda x: orc.math_eval("exp", np.asarray(x, F))    # noqa: E731
    conv = ref.linear_rgb(sc.render(4096)[0], 4096)
    g, _ = ref.oracle_gbuffer(orc, ps, (0, 0, W, Hh))
    S, Q, A = [np.zeros((Hh, W), F)], [np.zeros((Hh, W), F)], [np.zeros((Hh, W, 4), F)]
    for s in range(1, 65):
        a = sc.render(1, first_sample=s)[0]
        s_, q_ = aref.accumulate(a[None, ..., 1], S[-1], Q[-1])
        S.append(s_)
        Q.append(q_)
        A.append((A[-1] + a).astype(F))
    S, Q, A = np.stack(S), np.stack(Q), np.stack(A)
    counts = adaptive_schedule(S, Q, exp_)
    assert sorted(np.unique(counts).tolist()) == [16, 32, 48, 64]
    npx = aref.pixel_counts(counts, Hh, W)
    ii, jj = np.indices((Hh, W))
    noisy = vref.linear_rgb(A[npx, ii, jj], npx)
    v = vref.variance(S[npx, ii, jj], Q[npx, ii, jj], npx, exp_)
    plain = ref.atrous_gbuffer(noisy, g, ps.primitives)
    guided, v_out = vref.atrous_var_gbuffer(noisy, v, g, ps.primitives)
    m_noisy, m_plain, m_var = (ref.mse_display(x, conv) for x in (noisy, plain, guided))
    print(f"MSE in T at mean {counts.mean():.1f} spp: noisy {m_noisy:.5f}, plain {m_plain:.5f}, variance-guided {m_var:.5f}; "
          f"variance in {v.mean():.3g} out {v_out.mean():.3g}")
    assert m_var <= 0.6 * m_plain
    assert m_var <= 0.25 * m_noisy
    assert v_out.mean() < v.mean()
