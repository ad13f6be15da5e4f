"""CPU-only checks of crt_denoise_svgf (include/crt.h "Variance-guided temporal filter"): the interfaces exist
at every layer, the float64 restatement (tests/denoise_svgf_ref.py) gives the moments in closed form on small cases, and on
oracle renders of three orbits the variance-guided passes beat crt_denoise_temporal's fixed-sigma passes on the same
blend."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as ref
import denoise_svgf_ref as sref
import denoise_temporal_ref as tref
from conftest import ROOT

NODE = shutil.which("node")
F = np.float32
CALLS = ("crt_denoise_svgf", "crt_denoise_svgf_defaults", "crt_debug_read_moments")

# Cornell 64 x 64; MSE in display space against 1024 spp drawn at sample index 100 001.  A is ORBIT of
# tests/test_denoise_temporal_cpu.py.  `ratio`: crt_denoise_svgf over crt_denoise_temporal on the last frame, both at their
# defaults, measured with the float64 restatements on oracle renders (DESIGN.md 6g has the table and the sweep).
SETUPS = {
    "A": dict(size=64, frames=8, spp=4, turn=64, truth_spp=1024, truth_first=100001, ratio=0.883),
    "B": dict(size=64, frames=32, spp=4, turn=256, truth_spp=1024, truth_first=100001, ratio=0.817),
    "C": dict(size=64, frames=32, spp=1, turn=256, truth_spp=1024, truth_first=100001, ratio=0.795),
}


# ------------------------------------------------------------------ 1. the interface
def test_defaults_need_no_gpu():
    from computeraytracer_amd import _lib
    assert C.sizeof(_lib.DenoiseSvgfParams) == 32
    d = _lib.denoise_svgf_defaults()
    got = {k: getattr(d, k) for k in sref.DEFAULTS}
    assert got == {k: (v if k == "iterations" else float(F(v))) for k, v in sref.DEFAULTS.items()}
    assert _lib.load().crt_denoise_svgf_defaults(None) == -1


def test_header_declares_the_calls_and_the_bindings_have_them():
    from test_abi import declared_symbols
    from computeraytracer_amd import _lib
    from computeraytracer_amd.renderer import Renderer
    syms = declared_symbols()
    for name in CALLS:
        assert name in syms and name in _lib.SIGNATURES
    for name in ("denoise_svgf", "read_moments"):
        assert callable(getattr(Renderer, name))
    assert _lib.load().crt_abi_version() == 2                   # the change is additive


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_the_calls():
    addon = os.path.join(ROOT, "addon", "crt_napi.node")
    assert os.path.exists(addon), "build the addon first (__graft_entry__.build())"
    js = ("const a=require(%r);for(const n of ['denoiseSvgfDefaults','denoiseSvgf','denoiseSvgfAsync','readMoments'])"
          " if(typeof a[n]!=='function') throw new Error(n);console.log('ok')" % addon)
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ------------------------------------------------------------------ 2. the restatement on a static plane
def plane(W=16, Hh=16):
    """An unchanged 90 degree pinhole looking at the plane z = -5: every pixel finds itself (weights 1, 0, 0, 0)."""
    frame = np.float64([-1, -1, -2, 2, 0, 0, 0, 2, 0, 0, 0, 0])
    llc, hor, ver, eye = tref.frame_parts(frame)
    yy, xx = np.mgrid[0:Hh, 0:W].astype(np.float64)
    fs, ft = (xx + 17 / 32) / W, (Hh - yy + 17 / 32) / Hh
    d = llc + hor * fs[..., None] + ver * ft[..., None] - eye
    pos = eye + d * (5.0 / -d[..., 2:3])
    nrm = np.broadcast_to(np.float64([0, 0, 1]), pos.shape)
    g = np.concatenate([np.zeros((Hh, W, 1)), pos, nrm, np.zeros((Hh, W, 1))], -1)
    return frame, g, np.zeros((Hh, W), np.uint64), W, Hh


def accum_of(y, n, shape):
    """XYZ sums of n samples whose mean luminance is y (X = Z = Y: a grey)."""
    return np.full(shape + (3,), float(y) * n)


def run_frames(values, n, key=None, **bp):
    """The plane seen in len(values) frames of n samples with mean luminance values[k]: the last frame's (c, Hw, mom)."""
    frame, g, key0, W, Hh = plane()
    key = key0 if key is None else key
    prev = None
    for y in values:
        c, hw, mom, _ = sref.blend(accum_of(y, n, (Hh, W)), n, g, key, frame, prev, W, Hh, **bp)
        prev = sref.slot(c, hw, mom, g, key, frame)
    return c, hw, mom


def test_a_constant_history_has_no_spread():
    _, hw, mom = run_frames([0.3] * 6, 4)
    np.testing.assert_allclose(mom[..., 0], 0.3, rtol=1e-12)
    assert np.abs(mom[..., 1]).max() <= 1e-30
    np.testing.assert_allclose(mom[..., 2], 24.0, rtol=1e-12)
    np.testing.assert_allclose(hw, 24.0, rtol=1e-12)
    v, known = sref.variance(mom, 4)
    assert known.all() and np.abs(v).max() <= 1e-28


def test_two_frames_give_the_closed_form():
    """Frame means a, b of n samples each: m1 = (a + b) / 2, s = (a - b)^2 / 4 (the population variance of two values),
    and with min_frames 2 v = g^2 s / (2 - 1); three frames a, b, b: the weighted variance of {a, b, b}."""
    a, b, n = 0.2, 0.5, 4
    _, _, mom = run_frames([a, b], n)
    np.testing.assert_allclose(mom[..., 0], (a + b) / 2, rtol=1e-12)
    np.testing.assert_allclose(mom[..., 1], (a - b) ** 2 / 4, rtol=1e-12)
    np.testing.assert_allclose(mom[..., 2], 2.0 * n, rtol=1e-12)
    v, known = sref.variance(mom, n, min_frames=2.0)
    g = 2.2 * np.exp(-2.2 * (a + b) / 2)
    assert known.all()
    np.testing.assert_allclose(v, g * g * (a - b) ** 2 / 4, rtol=1e-12)
    v4, known4 = sref.variance(mom, n)                          # the default min_frames = 4: two frames are not trusted
    assert not known4.any() and (v4 == 1.0).all()
    _, _, mom = run_frames([a, b, b], n)
    np.testing.assert_allclose(mom[..., 0], np.mean([a, b, b]), rtol=1e-12)
    np.testing.assert_allclose(mom[..., 1], np.var([a, b, b]), rtol=1e-12)


def test_the_cap_binds_mw_as_it_binds_hw():
    _, hw, mom = run_frames([0.2, 0.5, 0.3], 4, max_history=6.0)
    np.testing.assert_allclose(hw, 10.0, rtol=1e-12)            # 4 + min(8, 6)
    np.testing.assert_allclose(mom[..., 2], 10.0, rtol=1e-12)
    # ... and the capped history counts as 6 samples of (m1', s'): the merge of (0.3, 0, 4) with (0.35, 0.0225, 6)
    np.testing.assert_allclose(mom[..., 0], (4 * 0.3 + 6 * 0.35) / 10, rtol=1e-12)
    np.testing.assert_allclose(mom[..., 1], 0.6 * 0.0225 + 24 * 0.05 ** 2 / 100, rtol=1e-12)


def test_misses_glass_and_pixels_without_history_know_nothing():
    frame, g, key, W, Hh = plane()
    for k in (np.uint64(tref.GLASS << 24), np.uint64(tref.MISS)):
        _, hw, mom = run_frames([0.2, 0.5, 0.3, 0.4, 0.1], 4, key=np.full((Hh, W), k, np.uint64))
        assert (hw == 4).all() and (mom[..., 2] == 4).all() and (mom[..., 1] == 0).all() and (mom[..., 0] == 0.1).all()
        v, known = sref.variance(mom, 4, min_frames=2.0)
        assert not known.any() and (v == 1.0).all()
    _, _, mom = run_frames([0.2], 4)                            # frame 0
    v, known = sref.variance(mom, 4, min_frames=2.0)
    assert (mom[..., 2] == 4).all() and not known.any() and (v == 1.0).all()
    # a slot crt_denoise_temporal wrote: the colour history is reused, the moments start again
    c, hw, mom, _ = sref.blend(accum_of(0.2, 4, (Hh, W)), 4, g, key, frame, None, W, Hh)
    c, hw, mom, _ = sref.blend(accum_of(0.5, 4, (Hh, W)), 4, g, key, frame, sref.slot(c, hw, None, g, key, frame), W, Hh)
    assert (hw == 8).all() and (mom[..., 2] == 4).all() and (mom[..., 1] == 0).all() and (mom[..., 0] == 0.5).all()
    # a variance that is not finite is not known
    v, known = sref.variance(np.float64([[[0.1, np.inf, 64.0]], [[np.nan, 0.1, 64.0]]]), 4)
    assert not known.any() and (v == 1.0).all()


# ------------------------------------------------------------------ 3. quality on three orbits
def setup_scenes(o):
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import PackedScene, orbit_cameras
    ps = cornell(o["size"], o["size"])
    cams = orbit_cameras(ps.camera, o["turn"])
    return [PackedScene(ps.primitives, ps.lights, cams[k].copy(), ps.spectra, ps.cie, ps.patches, ps.spectrum_index)
            for k in range(o["frames"])]


def orbit_mse(o, frame_of, truth_of, params=None, every_frame=False):
    """Set-up o with both filters on the same renders.  frame_of(k, first_sample) -> (accum, gbuf, keys, camera frame),
    truth_of(k) -> converged linear rgb.  Returns per measured frame (all, or the last alone) the display-space MSEs
    (blend alone, crt_denoise_temporal, crt_denoise_svgf)."""
    W = Hh = o["size"]
    p = dict(sref.DEFAULTS, **(params or {}))
    prev_t = prev_s = None
    rows = []
    for k in range(o["frames"]):
        acc, g, key, frame = frame_of(k, o["spp"] * k + 1)
        measured = every_frame or k == o["frames"] - 1
        if measured:
            out_t, c_t, hw_t, _ = tref.temporal(acc, o["spp"], g, key, frame, prev_t, W, Hh)
            out_s, _, c_s, hw_s, mom, _ = sref.svgf(acc, o["spp"], g, key, frame, prev_s, W, Hh, **p)
            assert np.array_equal(c_t, c_s) and np.array_equal(hw_t, hw_s)       # one blend
            truth = truth_of(k)
            rows.append((ref.mse_display(c_s, truth), ref.mse_display(out_t, truth), ref.mse_display(out_s, truth)))
        else:                                                   # (the passes leave nothing behind: only the blend is needed)
            c_s, hw_s, mom, _ = sref.blend(acc, o["spp"], g, key, frame, prev_s, W, Hh, **{k_: p[k_] for k_ in sref.BLEND})
            c_t, hw_t = c_s, hw_s
        prev_t = tref.slot(c_t, hw_t, g, key, frame)
        prev_s = sref.slot(c_s, hw_s, mom, g, key, frame)
    return rows


def oracle_renders(orc, o):
    """frame_of, truth_of of set-up o on oracle renders, each render made once."""
    scenes = setup_scenes(o)
    size = o["size"]
    frames, truths = {}, {}

    def frame_of(k, first):
        if (k, first) not in frames:
            sc = orc.Scene.from_packed(scenes[k])
            g, _ = ref.oracle_gbuffer(orc, scenes[k], (0, 0, size, size))
            frames[(k, first)] = (sc.render(o["spp"], first_sample=first)[0], g, ref.keys(g, scenes[k].primitives), sc.camera_frame())
        return frames[(k, first)]

    def truth_of(k):
        if k not in truths:
            sc = orc.Scene.from_packed(scenes[k])
            truths[k] = ref.linear_rgb(sc.render(o["truth_spp"], first_sample=o["truth_first"])[0], o["truth_spp"])
        return truths[k]
    return frame_of, truth_of


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_variance_guided_passes_beat_the_fixed_sigma_on_the_same_blend(orc, name):
    """The table of DESIGN.md 6g re-measured with the final restatement at the defaults.  Asserted: the ratio to
    crt_denoise_temporal is <= the measured value + 0.05 (libm differences: the oracle is deterministic), < 1 on A and
    <= 0.90 on B and C; on every frame of A the new MSE is <= 1.02 x the old."""
    o = SETUPS[name]
    rows = orbit_mse(o, *oracle_renders(orc, o), every_frame=name == "A")
    for k, (m_blend, m_t, m_s) in enumerate(rows):
        print(f"set-up {name}, frame {k + 1 if name == 'A' else o['frames']}: blend {m_blend:.5f}, temporal {m_t:.5f}, "
              f"svgf {m_s:.5f}, ratio {m_s / m_t:.3f}")
    _, m_t, m_s = rows[-1]
    assert m_s / m_t <= o["ratio"] + 0.05
    assert m_s / m_t < 1.0 if name == "A" else m_s / m_t <= 0.90
    if name == "A":
        assert all(s <= 1.02 * t for _, t, s in rows)
