"""CPU-only checks of option "adaptive_temporal" (include/crt.h "Sample offset" and "Temporal reuse across camera moves",
DESIGN.md 6i): the float64 restatement (tests/denoise_temporal_adaptive_ref.py) gives the closed forms where two halves of
a static plane hold different counts, the header documents the option, the command lines take --adaptive with --orbit, and
on oracle renders of an orbit the adaptive blend is no worse than the uniform one that spends more samples."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref
import denoise_ref as ref
import denoise_svgf_ref as sref
import denoise_temporal_adaptive_ref as taref
from conftest import ROOT
from test_denoise_svgf_cpu import plane

NODE = shutil.which("node")
F = np.float32


# ------------------------------------------------------------------ 1. the restatement on a static plane, two counts
def test_two_halves_with_their_own_counts_give_the_closed_forms_per_half():
    """The plane of test_denoise_svgf_cpu.py, every pixel finding itself; the left half's tiles hold 2 samples per
    frame and the right half's 6, over three frames of mean luminance ys[k] per half: Hw = Mw = 3 n, m1 the mean and s
    the population variance of the half's three frame means."""
    frame, g, key, W, Hh = plane()
    counts = np.uint32([[2, 6], [2, 6]])                        # 16 x 16: two tiles by two
    npx = taref.pixel_counts(counts, Hh, W)
    assert (npx[:, :8] == 2).all() and (npx[:, 8:] == 6).all()
    ys = {2: [0.2, 0.5, 0.35], 6: [0.7, 0.1, 0.4]}
    prev = None
    for k in range(3):
        y = np.where(npx == 2, ys[2][k], ys[6][k])
        accum = np.repeat((y * npx)[..., None], 3, -1)          # XYZ sums of n_p samples whose mean is y (a grey)
        c, hw, mom, _ = taref.blend(accum, npx, g, key, frame, prev, W, Hh)
        prev = taref.slot(c, hw, mom, g, key, frame)
    for n, half in ((2, np.s_[:, :8]), (6, np.s_[:, 8:])):
        np.testing.assert_allclose(hw[half], 3.0 * n, rtol=1e-12)
        np.testing.assert_allclose(mom[half][..., 2], 3.0 * n, rtol=1e-12)
        np.testing.assert_allclose(mom[half][..., 0], np.mean(ys[n]), rtol=1e-12)
        np.testing.assert_allclose(mom[half][..., 1], np.var(ys[n]), rtol=1e-12)
        np.testing.assert_allclose(c[half], ref.linear_rgb(np.full((1, 1, 3), np.mean(ys[n])), 1)[0, 0] + 0 * c[half], rtol=1e-12)
    # F = Mw / n_p = 3 frames on both halves, whatever the count
    v, known = taref.variance(mom, npx, min_frames=3.0)
    assert known.all()
    for n, half in ((2, np.s_[:, :8]), (6, np.s_[:, 8:])):
        gs = 2.2 * np.exp(-2.2 * np.mean(ys[n]))
        np.testing.assert_allclose(v[half], gs * gs * np.var(ys[n]) / 2.0, rtol=1e-12)
    # ... and one uniform n would see 9 frames on the right half (or 1 on the left): the substitution is what is tested
    v_uniform, _ = sref.variance(mom, 2, min_frames=3.0)
    assert not np.allclose(v_uniform[:, 8:], v[:, 8:])


def test_uniform_counts_are_the_uniform_restatement():
    frame, g, key, W, Hh = plane()
    rng = np.random.default_rng(5)
    prev_a = prev_u = None
    for k in range(3):
        accum = rng.random((Hh, W, 3)) * 4
        a = taref.blend(accum, np.full((Hh, W), 4, np.uint32), g, key, frame, prev_a, W, Hh)
        u = sref.blend(accum, 4, g, key, frame, prev_u, W, Hh)
        assert all(np.array_equal(x, y) for x, y in zip(a, u))
        prev_a, prev_u = taref.slot(*a[:3], g, key, frame), sref.slot(*u[:3], g, key, frame)
    assert all(np.array_equal(x, y) for x, y in zip(taref.variance(a[2], np.full((Hh, W), 4), 2.0), sref.variance(u[2], 4, 2.0)))


# ------------------------------------------------------------------ 2. the header and the option
def _section(text, title):
    m = re.search(r"/\* -+ " + re.escape(title) + r"\n(.*?)\*/", text, re.S)
    assert m, title
    return m.group(1)


def test_header_documents_the_option():
    text = open(os.path.join(ROOT, "include", "crt.h")).read()
    assert re.search(r"#define CRT_ABI_VERSION 2\b", text)
    assert '"adaptive_temporal"' in _section(text, "Sample offset")
    assert '"adaptive_temporal"' in _section(text, "Temporal reuse across camera moves")
    options = text[text.index("/* Tuning knobs."):text.index("int crt_set_option(")]
    assert re.search(r'"adaptive_temporal" \(0 \| 1, anything else is CRT_EINVAL', options)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "6i" in design and "adaptive_temporal" in design
    for inst in ("<false, false, true>", "<true, false, true>", "<false, true, true>", "<true, true, true>"):
        assert "k_dn_reproject" + inst in design, inst


def test_the_library_has_no_new_symbol():
    from computeraytracer_amd import _lib
    assert _lib.load().crt_abi_version() == 2                   # an option, not a call: the change is additive


# ------------------------------------------------------------------ 3. the command lines
def test_python_command_line_takes_adaptive_with_orbit():
    from computeraytracer_amd.__main__ import parse_args
    a = parse_args(["--adaptive", "0.3", "--orbit", "8", "--spp", "8", "--adaptive-step", "2", "--denoise", "5", "--temporal",
                    "--variance", "--counts-out", "c.png"])
    assert a.adaptive == pytest.approx(0.3) and a.orbit == 8 and a.temporal and a.variance and a.counts_out == "c.png"
    assert parse_args(["--adaptive", "0.3", "--orbit", "2"]).orbit == 2
    assert parse_args(["--adaptive", "0.3", "--orbit", "2", "--denoise", "3", "--temporal"]).denoise == 3
    for bad in (["--adaptive", "0.3", "--checkpoint", "x.npz"],
                ["--adaptive", "0.3", "--orbit", "2", "--checkpoint", "x.npz"],
                ["--adaptive", "0.3", "--temporal"],                                # --temporal still needs --orbit N --denoise K
                ["--adaptive", "0.3", "--orbit", "2", "--temporal"],
                ["--orbit", "2", "--counts-out", "c.png"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_command_line_no_longer_refuses_adaptive_with_orbit():
    """The refusals that remain are decided before a device is opened, and --adaptive with --orbit is not among them."""
    index = os.path.join(ROOT, "host", "index.js")
    out = subprocess.run([NODE, index, "--adaptive", "0.3", "--orbit", "2", "--temporal"], capture_output=True, text=True)
    assert out.returncode == 2 and "--temporal goes with --orbit N --denoise K" in out.stderr
    src = open(index).read()
    assert "does not go with --orbit" not in src and "setOption('adaptive_temporal', 1)" in src


# ------------------------------------------------------------------ 4. quality on an orbit
# Cornell 64 x 64, 8 frames, 1/64 turn per frame, frame k drawn from sample index 8 k + 1 on; adaptive rounds of 2 samples,
# min_samples 2, max_samples 8, threshold 0.3; MSE of the last frame in display space against 1024 spp drawn at sample
# index 100 001.  `ratio`: crt_denoise_svgf of the adaptive orbit over crt_denoise_svgf of the uniform orbit of 4 samples per
# frame, both at the defaults, measured with the float64 restatements on oracle renders (DESIGN.md 6i has the table).
SETUP = dict(size=64, frames=8, turn=64, stride=8, step=2, min_samples=2, max_samples=8, threshold=0.3, truth_spp=1024,
             truth_first=100001, ratio=1.017)


def adaptive_counts(samples_y, o, exp_):
    """The tile counts crt_trace_adaptive's rounds end at, from the per-sample luminances samples_y (max_samples, h, w) of
    the frame: the rule of adaptive_ref on the float32 sums, round by round."""
    h, w = samples_y.shape[1:]
    counts = np.zeros(((h + 7) // 8, (w + 7) // 8), np.uint32)
    S, Q = np.zeros((h, w), F), np.zeros((h, w), F)
    while True:
        E = adaptive_ref.tile_errors(S, Q, counts, exp_)
        act = adaptive_ref.active(counts, E, o["min_samples"], o["max_samples"], o["threshold"])
        if not act.any():
            return counts
        grow = adaptive_ref.pixel_counts(act, h, w).astype(bool)
        for _ in range(o["step"]):
            npx = adaptive_ref.pixel_counts(counts, h, w)
            y = np.take_along_axis(samples_y, np.minimum(npx, o["max_samples"] - 1)[None].astype(np.int64), 0)[0]
            S = np.where(grow, (S + y).astype(F), S)
            Q = np.where(grow, (Q + (y * y).astype(F)).astype(F), Q)
            counts = counts + act.astype(np.uint32)


def test_adaptive_frames_blend_no_worse_than_uniform_ones_that_cost_more(orc):
    """The table of DESIGN.md 6i re-measured with the final restatement.  Asserted: the adaptive orbit spends fewer
    samples than the uniform orbit of ceil(mean) = 4 per frame and its blend's MSE on the last frame is <= that orbit's;
    after crt_denoise_svgf's passes the ratio to uniform-4 is <= the measured value + 0.05 (libm differences: the
    oracle is deterministic)."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import PackedScene, orbit_cameras
    o = SETUP
    size = o["size"]
    ps = cornell(size, size)
    cams = orbit_cameras(ps.camera, o["turn"])
    exp_ = lambda x: orc.math_eval("exp", np.asarray(x, F))
    p = sref.DEFAULTS
    runs = {"uniform 4": 4, "uniform 6": 6, "adaptive": None}
    prev = dict.fromkeys(runs)
    rows, means = {}, []
    for k in range(o["frames"]):
        psk = PackedScene(ps.primitives, ps.lights, cams[k].copy(), ps.spectra, ps.cie, ps.patches, ps.spectrum_index)
        sc = orc.Scene.from_packed(psk)
        g, _ = ref.oracle_gbuffer(orc, psk, (0, 0, size, size))
        key, frame = ref.keys(g, psk.primitives), sc.camera_frame()
        # samples B + 1 .. B + 8 one by one, and their float32 sums in sample order: sums[n] is the frame of n samples
        each = [sc.render(1, first_sample=o["stride"] * k + j)[0] for j in range(1, o["max_samples"] + 1)]
        sums = [np.zeros_like(each[0])]
        for a in each:
            sums.append((sums[-1] + a).astype(F))
        counts = adaptive_counts(np.stack([a[..., 1] for a in each]), o, exp_)
        npx = taref.pixel_counts(counts, size, size)
        means.append(float(npx.mean()))
        last = k == o["frames"] - 1
        if last:
            truth = ref.linear_rgb(sc.render(o["truth_spp"], first_sample=o["truth_first"])[0], o["truth_spp"])
        for name, n in runs.items():
            if n is None:
                acc = np.take_along_axis(np.stack(sums), npx[None, ..., None].astype(np.int64), 0)[0]
                n_of = npx
            else:
                acc, n_of = sums[n], np.full((size, size), n, np.uint32)
            if last:
                out, _, c, hw, mom, _ = taref.svgf(acc, n_of, g, key, frame, prev[name], size, size)
                rows[name] = (ref.mse_display(c, truth), ref.mse_display(out, truth))
            else:
                c, hw, mom, _ = taref.blend(acc, n_of, g, key, frame, prev[name], size, size, **{q: p[q] for q in sref.BLEND})
            prev[name] = taref.slot(c, hw, mom, g, key, frame)
    mean = float(np.mean(means))
    for name, (m_blend, m_out) in rows.items():
        print(f"{name}: mean samples {mean if runs[name] is None else runs[name]:.2f}, blend alone {m_blend:.5f}, "
              f"after the passes {m_out:.5f}")
    ratio = rows["adaptive"][1] / rows["uniform 4"][1]
    print(f"mean samples per frame {['%.2f' % m for m in means]}; filtered ratio to uniform 4: {ratio:.3f}")
    assert mean < 4.0 and math.ceil(mean) == 4
    assert rows["adaptive"][0] <= rows["uniform 4"][0]
    assert ratio <= o["ratio"] + 0.05
