"""CPU-only checks of crt_denoise_svgf's spatial variance estimate (option "svgf_spatial_pct", include/crt.h
"Variance-guided temporal filter"): the option is documented at every layer, the float64 restatement
(tests/denoise_svgf_spatial_ref.py) gives closed forms on 6g's static plane, and on oracle renders of the three Cornell
orbits and of the mini atrium the estimate closes the gap to crt_denoise_temporal that v = 1 leaves on short histories."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as ref
import denoise_svgf_ref as sref
import denoise_svgf_spatial_ref as spref
import denoise_temporal_ref as tref
from conftest import ROOT
from test_denoise_svgf_cpu import SETUPS as CORNELL, accum_of, plane

NODE = shutil.which("node")
B = 4.0                     # P = 400


def g_of(x):
    return 2.2 * np.exp(-2.2 * max(x, 0.0))


# ------------------------------------------------------------------ 1. the interface
def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_documents_the_option_in_both_places():
    h = _text("include", "crt.h")
    section = h[h.index("Variance-guided temporal filter"):h.index("crt_denoise_svgf_defaults(")]
    assert '"svgf_spatial_pct"' in section and "7x7" in section
    options = h[h.rindex("crt_set_option(") - 6000:h.rindex("crt_set_option(")]
    assert '"svgf_spatial_pct"' in options and "25..10000" in options
    assert "CRT_ABI_VERSION 2" in re.sub(r"\s+", " ", h)


def test_design_has_section_6j_and_6g_points_to_it():
    d = _text("DESIGN.md")
    assert re.search(r"^## 6j\. ", d, re.M)
    g = d[d.index("## 6g. "):d.index("## 6h. ")]
    assert "out of scope here" not in g and "6j" in g
    j = d[d.index("## 6j. "):]
    for word in ("svgf_spatial_pct", "k_dn_spatial_var", "denoise_svgf_spatial_sweep.json", "denoise_svgf_spatial.json",
                 "test_denoise_svgf_spatial_cpu.py"):
        assert word in j, word


def test_the_command_lines_know_spatial():
    from computeraytracer_amd.__main__ import parse_args
    base = ["--orbit", "4", "--denoise", "5", "--temporal"]
    assert parse_args(base + ["--variance"]).spatial is None
    assert parse_args(base + ["--variance", "--spatial"]).spatial == 400
    assert parse_args(base + ["--variance", "--spatial", "800"]).spatial == 800
    for bad in (base + ["--spatial"], ["--spatial"], base + ["--variance", "--spatial", "24"], base + ["--variance", "--spatial", "10001"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    js = _text("host", "index.js")
    assert "'spatial' in args" in js and "setOption('svgf_spatial_pct'" in js
    assert "svgf_spatial_pct" in _text("tools", "denoise_svgf_bench.py") and "--spatial" in _text("README.md")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_the_command_line_refuses_spatial_without_variance_and_the_addon_exports_what_it_did():
    out = subprocess.run([NODE, os.path.join(ROOT, "host", "index.js"), "--orbit", "2", "--denoise", "5", "--temporal", "--spatial"],
                         capture_output=True, text=True)
    assert out.returncode == 2 and "--spatial" in out.stderr
    addon = os.path.join(ROOT, "addon", "crt_napi.node")
    assert os.path.exists(addon), "build the addon first (__graft_entry__.build())"
    js = ("const a=require(%r);for(const n of ['setOption','denoiseSvgfDefaults','denoiseSvgf','denoiseSvgfAsync','readMoments',"
          "'denoiseTemporal','denoiseAdaptive','readMotion']) if(typeof a[n]!=='function') throw new Error(n);console.log('ok')" % addon)
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ------------------------------------------------------------------ 2. closed forms on 6g's static plane
def field(m1, M=8.0, W=16, Hh=16, key=None):
    """The plane (coplanar, one normal: every weight is 1) holding the means m1 (Hh, W) of weight M: (mom, known, g, key)."""
    _, g, key0, _, _ = plane(W, Hh)
    m1 = np.broadcast_to(np.asarray(m1, np.float64), (Hh, W))
    mom = np.stack([m1, np.zeros((Hh, W)), np.full((Hh, W), float(M))], -1)
    return mom, np.zeros((Hh, W), bool), g, key0 if key is None else key


def window(a, y, x, mask=None):
    """The values of a in the 7x7 window of (y, x) that exist (and that mask keeps)."""
    ys, xs = slice(max(0, y - 3), y + 4), slice(max(0, x - 3), x + 4)
    return a[ys, xs][np.ones_like(a[ys, xs], bool) if mask is None else mask[ys, xs]]


def two_values(Hh, W, a=0.3, delta=0.05):
    yy, xx = np.mgrid[0:Hh, 0:W]
    return a + delta * (((3 * xx + 5 * yy + xx * yy) % 7) < 3)


def test_a_flat_field_has_no_spread():
    v, A, doubt = spref.spatial_variance(*field(0.25), B)
    assert (v == 0.0).all() and A.max() == 49.0 and A.min() == 16.0 and not doubt.any()


def test_two_values_give_the_sample_variance_of_the_window():
    M = 8.0
    m1 = two_values(16, 16)
    v, A, _ = spref.spatial_variance(*field(m1, M), B)
    for y, x in ((8, 8), (3, 12), (0, 0), (15, 7), (2, 1)):
        win = window(m1, y, x)
        assert A[y, x] == win.size
        sigma2 = np.var(win, ddof=1) * M                        # the variance per sample
        np.testing.assert_allclose(v[y, x], B * g_of(win.mean()) ** 2 * sigma2 / M, rtol=1e-12)
    assert A[8, 8] == 49 and A[0, 0] == 16
    v1, _, _ = spref.spatial_variance(*field(m1, M), 1.0)       # the factor multiplies and nothing else
    np.testing.assert_allclose(v, B * v1, rtol=1e-15)


def test_an_image_smaller_than_the_window_uses_the_taps_that_exist():
    m1 = two_values(3, 5)
    v, A, _ = spref.spatial_variance(*field(m1, 4.0, W=5, Hh=3), B)
    for y in range(3):
        for x in range(5):
            win = window(m1, y, x)
            assert A[y, x] == win.size == (min(4, 3 - y) + min(3, y)) * (min(4, 5 - x) + min(3, x))
            np.testing.assert_allclose(v[y, x], B * g_of(win.mean()) ** 2 * np.var(win, ddof=1), rtol=1e-12)


def test_fewer_than_four_units_of_weight_keep_v_1():
    m1 = two_values(16, 16)
    key = np.zeros((16, 16), np.uint64)
    key[5, 5] = 7                                               # alone
    key[10, 2:5] = 9                                            # three in a row: A = 3
    key[12, 8:12] = 11                                          # four: A = 4
    v, A, doubt = spref.spatial_variance(*field(m1, key=key), B)
    assert v[5, 5] == 1.0 and A[5, 5] == 1.0 and (v[10, 2:5] == 1.0).all() and (A[10, 2:5] == 3.0).all()
    assert (A[12, 8:12] == 4.0).all() and doubt[12, 8:12].all() and not doubt[10, 2:5].any()
    np.testing.assert_allclose(v[12, 8:12], B * g_of(m1[12, 8:12].mean()) ** 2 * np.var(m1[12, 8:12], ddof=1), rtol=1e-12)
    assert A[5, 4] == window(m1, 5, 4).size - 1                 # ... and the neighbours do not take them in


def test_glass_misses_and_moments_that_are_not_finite_keep_v_1_and_feed_no_neighbour():
    m1 = two_values(16, 16).copy()
    key = np.zeros((16, 16), np.uint64)
    key[4, 4:9] = np.uint64(tref.GLASS << 24)
    key[9, 3:6] = np.uint64(tref.MISS)
    mom, known, g, _ = field(m1, key=key)
    mom[6, 10, 0], mom[7, 11, 0], mom[8, 12, 2], mom[6, 13, 2], mom[13, 13, 2] = np.nan, np.inf, np.inf, 0.0, -1.0
    out = [(6, 10), (7, 11), (8, 12), (6, 13), (13, 13)]
    v, A, _ = spref.spatial_variance(mom, known, g, key, B)
    assert (v[4, 4:9] == 1.0).all() and (v[9, 3:6] == 1.0).all() and all(v[p] == 1.0 and A[p] == 0.0 for p in out)
    keep = key == 0
    for p in out:
        keep[p] = False
    for y, x in ((6, 6), (7, 12), (10, 5), (12, 12)):
        win = window(m1, y, x, keep)
        assert A[y, x] == win.size < 49
        np.testing.assert_allclose(v[y, x], B * g_of(win.mean()) ** 2 * np.var(win, ddof=1), rtol=1e-12)
    # glass that fills the image: the option changes nothing
    mom, known, g, _ = field(m1, key=np.full((16, 16), np.uint64(tref.GLASS << 24)))
    assert (spref.spatial_variance(mom, known, g, np.full((16, 16), np.uint64(tref.GLASS << 24)), B)[0] == 1.0).all()


def test_a_known_pixel_keeps_its_own_variance_whatever_its_neighbours_hold():
    frame, g, key, W, Hh = plane()
    rng = np.random.default_rng(5)
    prev = None
    for k in range(3):
        acc = accum_of(0.3, 4, (Hh, W)) * (1.0 + 0.2 * rng.standard_normal((Hh, W, 1)))
        if k == 2:
            key = key.copy()
            key[:, 8:] = 1                                      # the right half turns up new: no history there
        a = spref.svgf(acc, 4, g, key, frame, prev, W, Hh, spatial_pct=400, min_frames=2.0, iterations=0)
        b = spref.svgf(acc, 4, g, key, frame, prev, W, Hh, spatial_pct=0, min_frames=2.0, iterations=0)
        z = sref.svgf(acc, 4, g, key, frame, prev, W, Hh, min_frames=2.0, iterations=0)
        assert all(np.array_equal(x, y) for x, y in zip(b[:6], z))          # P = 0 is 6g
        assert all(np.array_equal(x, y) for x, y in zip(a[2:5], z[2:5]))    # what stays behind does not depend on P
        prev = sref.slot(z[2], z[3], z[4], g, key, frame)
    known = sref.variance(z[4], 4, 2.0)[1]
    assert known[:, :8].all() and not known[:, 8:].any()
    assert np.array_equal(a[6][known], b[6][known]) and (b[6][~known] == 1.0).all()
    assert (a[6][~known] != 1.0).all() and (a[6][~known] > 0).all()


def test_mini_atrium_is_what_the_issue_defines():
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = spref.mini_atrium(64, 64)
    assert len(ps.primitives) == 6 + 128 + 576 == 710
    assert ps.primitives.tobytes() == spref.mini_atrium(64, 64).primitives.tobytes()
    assert callable(atrium250k)


# ------------------------------------------------------------------ 3. quality on four orbits
SETUPS = dict(CORNELL, M=dict(size=64, frames=8, spp=4, turn=64, truth_spp=512, truth_first=100001))
MEASURED = {"A": (1, 2, 3, 4, 5, 6, 7, 8), "B": (32,), "C": (32,), "M": (3, 5, 8)}
# MSE(P = 400) / MSE(P = 0) per (set-up, frame), measured with the float64 restatements on oracle renders: DESIGN.md 6j has
# the table this is one column of
RATIO = {("A", 1): 1.093, ("A", 2): 0.930, ("A", 3): 0.826, ("A", 4): 1.023, ("A", 5): 1.002, ("A", 6): 1.026, ("A", 7): 1.025,
         ("A", 8): 1.018, ("B", 32): 1.000, ("C", 32): 1.000, ("M", 3): 0.757, ("M", 5): 0.910, ("M", 8): 0.897}
# ... and on the last frame of A for the other values of the S2 sweep (the rule for the recommendation)
A8_OTHER = {100: 1.026, 200: 1.019, 800: 1.019}
BETTER = (("M", 3), ("M", 5), ("M", 8), ("A", 2), ("A", 3))      # ... asserted < 1 whatever the measured value


def orbit_rows(orc, name):
    """Set-up `name`: per measured frame (frame, MSE of crt_denoise_temporal, of crt_denoise_svgf at P = 0, at P = 400,
    the largest share of pixels in any doubt mask)."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import PackedScene, orbit_cameras
    o = SETUPS[name]
    W = Hh = o["size"]
    ps = spref.mini_atrium(W, Hh) if name == "M" else cornell(W, Hh)
    cams = orbit_cameras(ps.camera, o["turn"])
    prev_t = prev_s = None
    rows = []
    for k in range(o["frames"]):
        scene = PackedScene(ps.primitives, ps.lights, cams[k].copy(), ps.spectra, ps.cie, ps.patches, ps.spectrum_index)
        sc = orc.Scene.from_packed(scene)
        g, _ = ref.oracle_gbuffer(orc, scene, (0, 0, W, Hh))
        key, frame = ref.keys(g, scene.primitives), sc.camera_frame()
        acc = sc.render(o["spp"], first_sample=o["spp"] * k + 1)[0]
        if k + 1 in MEASURED[name]:
            truth = ref.linear_rgb(sc.render(o["truth_spp"], first_sample=o["truth_first"])[0], o["truth_spp"])
            out_t = tref.temporal(acc, o["spp"], g, key, frame, prev_t, W, Hh)[0]
            out_0, _, c, hw, mom, doubt, _, _ = spref.svgf(acc, o["spp"], g, key, frame, prev_s, W, Hh, spatial_pct=0)
            out_4, _, c4, hw4, mom4, _, v4, doubt_s = spref.svgf(acc, o["spp"], g, key, frame, prev_s, W, Hh, spatial_pct=400)
            assert np.array_equal(c, c4) and np.array_equal(hw, hw4) and np.array_equal(mom, mom4)
            rows.append((k + 1, ref.mse_display(out_t, truth), ref.mse_display(out_0, truth), ref.mse_display(out_4, truth),
                         max(float(doubt.mean()), float(doubt_s.mean()))))
            if (name, k + 1) == ("A", 8):
                for pct in A8_OTHER:
                    out_p = spref.svgf(acc, o["spp"], g, key, frame, prev_s, W, Hh, spatial_pct=pct)[0]
                    rows.append((pct, ref.mse_display(out_p, truth)))
        else:
            c, hw, mom, _ = sref.blend(acc, o["spp"], g, key, frame, prev_s, W, Hh, **{k_: sref.DEFAULTS[k_] for k_ in sref.BLEND})
        prev_t = tref.slot(c, hw, g, key, frame)
        prev_s = sref.slot(c, hw, mom, g, key, frame)
    return rows


@pytest.mark.parametrize("name", ["A", "B", "C", "M"])
def test_the_estimate_closes_the_gap_on_short_histories(orc, name):
    """The table of DESIGN.md 6j re-measured with the final restatement.  Asserted per row: MSE(P = 400) <= (measured ratio
    + 0.05) x MSE(P = 0) (libm differences: the oracle is deterministic); P = 400 better than P = 0 on M frames 3, 5, 8 and
    A frames 2, 3; M frame 8 at P = 400 within 1.02 x crt_denoise_temporal; every doubt mask <= 2 %."""
    rows = orbit_rows(orc, name)
    other, rows = [r for r in rows if len(r) == 2], [r for r in rows if len(r) == 5]
    for pct, m_p in other:
        print(f"set-up {name}, frame 8: P={pct} {m_p:.5f}; P={pct} / P=0 {m_p / rows[-1][2]:.3f}")
        assert m_p <= (A8_OTHER[pct] + 0.05) * rows[-1][2], pct
    for k, m_t, m_0, m_4, doubt in rows:
        print(f"set-up {name}, frame {k}: temporal {m_t:.5f}, svgf P=0 {m_0:.5f}, P=400 {m_4:.5f}; P=400 / P=0 {m_4 / m_0:.3f}, "
              f"P=400 / temporal {m_4 / m_t:.3f}; doubt {doubt:.4f}")
    for k, m_t, m_0, m_4, doubt in rows:
        assert m_4 <= (RATIO[(name, k)] + 0.05) * m_0, (name, k)
        if (name, k) in BETTER:
            assert m_4 < m_0, (name, k)
        if (name, k) == ("M", 8):
            assert m_4 <= 1.02 * m_t
        assert doubt <= 0.02, (name, k)
