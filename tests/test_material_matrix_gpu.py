"""GPU parity on the scenes of material_matrix_scenes.py (run with -m gpu on an MI355X): glass patches, glass
triangles, triangle lights, a sphere light, a scene without a patch (S.npatch == 0, the one-light scalar load of the
light record holding a triangle) and a scene of spheres only (a light of area 0: NaN wherever it contributes).  Every
render is 96 x 96 at 4 samples against the oracle -- bit for bit on the f32 accumulator and on every rgba8 byte -- in
every pipeline form and under every builder; then progressive frames, the counters, two pipes with the tail forms, the
ray level and the first-hit G-buffer.  test_material_matrix_cpu.py asserts that the scenes reach the pairs."""
import numpy as np
import pytest

import denoise_ref as ref
import material_matrix_scenes as MM
from conftest import bits
from test_denoise_gpu import assert_gbuffer
from test_gpu_parity import MAXU, assert_same_image, render

pytestmark = pytest.mark.gpu

W = H = 96
SPP = 4
BUILDER = {"bvh2": "sah-host", "lbvh": "lbvh-gpu", "ploc": "ploc-gpu"}
# (pipeline, quantize, wf_width, wf_trace_form, accel mode)
FORMS = [(1, 1, 4, 2, "bvh2"), (1, 1, 4, 1, "bvh2"), (1, 1, 8, 2, "bvh2"), (1, 0, 4, 2, "bvh2"), (0, 1, 4, 2, "bvh2"),
         (1, 1, 4, 2, "none"), (1, 1, 4, 2, "lbvh"), (1, 1, 4, 2, "ploc")]

_ORACLE = {}


def oracle_frame(orc, name):
    """(scene, oracle scene, accumulator, rgba8, counters) of the 4-sample frame: rendered once, shared, left unchanged."""
    if name not in _ORACLE:
        ps = MM.build(name, W, H)
        sc = orc.Scene.from_packed(ps)
        acc, rgba, cnt = sc.render(SPP)
        for a in (acc, rgba, cnt):
            a.setflags(write=False)
        _ORACLE[name] = (ps, sc, acc, rgba, cnt)
    return _ORACLE[name]


def assert_frame(name, acc, rgba, acc_o, rgba_o, what):
    """assert_same_image; on sphere_only the rule of the NaN-light tests: the same NaN mask, bit-identical elsewhere
    (NaN payloads are not part of the contract), rgba8 equal everywhere."""
    if name != "sphere_only":
        assert not np.isnan(acc_o[..., :3]).any()
        assert_same_image(acc, rgba, acc_o, rgba_o)
        return
    nan_o = np.isnan(acc_o[..., :3]).any(-1)
    assert 0.1 <= nan_o.mean() <= 0.9
    assert np.array_equal(np.isnan(acc[..., :3]), np.isnan(acc_o[..., :3])), what
    assert np.array_equal(bits(acc[~nan_o])[..., :3], bits(acc_o[~nan_o])[..., :3]), what
    assert np.array_equal(rgba, rgba_o), what


def set_form(r, pipeline=1, quantize=1, wf_width=4, wf_trace_form=2):
    r.set_option("pipeline", pipeline).set_option("quantize", quantize).set_option("wf_width", wf_width).set_option("wf_trace_form", wf_trace_form)


# ------------------------------------------------------------------ 1. image parity in every form
@pytest.mark.parametrize("name", MM.NAMES)
def test_every_form_gives_the_oracle_image(renderer, orc, name):
    ps, _, acc_o, rgba_o, _ = oracle_frame(orc, name)
    try:
        for pipeline, quant, width, form, mode in FORMS:
            set_form(renderer, pipeline, quant, width, form)
            acc, rgba = render(renderer, ps, SPP, mode)
            if mode != "none":
                assert renderer.accel_stats()["builder"] == BUILDER[mode], (name, mode)
            try:
                assert_frame(name, acc, rgba, acc_o, rgba_o, (pipeline, quant, width, form, mode))
            except AssertionError as e:
                raise AssertionError(f"{name}: pipeline {pipeline} quantize {quant} wf_width {width} wf_trace_form {form} accel {mode}: {e}") from None
    finally:
        set_form(renderer)


# ------------------------------------------------------------------ 2. progressive == fused
@pytest.mark.parametrize("name", MM.NAMES)
def test_progressive_frames_equal_the_fused_frame(renderer, orc, name):
    """1 + 1 + 2 samples, with a sync after each call and with none: the NEE term of a triangle or sphere light parks in
    the slot across a bounce and across the slot refills of the next samples."""
    ps, _, acc_o, rgba_o, _ = oracle_frame(orc, name)
    renderer.upload(ps).build_accel("bvh2")
    for synced in (True, False):
        renderer.reset()
        for n in (1, 1, 2):
            renderer.frame(n)
            if synced:
                renderer.sync()
        renderer.sync()
        assert renderer.sample == SPP
        assert_frame(name, renderer.read_accum(), renderer.read_rgba8(), acc_o, rgba_o, f"1 + 1 + 2, synced {synced}")


# ------------------------------------------------------------------ 3. counters
@pytest.mark.parametrize("name", ["tri", "tri_only"])
def test_counters_match_the_oracle(renderer, orc, name):
    ps, _, acc_o, rgba_o, cnt = oracle_frame(orc, name)
    try:
        renderer.upload(ps).build_accel("bvh2").enable_counters(True).reset_counters()
        renderer.frame(SPP).sync()
        c = renderer.counters()
    finally:
        renderer.enable_counters(False)
    assert_same_image(renderer.read_accum(), renderer.read_rgba8(), acc_o, rgba_o)
    assert (c["rays"], c["paths"], c["bounces"], c["shadow"]) == (int(cnt[0]), int(cnt[2]), int(cnt[3]), int(cnt[4]))
    assert 0 < c["walked"] <= c["rays"] and c["rays"] - c["walked"] <= c["shadow"]


# ------------------------------------------------------------------ 4. two pipes and the tail
def test_two_pipes_and_the_tail_forms_on_triangle_lights(renderer, orc):
    """wf_finish_at = 4096 moves the last paths to the side pool: k_wf_finish's form of light_sample on a triangle light."""
    ps, _, acc_o, rgba_o, _ = oracle_frame(orc, "tri")
    try:
        for tail_walk in (0, 1):
            for finish_at in (0, 4096):
                renderer.set_option("wf_pipes", 2).set_option("wf_tail_walk", tail_walk).set_option("wf_finish_at", finish_at)
                acc, rgba = render(renderer, ps, SPP)
                try:
                    assert_same_image(acc, rgba, acc_o, rgba_o)
                except AssertionError as e:
                    raise AssertionError(f"wf_tail_walk {tail_walk} wf_finish_at {finish_at}: {e}") from None
    finally:
        renderer.set_option("wf_pipes", 2).set_option("wf_tail_walk", 1).set_option("wf_finish_at", 32768)


# ------------------------------------------------------------------ 5. ray level
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(ps, sc, name, rng):
    """~20 000 rays: random ones (exclude on every 7th); rays started ON glass surfaces with no exclusion, through and
    along the surface (origins: the oracle's hit positions of rays aimed at the glass); rays in the plane of the lights
    (for a sphere light: its top tangent plane); a block of NaN directions."""
    prims = ps.primitives
    cat, mat = prims["category"], prims["data4"][:, 2]
    lo, hi = (np.float32([-40, -40, -40]), np.float32([600, 600, 600]))
    n_rand = 12000
    o = [rng.uniform(lo, hi, (n_rand, 3))]
    d = [_unit(rng.normal(size=(n_rand, 3)))]
    ex = [np.full(n_rand, MAXU, np.uint32)]
    ex[0][::7] = rng.integers(0, len(prims), len(ex[0][::7]))
    # on the glass: aim at points of the glass primitives from outside, keep what the oracle says lands on glass
    glass = np.flatnonzero(mat == 2)
    pos, nrm, din, own = [], [], [], []
    tries = 0
    while len(pos) < 1000 and tries < 20000:
        tries += 1
        g = prims[rng.choice(glass)]
        if g["category"] == 1:
            target = g["data1"] + g["data2"][0] * 0.7 * _unit(rng.normal(size=(1, 3)))[0]
        else:
            u, v = rng.uniform(0.05, 0.95, 2)
            if g["category"] == 2 and u + v > 1:
                u, v = 1 - u, 1 - v
            target = g["data1"] + u * g["data2"] + v * g["data3"]
        src = rng.uniform(lo, hi, 3)
        dd = (target - src).astype(np.float32)
        dd /= np.linalg.norm(dd)
        of, ou = sc.intersect(src.astype(np.float32), dd)
        if ou[0] and mat[int(ou[1])] == 2:
            pos.append(of[1:4].copy()); nrm.append(of[4:7].copy()); din.append(dd); own.append(int(ou[1]))
    pos, nrm, din = np.float32(pos), np.float32(nrm), np.float32(din)
    assert len(pos) == 1000 and len(set(cat[own])) == len(set(cat[glass])), "the on-surface rays cover every glass category"
    tang = _unit(np.cross(nrm, rng.normal(size=nrm.shape)))
    for dirs in (din, -nrm, tang, _unit(tang + 1e-3 * nrm), _unit(tang - 1e-3 * nrm)):      # through, straight in, along, grazing out / in
        o.append(pos); d.append(dirs); ex.append(np.full(len(pos), MAXU, np.uint32))
    # in the plane of the lights
    lights = prims[mat == 1]
    n_pl = 2000
    L = lights[rng.integers(0, len(lights), n_pl)]
    sph = (L["category"] == 1)[:, None]
    y = np.where(sph[:, 0], L["data1"][:, 1] + L["data2"][:, 0], L["data1"][:, 1])
    po = rng.uniform(lo, hi, (n_pl, 3))
    po[:, 1] = y
    pd = rng.normal(size=(n_pl, 3))
    pd[:, 1] = 0.0
    o.append(po); d.append(_unit(pd)); ex.append(np.full(n_pl, MAXU, np.uint32))
    # NaN directions
    o.append(rng.uniform(lo, hi, (200, 3))); d.append(np.full((200, 3), np.nan)); ex.append(np.full(200, MAXU, np.uint32))
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32), np.concatenate(ex)


@pytest.mark.parametrize("name", ["tri", "tri_only", "sphere_only"])
def test_ray_level_on_the_new_geometry(renderer, orc, name):
    ps, sc, *_ = oracle_frame(orc, name)
    o, d, ex = _rays(ps, sc, name, np.random.default_rng(sum(map(ord, name))))
    assert 19000 <= len(o) <= 21000
    renderer.upload(ps).build_accel("none")
    brute = renderer.debug_intersect(o, d, ex)
    i_ref = brute[:, 7].view(np.uint32)
    hit = i_ref != MAXU
    fin = hit & ~np.isnan(d).any(1)
    assert 0.2 < hit.mean() <= 1.0, hit.mean()
    for mode in ("bvh2", "lbvh", "ploc"):
        renderer.build_accel(mode)
        assert renderer.accel_stats()["builder"] == BUILDER[mode]
        got = renderer.debug_intersect(o, d, ex)
        bad = got[:, 7].view(np.uint32) != i_ref
        assert not bad.any(), f"{name} / {mode}: {int(bad.sum())} hit indices differ from the loop, first ray {int(np.flatnonzero(bad)[0])}"
        bad = (bits(got[fin]) != bits(brute[fin])).any(1)
        assert not bad.any(), f"{name} / {mode}: {int(bad.sum())} hit records differ from the loop, first ray {int(np.flatnonzero(fin)[np.flatnonzero(bad)[0]])}"
        # ... and through the kernel frame() launches on the wide tree (the finite rays: a non-finite one never reaches it)
        ok = np.isfinite(d).all(1)
        t_wf, i_wf, _, rep = renderer.debug_trace_rays(o[ok], d[ok], ex[ok])
        assert rep["kernel"] == "k_wf_trace2", rep
        bad = (i_wf != i_ref[ok]) | (hit[ok] & (bits(t_wf) != bits(brute[ok, 0])))
        assert not bad.any(), f"{name} / {mode}: {int(bad.sum())} rays differ from the loop in {rep['kernel']}, first ray {int(np.flatnonzero(ok)[np.flatnonzero(bad)[0]])}"
    for i in range(0, len(o), 40):
        of, ou = sc.intersect(o[i], d[i], int(ex[i]))
        assert int(i_ref[i]) == (int(ou[1]) if ou[0] else MAXU), (name, i)
        if ou[0] and not np.isnan(d[i]).any():          # NaN payloads are not part of the contract
            assert np.array_equal(bits(brute[i, :7]), bits(of)), (name, i)


# ------------------------------------------------------------------ 6. first-hit G-buffer
def test_gbuffer_carries_glass_on_flat_primitives(renderer, orc):
    """crt_read_gbuffer's record is the oracle's first hit, and the filter's key holds the glass material for a glass
    patch and a glass triangle as it does for a glass sphere."""
    ps, sc, *_ = oracle_frame(orc, "tri")
    want, hit = ref.oracle_gbuffer(orc, ps, (0, 0, W, H))
    idx = want[..., 7].view(np.uint32)
    cat = np.where(hit, ps.primitives["category"][np.where(hit, idx, 0)], 9)
    mat = np.where(hit, ps.primitives["data4"][:, 2][np.where(hit, idx, 0)], 9)
    key_o = sc.denoise_keys(want)
    for c in (0, 2):
        px = (cat == c) & (mat == 2)
        assert px.sum() >= 100, (c, int(px.sum()))
        assert (key_o[px] >> 24 == 2).all()
    for mode in ("bvh2", "none"):
        renderer.upload(ps).build_accel(mode).frame(1).sync()
        g = renderer.read_gbuffer()
        assert_gbuffer(g, want, hit)
        assert np.array_equal(sc.denoise_keys(g), key_o), mode
        assert np.array_equal(ref.keys(g, ps.primitives)[hit], key_o[hit].astype(np.uint64)), mode
