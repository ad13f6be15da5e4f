"""GPU parity of the denoised preview (run with -m gpu on an MI355X): crt_denoise's linear rgb bits and rgba8 bytes
`==` the oracle's restatement of the f32 contract (orc.denoise, DESIGN.md 6a "f32 contract") applied to the product's
own G-buffer -- at every K, at the sigmas' extremes, at shapes that are not multiples of the 16 x 16 filter blocks or
the 8 x 8 G-buffer tiles, and on crafted accumulators.  The G-buffer itself is pinned to the oracle's first hit here
for the scenes tests/test_denoise_gpu.py does not cover."""
import numpy as np
import pytest

import denoise_ref as ref
from conftest import bits
from test_denoise_gpu import _render, assert_gbuffer
from test_gpu_parity import _mixed_scene

pytestmark = pytest.mark.gpu

SIGMAS = [1e-30, 1e-3, 1.0, 1e3, 3.4e38]


def _where(mask):
    y, x = np.argwhere(mask)[0]
    return int(x), int(y)


def assert_parity(r, sc, iterations=5, **sig):
    """crt_denoise == orc.denoise on the context's accumulator, sample count and G-buffer.  NaN payloads are not part of
    the contract (as for the accumulator in test_gpu_parity.py): a NaN channel must be NaN on both sides."""
    acc, g = r.read_accum(), r.read_gbuffer()
    rgba, rgb = r.denoise(iterations, rgb=True, **sig)
    want, want_rgba = sc.denoise(acc, r.sample, g, iterations=iterations, **sig)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(rgb), nan), f"NaN pattern differs (K = {iterations}, {sig})"
    bad = ((bits(rgb) != bits(want)) & ~nan).any(-1)
    if bad.any():
        x, y = _where(bad)
        raise AssertionError(f"K = {iterations}, {sig}: {int(bad.sum())} pixels differ, first at ({x}, {y}): "
                             f"{rgb[y, x, :3].tolist()} != {want[y, x, :3].tolist()}")
    bad = (rgba != want_rgba).any(-1)
    assert not bad.any(), f"K = {iterations}, {sig}: {int(bad.sum())} rgba8 pixels differ, first at {_where(bad)}"
    assert (bits(rgb[..., 3]) == 0).all()                               # channel 3 is +0.0 everywhere
    return rgb


def _oracle(ps):
    from oracle import orc
    return orc.Scene.from_packed(ps)


# ------------------------------------------------------------------ 1. every K, every sigma
def test_every_iteration_count_cornell(renderer):
    from computeraytracer_amd import cornell
    ps = cornell(256, 256)
    r, sc = _render(renderer, ps, 4), _oracle(ps)
    prev = None
    for K in range(11):
        rgb = assert_parity(r, sc, K)
        if 1 <= K <= 8:                                                 # (from K = 9 on every step leaves 256 x 256)
            assert not np.array_equal(bits(rgb), bits(prev))
        prev = rgb


@pytest.mark.parametrize("K", [3, 10])
def test_sigma_extremes(renderer, K):
    """Each sigma alone at 1e-30 .. 3.4e38 (the host clamp of 2^i / sigma^2 to 3e38 at one end, inverses that round to
    0 or a denormal at the other), then all three tiny and all three huge."""
    from computeraytracer_amd import cornell
    ps = cornell(256, 256)
    r, sc = _render(renderer, ps, 4), _oracle(ps)
    cases = [{name: s} for name in ("sigma_color", "sigma_normal", "sigma_plane") for s in SIGMAS]
    cases += [dict(sigma_color=s, sigma_normal=s, sigma_plane=s) for s in (SIGMAS[0], SIGMAS[-1])]
    for sig in cases:
        assert_parity(r, sc, K, **sig)


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("w, h", [(257, 131), (97, 61)])
def test_odd_full_frames(renderer, w, h):
    from computeraytracer_amd import cornell
    ps = cornell(w, h)
    r, sc = _render(renderer, ps, 3), _oracle(ps)
    for K in (1, 10):
        assert_parity(r, sc, K)


@pytest.mark.parametrize("tw, th", [(1, 1), (1, 37), (37, 1), (3, 3), (15, 17)])
def test_tiles_at_the_bottom_right_corner(renderer, tw, th):
    """Tiles narrower than the 5-tap footprint: every step from 1 on leaves the tile, so only the border rule acts."""
    from computeraytracer_amd import cornell
    ps = cornell(257, 131)
    r = _render(renderer, ps, 4, tile=(257 - tw, 131 - th, 257, 131))
    assert r.read_accum().shape == (th, tw, 4)
    assert_parity(r, _oracle(ps), 10)


def test_tile_one_more_than_a_block_wide(renderer):
    """16 k + 1 pixels wide (and 8 k + 1 tall): the last block column and G-buffer tile row hold one pixel."""
    from computeraytracer_amd import cornell
    ps = cornell(257, 131)
    r = _render(renderer, ps, 4, tile=(37, 29, 37 + 16 * 5 + 1, 29 + 8 * 6 + 1))
    assert_parity(r, _oracle(ps), 10)
    assert_parity(r, _oracle(ps), 4, sigma_color=0.05)


# ------------------------------------------------------------------ 3. crafted accumulators
def _crafted(acc, rng):
    """Negatives, zeros, NaN, +-inf, 1e38, denormals and islands of constant colour, at the centre, borders and
    corners of a 96 x 72 image."""
    a = acc.copy()
    h, w = a.shape[:2]
    spots = [(h // 2, w // 2), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 3), (h // 3, 0),
             (h - 1, w // 2), (h // 2, w - 1), (1, 1), (h - 2, w - 2)]
    values = [np.nan, np.inf, -np.inf, 1e38, -1e38, 0.0, -0.5, 1e-40, -1e-42, 3e38, 2.0]
    for (y, x), v in zip(spots, values):
        a[y, x, :3] = v
    a[5, 40, 1] = np.nan                                                # one channel only
    a[60, 7, 2] = np.inf
    a[30:38, 10:18, :3] = (0.4, 0.3, 0.2)                               # islands of one colour
    a[0:6, 60:70, :3] = 0.0
    a[40:50, 86:96, :3] = (2.0, 2.0, 2.0)
    a[20:24, 30:50, :3] = -a[20:24, 30:50, :3]                          # negative XYZ
    a[50:70:3, 20:60:7, :3] = rng.uniform(1e-45, 1e-38, (7, 6, 3))      # denormal and tiny
    return a


@pytest.mark.parametrize("sample", [1, 3, 2 ** 24 + 1])
def test_crafted_accumulators(renderer, sample):
    """write_accum puts crafted values under cornell 96 x 72's G-buffer; n = (float)sample rounds 2^24 + 1 to 2^24."""
    from computeraytracer_amd import cornell
    ps = cornell(96, 72)
    r, sc = _render(renderer, ps, 2), _oracle(ps)
    rng = np.random.default_rng(sample)
    a = _crafted(r.read_accum() * np.float32(sample / 2.0), rng)
    r.write_accum(a, sample)
    assert r.sample == sample
    for K in (0, 1, 2, 5, 10):
        rgb = assert_parity(r, sc, K)
    assert np.isnan(rgb[36, 48, :3]).all()                              # the NaN centre stays NaN
    assert np.isfinite(rgb[36, 40]).all()                               # and reaches no neighbour


# ------------------------------------------------------------------ 4. guides
def test_mixed_scene_gbuffer_and_filter(renderer, orc):
    """Patches, a glass and a diffuse sphere and triangles: the G-buffer is the oracle's first hit, and the filter over
    it (keys of three categories and materials) is the oracle's."""
    ps = _mixed_scene(160, 90)
    want, hit = ref.oracle_gbuffer(orc, ps, (0, 0, 160, 90), full_log=False)
    sc = orc.Scene.from_packed(ps)
    for mode in ("bvh2", "none"):
        r = _render(renderer, ps, 4, mode)
        assert_gbuffer(r.read_gbuffer(), want, hit)
        assert len(np.unique(sc.denoise_keys(want)[hit])) >= 3
        for K in (2, 5, 10):
            assert_parity(r, sc, K)


def test_atrium_brute_force_gbuffer_crop(renderer, orc):
    """CRT_ACCEL_NONE: k_dn_gbuffer takes intersect_all over 250k primitives."""
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(480, 270)
    x0, y0, w, h = rect = (300, 60, 24, 24)
    want, hit = ref.oracle_gbuffer(orc, ps, rect, full_log=False)
    r = _render(renderer, ps, 1, "none", tile=(x0, y0, x0 + w, y0 + h))
    assert_gbuffer(r.read_gbuffer(), want, hit)
    assert_parity(r, orc.Scene.from_packed(ps), 5)


def test_non_finite_camera_gbuffer(renderer, orc):
    """An eye at infinity: every primary ray is non-finite, so k_dn_gbuffer takes intersect_all (the reference loop)
    even under a BVH, and the record is the oracle's (NaN payloads aside)."""
    from computeraytracer_amd import cornell, scene as S
    c = cornell(48, 40)
    cam = c.camera.copy()
    cam[0] = np.inf
    ps = S.PackedScene(c.primitives, c.lights, cam, c.spectra, c.cie)
    want, hit = ref.oracle_gbuffer(orc, ps, (0, 0, 48, 40))
    assert hit.all()                                                    # the last primitive, for every pixel
    for mode in ("bvh2", "none"):
        g = _render(renderer, ps, 1, mode).read_gbuffer()
        assert np.array_equal(bits(g[..., 7]), bits(want[..., 7])), mode
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(g), nan), mode
        assert np.array_equal(bits(g)[~nan], bits(want)[~nan]), mode


def test_benchmark_size_atrium(renderer, orc):
    """Atrium at 1920 x 1080, K = 5: the oracle runs on every core."""
    from computeraytracer_amd.scenes_synth import atrium250k
    ps = atrium250k(1920, 1080)
    r = _render(renderer, ps, 2)
    assert_parity(r, orc.Scene.from_packed(ps), 5)


# ------------------------------------------------------------------ 5. the cache
def test_gbuffer_follows_a_new_camera_of_the_same_size(renderer, orc):
    from computeraytracer_amd import cornell, scene as S
    ps = cornell(64, 48)
    g1 = _render(renderer, ps, 1).read_gbuffer()
    cam = ps.camera.copy()
    cam[0] += 40.0                                                      # the eye moves; the size does not
    ps2 = S.PackedScene(ps.primitives, ps.lights, cam, ps.spectra, ps.cie)
    r = _render(renderer, ps2, 2)
    g2 = r.read_gbuffer()
    want, hit = ref.oracle_gbuffer(orc, ps2, (0, 0, 64, 48))
    assert_gbuffer(g2, want, hit)
    assert not np.array_equal(bits(g1), bits(g2))
    assert_parity(r, orc.Scene.from_packed(ps2), 5)
