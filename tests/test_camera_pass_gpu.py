"""GPU tests of the first-hit camera pass (run with -m gpu on an MI355X): the G-buffer,
crt_render_aovs, crt_render_mattes and crt_pick are each pinned to the oracle elsewhere; here they are pinned to each other.  At sample
offset kDnSample - 1 with one sample, the one camera ray every pass traces per pixel is the G-buffer's, so all four must
report the same hit, bit for bit -- on a tile whose sides are no multiple of 8 and that does not start at the origin,
under the reference's loop, the default tree and the unquantised one.  The two render calls also share their refusals."""
import ctypes as C

import numpy as np
import pytest

import aov_ref
import matte_ref
from conftest import bits

pytestmark = pytest.mark.gpu

K_DN_SAMPLE = 8                         # crt_device.h kDnSample
W, H = 40, 32
X0, Y0, TW, TH = 7, 5, 27, 21           # neither side a multiple of 8, and not at the origin
MISS = 0xFFFFFFFF
EINVAL, ESTATE = -1, -3
_SCENE = []


def mixed_scene():
    """The Cornell box without its back wall (floor, ceiling, light, side walls: patches), a small torus of 2 * 16 * 10
    triangles, a glass and a diffuse sphere: rays between them leave the scene."""
    if not _SCENE:
        from computeraytracer_amd import scene as S
        from computeraytracer_amd import scenes_synth as SY
        sc = S.load_scene()
        base = S.pack_scene({"camera": dict(sc["camera"], width=W, height=H), "spectra": sc["spectra"],
                             "objects": {"patches": [sc["objects"]["patches"][k] for k in (0, 1, 2, 4, 5)], "spheres": []}})
        a, b = np.arange(16) * (2 * np.pi / 16), np.arange(10) * (2 * np.pi / 10)
        rad = 110.0 + 45.0 * np.cos(b)[None, :]
        P = np.stack([278.0 + rad * np.cos(a)[:, None], 230.0 + 45.0 * np.sin(b)[None, :] + 0.0 * a[:, None],
                      300.0 + rad * np.sin(a)[:, None]], axis=-1)
        v0, v1, v2 = SY._grid_tris(P, True, True)
        idx = base.spectrum_index
        tri = SY._with_triangles(base, v0, v1, v2, np.where(np.arange(len(v0)) % 2, idx["red"], idx["white"]))
        n = len(tri.primitives)
        sph = S.make_primitives([1, 1], [[130, 90, 160], [430, 100, 200]], [[90] * 3, [100] * 3], [[0] * 3] * 2, [idx["dark"]] * 2,
                                [idx["red"], idx["white"]], [S.TYPE_INDEX["glass"], S.TYPE_INDEX["diffuse"]], first_index=n)
        prims = np.zeros(n + 2, S.PRIM_DTYPE)
        prims[:n] = tri.primitives
        prims[n:] = sph
        prims.setflags(write=False)
        _SCENE.append(S.PackedScene(prims, S.lights_of(prims), base.camera, base.spectra, base.cie))
    return _SCENE[0]


@pytest.mark.parametrize("mode,quantize", [("none", 1), ("bvh2", 1), ("bvh2", 0)])
def test_one_sample_of_every_pass_is_the_gbuffer(renderer, mode, quantize):
    ps = mixed_scene()
    prims = np.asarray(ps.primitives)
    assert 300 <= len(prims) <= 400 and len(ps.lights) == 1
    assert sorted(np.unique(prims["category"])) == [0, 1, 2] and sorted(np.unique(prims["data4"][:, 2])) == [0, 1, 2]
    r = renderer
    try:
        r.set_option("quantize", quantize)
        r.upload(ps).set_tile(X0, Y0, X0 + TW, Y0 + TH).build_accel(mode)
        r.frame(1).sync()                                    # (crt_read_gbuffer wants a sample in the accumulator)
        g = r.read_gbuffer()
        # the render calls take an explicit n at sample 0; the offset is set there (CRT_ACCEL_NONE traces under no offset)
        r.reset().set_sample_offset(K_DN_SAMPLE - 1)
        aov = r.render_aovs(1)
        prim = r.render_mattes(1, "primitive", 1)
        mat = r.render_mattes(1, "material", 1)
        xs, ys = np.meshgrid(np.arange(X0, X0 + TW), np.arange(Y0, Y0 + TH))
        pick = r.pick_pixels(np.stack([xs.ravel(), ys.ravel()], 1))      # global coordinates, row-major over the tile
    finally:
        r.set_option("quantize", 1)
        r.set_sample_offset(0)
    assert g.shape == (TH, TW, 8)
    index = bits(g[..., 7])
    hit = index != MISS
    hits = hit.astype(np.uint32)
    # the tile shows every kind of primitive, every material, and the background
    seen = prims[index[hit]]
    assert 0.2 < hit.mean() < 1.0 and (~hit).sum() >= 8
    assert sorted(np.unique(seen["category"])) == [0, 1, 2] and sorted(np.unique(seen["data4"][:, 2])) == [0, 1, 2]

    # crt_render_aovs
    assert np.array_equal(aov["hits"], hits)
    assert np.array_equal(bits(aov["alpha"]), bits(hits.astype(np.float32)))
    assert np.array_equal(bits(aov["depth"])[hit], bits(g[..., 0])[hit])
    assert (bits(aov["depth"])[~hit] == bits(aov_ref.INF)).all()
    # the plane is (+0 + n) / 1 by its definition: the G-buffer's normal bit for bit, but for a component of -0 (a flipped
    # axis-aligned patch normal), which the sum from +0 turns into +0 -- so the bits of +0 + n, and the values of n
    assert np.array_equal(bits(aov["normal"][..., :3])[hit], bits(np.float32(0) + g[..., 4:7])[hit])
    assert np.array_equal(aov["normal"][..., :3][hit], g[..., 4:7][hit])

    # crt_render_mattes
    assert np.array_equal(prim["ids"][0], index)             # (a miss: MATTE_NONE, the G-buffer's own word)
    assert matte_ref.MISS == MISS and (prim["ids"][0][~hit] == MISS).all()
    assert np.array_equal(prim["counts"][0], hits) and np.array_equal(prim["hits"], hits) and not prim["overflow"].any()
    # (the denoiser's key plane cannot be read from Python: the key of the G-buffer's primitive, formed from its record)
    assert np.array_equal(mat["ids"][0], matte_ref.hit_ids(ps, index, matte_ref.MATERIAL))
    assert np.array_equal(mat["counts"][0], hits) and not mat["overflow"].any()

    # crt_pick: the G-buffer's record where the ray hits; at a miss `hit` and `prim` only (t is the ray's own limit)
    f = hit.ravel()
    rec = g.reshape(-1, 8)
    assert np.array_equal(pick["hit"], hits.ravel())
    assert np.array_equal(pick["prim"], index.ravel())
    assert np.array_equal(bits(pick["t"])[f], bits(rec[:, 0])[f])
    assert np.array_equal(bits(pick["position"][:, :3])[f], bits(rec[:, 1:4])[f])
    assert np.array_equal(bits(pick["normal"][:, :3])[f], bits(rec[:, 4:7])[f])


def test_the_two_render_calls_share_their_refusals():
    """No scene; n_samples = 0 with nothing in the accumulator; a sample range that passes 2^32 - 1: the same code and the
    same message but for the function's name.  (No test helper reaches the adaptive state's `broken` flag.)"""
    from computeraytracer_amd import Renderer, _lib
    plane = np.zeros((H, W), np.uint32)
    a_arg, m_arg = _lib.AovPlanes(hits=plane.ctypes.data), _lib.MattePlanes(hits=plane.ctypes.data)

    def both(r, n):
        out = []
        for name, call in (("crt_render_aovs", lambda: r._lib.crt_render_aovs(r._h, n, C.byref(a_arg))),
                           ("crt_render_mattes", lambda: r._lib.crt_render_mattes(r._h, n, 0, 1, C.byref(m_arg)))):
            rc = call()
            msg = (r._lib.crt_last_error(r._h) or b"").decode()
            assert name in msg, msg
            out.append((rc, msg.replace(name, "<call>")))
        assert out[0] == out[1], out
        return out[0]

    with Renderer(0) as r:
        rc, msg = both(r, 1)
        assert rc == ESTATE and "scene" in msg                                   # no scene
        r.upload(mixed_scene()).build_accel("bvh2")
        rc, msg = both(r, 0)
        assert rc == ESTATE and "holds none" in msg                              # nothing traced, and n_samples = 0
        r.set_sample_offset(0xFFFFFFF0)
        rc, msg = both(r, 16)
        assert rc == EINVAL and "2^32 - 1" in msg                                # B + n = 2^32
        assert r._lib.crt_render_aovs(r._h, 15, C.byref(a_arg)) == 0 and r._lib.crt_render_mattes(r._h, 15, 0, 1, C.byref(m_arg)) == 0
