"""CPU side of the radiance queries' tests (include/crt.h "Radiance queries"): what makes the ray set of
tests/radiance_ref.py worth tracing, asserted on the oracle alone, and the parts of the Python wrapper that need no
device."""
import numpy as np
import pytest

import radiance_ref as R
from material_matrix_scenes import NAMES

F = np.float32


def test_every_probe_has_the_pad_of_the_uploaded_scene(orc):
    """The pad is part of the triangles' acceptance rule and the call takes it from the context's camera: the scene is
    uploaded with probe 0's camera, so every probe camera's pad must be that one."""
    for name in R.SCENES:
        ps = R.scene(name)
        up = orc.Scene.from_packed(ps).hit_pad()
        for p in R.PROBES + (R.EXTRA,):
            assert orc.Scene.from_packed(R.with_probe(ps, p)).hit_pad() == up, (name, p)
    # (cornell's own eye at z = -800 gives another pad: why the scene's own camera is not the one uploaded)
    from computeraytracer_amd import cornell
    assert orc.Scene.from_packed(cornell(R.W, R.H)).hit_pad() != orc.Scene.from_packed(R.scene("patch")).hit_pad()


def test_the_ray_set_reaches_what_it_is_made_for(orc):
    n = first = 0
    mat, segs, nan, walked = [], [], [], []
    for name in NAMES:
        ps, rs = R.rays_of(orc, name)
        assert len(rs.o) == 4 * 2 * 12 * 12 == 1152
        mat.append(R.materials(ps, rs.first)); segs.append(rs.segments); nan.append(np.isnan(rs.xyz).any(axis=1)); walked.append(rs.finite)
    mat, segs, nan, walked = (np.concatenate(v) for v in (mat, segs, nan, walked))
    counts = {m: int((mat == m).sum()) for m in (0, 1, 2, -1)}
    print(f"first hits by material {counts}; paths of four or more segments {int((segs >= 4).sum())}; longest {int(segs.max())}; "
          f"NaN results {int(nan.sum())}; rays the definition walks {int(walked.sum())} of {len(walked)}")
    assert all(counts[m] >= 200 for m in (0, 1, 2)), counts
    assert counts[-1] >= 200, counts
    assert (segs >= 4).sum() >= 200
    assert segs.max() >= 101, "no path reaches the depth cap (kMaxDepthPath = 100: 101 extension rays)"
    assert nan.sum() >= 5
    # ... and among the rays the kernel walks (probe 2's directions are NaN: zeros by definition, radiance_ref.expected)
    assert all(int(((mat == m) & walked).sum()) >= 200 for m in (0, 1, 2, -1))
    assert ((segs >= 4) & walked).sum() >= 200 and (nan & walked).sum() >= 5
    # (the paths that reach the depth cap are probe 2's: a NaN ray passes every patch's test for ever.  No walked ray of
    # the set gets there -- roulette ends a finite path long before; measured: 11 segments at the most)
    print(f"among the walked rays: longest path {int(segs[walked].max())} segments")
    # ... which is what the DEEP probe is for: walked paths that do reach the cap, some that leave the sphere beside them
    _, deep = R.deep_rays(orc)
    at_cap = deep.segments == 101
    print(f"the deep probe: {int(at_cap.sum())} of {len(at_cap)} paths reach the depth cap, {int((deep.xyz != 0).any(axis=1).sum())} carry light")
    assert deep.finite.all() and at_cap.sum() >= 100 and (~at_cap).sum() >= 20 and (deep.xyz != 0).any(axis=1).sum() >= 5
    assert deep.pads[0] == orc.Scene.from_packed(R.scene("sphere_only")).hit_pad()
    assert not walked.all(), "the set holds no non-finite caller ray any more: say so where expected() is described"
    # the extra probe looks up with finite rays
    for name in NAMES:
        _, ex = R.rays_of(orc, name, extra=True)
        assert ex.finite.all() and ex.d[:, 1].min() > 0.5


def test_two_discarded_draws_put_the_stream_where_path_trace_starts(orc):
    """rand_kat(x, y, s, 2) is the state after the camera's two jitter draws; the next draw is sample_wavelengths'."""
    ps = R.scene("patch")
    sc = orc.Scene.from_packed(ps)
    for x, y, s in [(0, 0, 1), (5, 7, 1), (23, 23, 7), (11, 2, 0xFFFFFFFF), (3, 19, 0)]:
        _, seed = orc.rand_kat(x, y, s, 2)
        tr = sc.trace_pixel(x, y, s)
        assert R.wavelengths_after(seed) == list(tr.wavelengths), (x, y, s)
        # (the restated generator is the oracle's)
        out, seed3 = orc.rand_kat(x, y, s, 3)
        assert R.pcg4d(seed) == [int(v) for v in seed3] and (R.pcg4d(seed)[0] & 0xFFFFFF) == int(out[2])


def test_path_keys_are_16_byte_records():
    from computeraytracer_amd import _lib
    from computeraytracer_amd.renderer import PATH_KEY_DTYPE, pack_keys
    import ctypes as C
    assert PATH_KEY_DTYPE.itemsize == 16 == C.sizeof(_lib.PathKey)
    assert [PATH_KEY_DTYPE.fields[f][1] for f in ("x", "y", "first_sample", "reserved")] == [0, 4, 8, 12]
    assert [getattr(_lib.PathKey, f).offset for f in ("x", "y", "first_sample", "reserved")] == [0, 4, 8, 12]
    k = pack_keys([1, 2, 0xFFFFFFFF], [4, 5, 6], 7)
    assert k.dtype == PATH_KEY_DTYPE and k.shape == (3,)
    assert k.view(np.uint32).reshape(3, 4).tolist() == [[1, 4, 7, 0], [2, 5, 7, 0], [0xFFFFFFFF, 6, 7, 0]]
    assert pack_keys([1, 2], 0, [3, 0xFFFFFFFE]).view(np.uint32).reshape(2, 4).tolist() == [[1, 0, 3, 0], [2, 0, 0xFFFFFFFE, 0]]
    assert len(pack_keys([], [], 1)) == 0
    for bad in (([-1], [0], 1), ([0], [1 << 32], 1), ([0], [0], -2)):
        with pytest.raises(ValueError, match="unsigned 32-bit"):
            pack_keys(*bad)
    assert _lib.RadiancePlanes._fields_ == [("xyz", C.c_void_p), ("y2", C.c_void_p), ("rgba8", C.c_void_p)]
    assert all(n in _lib.SIGNATURES for n in ("crt_radiance_rays", "crt_radiance_rays_device"))


def test_wrapper_checks_that_need_no_device():
    from computeraytracer_amd.renderer import Renderer
    with pytest.raises(ValueError, match="n_samples"):
        Renderer._radiance_args(0, None)
    with pytest.raises(ValueError, match="n_samples"):
        Renderer._radiance_args(1 << 32, None)
    with pytest.raises(ValueError, match="unknown planes"):
        Renderer._radiance_args(1, ("xyz", "t"))
    with pytest.raises(ValueError, match="no plane"):
        Renderer._radiance_args(1, ())
    assert Renderer._radiance_args(3, None) == (3, ["xyz", "y2", "rgba8"])
    assert Renderer._radiance_args(1, ("rgba8", "xyz")) == (1, ["xyz", "rgba8"])
    r = object.__new__(Renderer)                                 # (no context: the checks below come before any call into the library)
    r._h = None
    with pytest.raises(ValueError, match="same length"):
        r.radiance_rays(np.zeros((2, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError, match="n_samples"):
        r.radiance_rays(np.zeros((2, 3)), np.zeros((2, 3)), n_samples=0)
    with pytest.raises(ValueError, match="keys for"):
        r.radiance_rays(np.zeros((2, 3)), np.ones((2, 3)), keys=np.zeros((3, 4), np.uint32))
    with pytest.raises(ValueError, match="integer array"):
        r.radiance_rays(np.zeros((2, 3)), np.ones((2, 3)), keys=np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="at least 1"):
        Renderer.panorama_rays(0, 4, (0, 0, 0))


def test_panorama_mapping():
    """The docstring's mapping: the centre looks along +z, the right half towards +x, the top towards +y; unit vectors."""
    from computeraytracer_amd.renderer import Renderer
    w, h = 16, 8
    rays, keys = Renderer.panorama_rays(w, h, (1, 2, 3), first_sample=5)
    assert len(rays) == len(keys) == w * h
    d = rays["d"].reshape(h, w, 3)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1).max() < 2e-7
    assert (rays["o"] == np.array([1, 2, 3], F)).all() and (rays["exclude"] == 0xFFFFFFFF).all() and (rays["t_max"] == R.NO_LIMIT).all()
    assert (d[:, w // 2:, 0] > 0).all() and (d[:, :w // 2, 0] < 0).all()
    assert (d[:h // 2, :, 1] > 0).all() and (d[h // 2:, :, 1] < 0).all()
    mid = d[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1].mean(axis=(0, 1))
    assert mid[2] > 0.9 and abs(mid[0]) < 1e-6 and abs(mid[1]) < 1e-6
    k = keys.view(np.uint32).reshape(h, w, 4)
    assert (k[..., 0] == np.arange(w)[None, :]).all() and (k[..., 1] == np.arange(h)[:, None]).all() and (k[..., 2] == 5).all()


def test_the_excluded_ceiling_has_a_light_behind_it(orc):
    ps, o, d, ex, keys, xyz, ceiling, lights = R.behind_the_ceiling(orc)
    print(f"{len(o)} rays through ceiling {ceiling} onto lights {lights}")
    assert len(o) >= 50 and len(lights) == 2 and (ex == ceiling).all()
    assert len({tuple(k) for k in keys.tolist()}) >= 10 and (xyz[:, 1] > 0).all()


def test_the_oracle_as_a_tone_map(orc):
    """oracle_rgba8(sums, n) of the oracle's own accumulator is the oracle's own frame."""
    sc = orc.Scene.from_packed(R.scene("patch"))
    for n in (1, 5):
        acc, img, _ = sc.render(n)
        assert np.array_equal(R.oracle_rgba8(orc, acc.reshape(-1, 4), n), img.reshape(-1, 4)) and img[..., :3].any()
