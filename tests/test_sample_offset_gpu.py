"""GPU tests of the sample offset (include/crt.h "Sample offset"; run with -m gpu on an MI355X): with
offset B a frame of n samples is the oracle's samples B+1 .. B+n summed into a zero accumulator, bit for bit, while
everything that counts samples -- the tone map's divisor, crt_sample_count, the frame ring -- counts from the reset."""
import numpy as np
import pytest

from conftest import bits
from test_adaptive_gpu import FORMS, options

pytestmark = pytest.mark.gpu
WAVEFRONT = [f for f, (mode, o) in FORMS.items() if mode != "none" and o.get("pipeline", 1) == 1]
W, H = 40, 28                                                # ragged 8x8 tiles on both edges


@pytest.fixture(scope="module")
def scene(orc):
    from computeraytracer_amd import cornell
    ps = cornell(W, H)
    return ps, orc.Scene.from_packed(ps)


def _want(sc, g, B, n):
    """The oracle's frame of samples B+1 .. B+n: its accumulator, and the rgba8 tone-mapped with n."""
    acc = sc.render(n, first_sample=B + 1)[0]
    return acc, sc.denoise(acc, n, g, iterations=0)[1]


def test_the_wavefront_forms_are_the_ones_expected():
    assert sorted(WAVEFRONT) == ["batches-in-flight", "wavefront-bvh2", "wavefront-lbvh", "wf_pipes1"]


@pytest.mark.parametrize("form", WAVEFRONT)
@pytest.mark.parametrize("B", [0, 4, 1000])
def test_offset_frames_are_the_oracles_samples(renderer, scene, form, B):
    ps, sc = scene
    mode, opts = FORMS[form]
    try:
        options(renderer, **opts)
        renderer.upload(ps).build_accel(mode)
        assert renderer.sample_offset == 0
        for n in (1, 5, 17):
            renderer.reset().set_sample_offset(B)
            assert renderer.sample_offset == B
            renderer.frame(n).sync()
            acc, rgba, g = renderer.read_accum(), renderer.read_rgba8(), renderer.read_gbuffer()
            want_acc, want_rgba = _want(sc, g, B, n)
            assert renderer.sample == n
            assert np.array_equal(bits(acc)[..., :3], bits(want_acc)[..., :3]), f"B {B}, n {n}: accumulator differs from the oracle"
            assert np.array_equal(rgba, want_rgba), f"B {B}, n {n}: rgba8 is not the tone map with n"
            # two calls of n / 2 are one of n (the offset persists over the reset)
            renderer.reset()
            assert renderer.sample_offset == B
            if n // 2:
                renderer.frame(n // 2)
            renderer.frame(n - n // 2).sync()
            assert np.array_equal(bits(renderer.read_accum()), bits(acc)) and np.array_equal(renderer.read_rgba8(), rgba)
    finally:
        renderer.reset().set_sample_offset(0)
        options(renderer)


@pytest.mark.parametrize("form", WAVEFRONT)
def test_the_frame_ring_is_indexed_by_count(renderer, scene, form):
    ps, sc = scene
    mode, opts = FORMS[form]
    B, n = 1000, 5
    try:
        options(renderer, **opts)
        renderer.upload(ps).build_accel(mode).set_option("frame_ring", 8)
        renderer.reset().set_sample_offset(B).frame(n).sync()
        g = renderer.read_gbuffer()
        for s in range(1, n + 1):
            assert np.array_equal(renderer.read_sample_rgba8(s), _want(sc, g, B, s)[1]), f"frame {s} of the ring"
        assert renderer.latest_sample == n
    finally:
        renderer.set_option("frame_ring", 0)
        renderer.reset().set_sample_offset(0)
        options(renderer)


def test_offset_rules():
    """CRT_ESTATE / CRT_EINVAL of crt_set_sample_offset and of crt_trace under an offset, the context unchanged after
    each; what the offset persists over; crt_write_accum continues at B + s + 1.  On a context of its own."""
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import CrtError
    from oracle import orc
    ps = cornell(W, H)
    sc = orc.Scene.from_packed(ps)
    B = 4

    def refused(fn, code):
        with pytest.raises(CrtError) as e:
            fn()
        assert e.value.code == code

    with Renderer(0) as r:
        r.set_sample_offset(7)                                 # before any scene: allowed; the upload returns it to 0
        r.upload(ps).build_accel("bvh2")
        assert r.sample_offset == 0
        r.set_sample_offset(B).frame(3).sync()
        acc3 = r.read_accum()
        refused(lambda: r.set_sample_offset(9), -3)            # not at sample 0
        assert r.sample_offset == B and r.sample == 3 and np.array_equal(bits(r.read_accum()), bits(acc3))
        r.set_camera(ps.camera)                                # the edits keep it
        assert r.sample_offset == B and r.sample == 0
        r.build_accel("lbvh")
        assert r.sample_offset == B
        # a restored accumulator continues at index B + s + 1
        r.write_accum(acc3, 3).frame(2).sync()
        want = sc.render(5, first_sample=B + 1)[0]
        assert r.sample == 5 and np.array_equal(bits(r.read_accum())[..., :3], bits(want)[..., :3])
        # the adaptive state and the forms without the wavefront pipeline refuse an offset
        r.reset()
        refused(lambda: r.trace_adaptive(samples=2), -3)
        assert r.sample == 0 and r.sample_offset == B
        r.set_option("pipeline", 0)
        refused(lambda: r.frame(1), -3)
        assert r.sample == 0 and not r.read_accum().any()
        r.set_option("pipeline", 1).build_accel("none")
        refused(lambda: r.frame(1), -3)
        assert r.sample == 0 and not r.read_accum().any()
        r.set_sample_offset(0).frame(2).sync()                 # offset 0 is the behaviour without the call, in every form
        assert np.array_equal(bits(r.read_accum())[..., :3], bits(sc.render(2)[0])[..., :3])
        r.set_option("pipeline", 0).build_accel("bvh2").reset().frame(2).sync()
        assert np.array_equal(bits(r.read_accum())[..., :3], bits(sc.render(2)[0])[..., :3])
        r.set_option("pipeline", 1).reset()
        assert r.trace_adaptive(samples=2, min_samples=2) > 0
        refused(lambda: r.set_sample_offset(1), -3)            # not in the adaptive state
        r.reset()
        # B + the samples requested may not pass 2^32 - 1
        top = 0xFFFFFFFF - 3
        r.set_sample_offset(top)
        refused(lambda: r.frame(4), -1)
        assert r.sample == 0 and r.sample_offset == top and not r.read_accum().any()
        r.frame(2).sync()
        refused(lambda: r.frame(2), -1)                        # 2 so far + 2 more
        assert r.sample == 2
        r.frame(1).sync()                                      # index 2^32 - 1 itself is drawn
        assert r.sample == 3
