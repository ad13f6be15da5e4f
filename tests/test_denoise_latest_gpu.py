"""GPU tests of crt_denoise_latest (include/crt.h "Denoised preview"; run with -m gpu on an MI355X): the
filtered frame of the newest complete sample index s, taken without a flush.  Every comparison is bit for bit against
crt_denoise on a second context that holds exactly s samples after crt_sync.  Cornell at 72 x 61: partial 16 x 16 and
8 x 8 blocks on both axes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 72, 61
DEFAULTS = (5, 1.0, 0.5, 0.3)
PARAM_SETS = ((0, 1.0, 0.5, 0.3), DEFAULTS, (10, 0.7, 0.4, 0.2))
EINVAL, ESTATE, ENOMEM = -1, -3, -4
PIPELINE_DEFAULTS = {"wf_pipes": 2, "wf_ring": 32, "wf_cohort": 16, "frame_ring": 0, "wf_defer": 1, "pipeline": 1,
                     "denoise_latest_wave_blocks": 0}


def _scene():
    from computeraytracer_amd import cornell
    return cornell(W, H)


def _cams():
    from computeraytracer_amd.scene import orbit_cameras
    return orbit_cameras(_scene().camera, 64)[:2]


def latest(r, params=DEFAULTS, shape=(H, W)):
    """The raw call into sentinel-filled buffers: (code, rgb, rgba8, s); s = 0xFFFFFFFF where the call did not write it."""
    from computeraytracer_amd._lib import DenoiseParams
    rgb = np.full(shape + (4,), -7.0, np.float32)
    rgba = np.full(shape + (4,), 0x5A, np.uint8)
    s = C.c_uint32(0xFFFFFFFF)
    p = DenoiseParams(*params) if params is not None else None
    rc = r._lib.crt_denoise_latest(r._h, C.byref(p) if p is not None else None, rgb.ctypes.data, rgba.ctypes.data, C.byref(s))
    return rc, rgb, rgba, s.value


def untouched(rgb, rgba):
    return bool((rgb == -7.0).all() and (rgba == 0x5A).all())


def same(got_rgb, got_rgba, want):
    return np.array_equal(got_rgba, want[0]) and np.array_equal(got_rgb.view(np.uint32), want[1].view(np.uint32))


class Reference:
    """A second context of the same scene: crt_denoise and crt_read_accum of exactly s samples after crt_sync, per camera,
    each computed once."""

    def __init__(self):
        from computeraytracer_amd import Renderer
        self.r = Renderer(0)
        self.r.upload(_scene()).build_accel("bvh2")
        self.cams = _cams()
        self.cam, self.have = 0, 0
        self.r.set_camera(self.cams[0])
        self.filtered, self.accums = {}, {}

    def _goto(self, cam, s):
        if cam != self.cam:
            self.r.set_camera(self.cams[cam])
            self.cam, self.have = cam, 0
        if s < self.have:
            self.r.reset()
            self.have = 0
        if s > self.have:
            self.r.frame(s - self.have).sync()
            self.have = s
        assert self.r.sample == s

    def denoise(self, s, params=DEFAULTS, cam=0):
        """(rgba8, rgb) of crt_denoise at exactly s samples."""
        key = (cam, s, params)
        if key not in self.filtered:
            self._goto(cam, s)
            self.filtered[key] = self.r.denoise(*params, rgb=True)
        return self.filtered[key]

    def accum(self, s, cam=0):
        if (cam, s) not in self.accums:
            self._goto(cam, s)
            self.accums[(cam, s)] = self.r.read_accum()
        return self.accums[(cam, s)]


@pytest.fixture(scope="module")
def reference():
    ref = Reference()
    yield ref
    ref.r.close()


@pytest.fixture()
def live():
    """A fresh context of the scene with the driver's default options."""
    from computeraytracer_amd import Renderer
    with Renderer(0) as r:
        r.upload(_scene()).build_accel("bvh2").set_camera(_cams()[0])
        try:
            yield r
        finally:
            r.set_option("debug_fail_alloc", 0)


# ------------------------------------------------------------------ 1. no flush, deterministically
@pytest.mark.parametrize("wave_blocks", [0, 1])
def test_pending_samples_stay_unpublished(live, reference, wave_blocks):
    """16 samples synced, then five crt_trace(1) calls that the cohort of 16 keeps merged and unpublished: the call shows
    sample 16 whatever the timing, leaves the five where they are, and a later crt_sync gives the plain 21-sample render."""
    live.set_option("wf_defer", 1).set_option("wf_cohort", 16).set_option("denoise_latest_wave_blocks", wave_blocks)
    live.frame(16).sync()
    for _ in range(5):
        live.frame(1)
    rc, rgb, rgba, s = latest(live)
    assert (rc, s) == (0, 16)
    assert live.sample == 21 and live.latest_sample == 16
    assert same(rgb, rgba, reference.denoise(16))
    live.sync()
    assert live.latest_sample == 21
    assert np.array_equal(live.read_accum().view(np.uint32), reference.accum(21).view(np.uint32))


# ------------------------------------------------------------------ 2. batches in flight
@pytest.mark.parametrize("option,value", [("wf_pipes", 1), ("wf_pipes", 3), ("wf_ring", 2)])
def test_batches_in_flight(live, reference, option, value):
    want = {s: reference.denoise(s) for s in range(1, 41)}
    acc40 = reference.accum(40)
    live.set_option("wf_defer", 1).set_option("wf_cohort", 1).set_option(option, value)
    last, log = 0, []
    for k in range(1, 41):
        live.frame(1)
        if k % 4:
            continue
        rc, rgb, rgba, s = latest(live)
        log.append((k, rc, s))
        if rc == ESTATE:
            assert s == 0 and last == 0 and untouched(rgb, rgba), log
            continue
        assert rc == 0 and 1 <= s <= k and last <= s, log
        last = s
        assert same(rgb, rgba, want[s]), log
    print(log)
    assert live.sample == 40
    live.sync()
    assert np.array_equal(live.read_accum().view(np.uint32), acc40.view(np.uint32))
    rc, rgb, rgba, s = latest(live)
    assert (rc, s) == (0, 40) and same(rgb, rgba, want[40])


# ------------------------------------------------------------------ 3. random walk
@pytest.mark.parametrize("seed", [20261020, 7])
def test_random_walk(live, reference, seed):
    """Seeded sequences of small crt_trace calls, the non-flushing reads and the sync points in between, over random driver
    settings: every filtered frame handed out is crt_denoise of its own sample index, the indices never go back between
    resets, and zero iterations are the bytes crt_read_latest_rgba8 shows for the same index."""
    from computeraytracer_amd._lib import CrtError
    rng = np.random.default_rng(seed)
    cams = _cams()
    cam, total, seen, log = 0, 0, 0, []
    try:
        for step in range(300):
            if step % 60 == 0:
                opts = {"wf_pipes": int(rng.choice([1, 2, 3])), "wf_ring": int(rng.choice([2, 3, 32])),
                        "wf_cohort": int(rng.choice([1, 4, 16])), "denoise_latest_wave_blocks": int(rng.choice([0, 1]))}
                for k, v in opts.items():
                    live.set_option(k, v)                       # (each a flush)
                seen = total
                log.append(("options", opts))
            what = rng.random()
            if what < 0.4:
                n = int(rng.integers(1, 4))
                if total + n > 40:
                    live.reset()
                    total = seen = 0
                    log.append(("reset",))
                live.frame(n)
                total += n
                log.append(("trace", n))
            elif what < 0.7:
                params = PARAM_SETS[int(rng.integers(0, 3))]
                rc, rgb, rgba, s = latest(live, params)
                log.append(("denoise_latest", params[0], rc, s))
                if rc == ESTATE:
                    assert s == 0 and seen == 0 and untouched(rgb, rgba), log[-12:]
                    continue
                assert rc == 0 and max(seen, 1) <= s <= total, log[-12:]
                seen = s
                assert same(rgb, rgba, reference.denoise(s, params, cam)), log[-12:]
                if params[0] == 0:
                    img, s2 = live.read_latest_rgba8()
                    assert s <= s2 <= total
                    seen = s2
                    if s2 == s:
                        assert np.array_equal(img, rgba), log[-12:]
            elif what < 0.76:
                img, s = live.read_latest_rgba8()
                log.append(("read_latest", s))
                assert seen <= s <= total, log[-12:]
                seen = s
                if s:
                    assert np.array_equal(img, reference.denoise(s, PARAM_SETS[0], cam)[0]), log[-12:]
            elif what < 0.82:
                s = live.latest_sample
                log.append(("latest_sample", s))
                assert seen <= s <= total, log[-12:]
                seen = s
            elif what < 0.88:
                log.append(("denoise", total))
                if total == 0:
                    with pytest.raises(CrtError):
                        live.denoise()
                    continue
                rgba, rgb = live.denoise(rgb=True)
                assert same(rgb, rgba, reference.denoise(total, DEFAULTS, cam)), log[-12:]
                seen = total
            elif what < 0.93:
                live.sync()
                log.append(("sync", total))
                assert live.latest_sample == total
                seen = total
            elif what < 0.96:
                live.reset()
                total = seen = 0
                log.append(("reset",))
            else:
                cam = 1 - cam
                live.set_camera(cams[cam])
                total = seen = 0
                log.append(("set_camera", cam))
                assert live.sample == 0
        live.sync()
        assert live.sample == total
        if total:
            assert np.array_equal(live.read_accum().view(np.uint32), reference.accum(total, cam).view(np.uint32))
    finally:
        for k, v in PIPELINE_DEFAULTS.items():
            live.set_option(k, v)


# ------------------------------------------------------------------ 4. context variants: nothing in flight, the call is crt_denoise
def _equals_denoise(r, shape=(H, W), samples=4):
    rc, rgb, rgba, s = latest(r, DEFAULTS, shape)
    assert (rc, s) == (0, samples) and r.sample == samples
    rgba_d, rgb_d = r.denoise(rgb=True)
    assert same(rgb, rgba, (rgba_d, rgb_d))
    rc, rgb, rgba, s = latest(r, DEFAULTS, shape)                # (and with the G-buffer crt_denoise left)
    assert (rc, s) == (0, samples) and same(rgb, rgba, (rgba_d, rgb_d))
    return rgba_d, rgb_d


def test_tile_with_odd_origin_and_size(live):
    live.set_tile(5, 3, 5 + 43, 3 + 29).frame(4).sync()
    _equals_denoise(live, (29, 43))


def test_bound_output(live, reference):
    """The accumulator and the framebuffer in caller-owned device memory (here: a second context's tile buffers)."""
    from computeraytracer_amd import Renderer
    with Renderer(0) as other:
        other.upload(_scene()).reset().sync()                     # (its buffers: the tile's size, zeroed)
        live.bind_output(*other.device_buffers())
        try:
            live.frame(4).sync()
            assert same(*_equals_denoise(live)[::-1], reference.denoise(4))
            live.set_option("wf_cohort", 1)
            live.frame(1).frame(1).frame(1)                      # in flight, into the bound accumulator
            rc, rgb, rgba, s = latest(live)
            assert rc == 0 and 4 <= s <= 7 and same(rgb, rgba, reference.denoise(s))
            live.sync()
        finally:
            live.bind_output(None, None)


def test_frame_ring_on(live, reference):
    live.set_option("frame_ring", 8)
    live.frame(4).sync()
    assert same(*_equals_denoise(live)[::-1], reference.denoise(4))
    live.frame(1).frame(1)
    rc, rgb, rgba, s = latest(live)
    assert rc == 0 and s >= 4 and same(rgb, rgba, reference.denoise(s))
    assert np.array_equal(live.read_sample_rgba8(6), reference.denoise(6, PARAM_SETS[0])[0])     # the ring is intact


def test_pipeline_off(live, reference):
    live.set_option("pipeline", 0)
    live.frame(3).frame(1)                                       # (no sync: one stream, nothing deferred)
    assert same(*_equals_denoise(live)[::-1], reference.denoise(4))


def test_without_deferral(live, reference):
    live.set_option("wf_defer", 0)
    live.frame(4).sync()
    assert same(*_equals_denoise(live)[::-1], reference.denoise(4))


@pytest.mark.parametrize("mode", ["none", "lbvh", "ploc"])
def test_other_builders(live, reference, mode):
    live.build_accel(mode).frame(4)
    if mode != "none":
        live.sync()
    assert same(*_equals_denoise(live)[::-1], reference.denoise(4))


# ------------------------------------------------------------------ 5. refusals
def _refused(r, code, params=DEFAULTS, want_s=0xFFFFFFFF, shape=(H, W)):
    from computeraytracer_amd._lib import CrtError
    try:
        before = (r.sample, r.latest_sample)
    except CrtError:                                              # (the adaptive state has no sample count)
        before = None
    rc, rgb, rgba, s = latest(r, params, shape)
    assert rc == code and s == want_s and untouched(rgb, rgba), (rc, s, r._lib.crt_last_error(r._h))
    if before is not None:
        assert (r.sample, r.latest_sample) == before


def test_refusals(reference):
    from computeraytracer_amd import Renderer
    ps = _scene()
    with Renderer(0) as r:
        _refused(r, ESTATE)                                       # no scene
        r.upload(ps)
        _refused(r, ESTATE)                                       # no tree
        r.build_accel("bvh2").set_camera(_cams()[0])
        _refused(r, ESTATE, want_s=0)                             # sample 0
        r.frame(1)                                                # (requested, merged, unpublished: still no complete frame)
        _refused(r, ESTATE, want_s=0)
        assert r.sample == 1
        r.frame(3).sync()
        for bad in ((11, 1.0, 0.5, 0.3), (5, float("nan"), 0.5, 0.3), (5, 1.0, float("inf"), 0.3), (5, 1.0, 0.5, 0.0), (5, 1.0, 0.5, -1.0)):
            _refused(r, EINVAL, bad)
        rc, rgb, rgba, s = latest(r, None)                        # NULL = the defaults
        assert (rc, s) == (0, 4) and same(rgb, rgba, reference.denoise(4))
        assert r._lib.crt_denoise_latest(r._h, None, None, None, None) == 0     # every output may be NULL
        r.update_primitives(0, ps.primitives[:1])
        _refused(r, ESTATE)                                       # a stale tree
        r.refit_accel()
        assert r.trace_adaptive(samples=4, min_samples=4) > 0
        _refused(r, ESTATE)                                       # the adaptive state
        r.reset()
        r.set_row_bands(8, 2, 1).frame(2).sync()
        _refused(r, ESTATE, shape=tuple(r.tile[:1:-1]))           # row bands
        r.set_tile(0, 0, W, H).frame(4).sync()
        rc, rgb, rgba, s = latest(r)
        assert (rc, s) == (0, 4) and same(rgb, rgba, reference.denoise(4))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_failed_allocation_on_a_fresh_context(live, reference, k):
    """The call's five allocations on a context that has filtered nothing yet (G-buffer, keys, two colour buffers, rgba8):
    whichever fails, nothing is written, the pipeline state stays, and the next call succeeds.  There is no sixth."""
    live.frame(4).sync()
    live.frame(1)                                                 # (pending: the refused call must not publish it)
    live.set_option("debug_fail_alloc", k)                        # (a flush: sample 5 is complete from here on)
    if k <= 5:
        _refused(live, ENOMEM)
        live.set_option("debug_fail_alloc", 0)
    rc, rgb, rgba, s = latest(live)
    live.set_option("debug_fail_alloc", 0)
    assert (rc, s) == (0, 5) and same(rgb, rgba, reference.denoise(5))


# ------------------------------------------------------------------ 6. the temporal history
def _temporal_sequence(middle):
    """crt_denoise_temporal on frame 0, `middle` on frame 1, then frame 1's and frame 2's crt_denoise_temporal."""
    from computeraytracer_amd import Renderer
    cams = _cams()
    out = []
    with Renderer(0) as r:
        try:
            r.upload(_scene()).build_accel("bvh2").set_camera(cams[0]).frame(4).sync()
            r.denoise_temporal()
            r.set_camera(cams[1]).set_sample_offset(4).frame(4).sync()
            if middle:
                middle(r)
            out += list(r.denoise_temporal(rgb=True, history=True))
            r.set_camera(cams[0]).set_sample_offset(8).frame(4).sync()
            if middle:
                middle(r)
            out += list(r.denoise_temporal(rgb=True, history=True))
        finally:
            r.set_option("debug_fail_alloc", 0)
    return out


@pytest.fixture(scope="module")
def temporal_alone():
    return _temporal_sequence(None)


def _assert_same_sequence(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def test_temporal_history_untouched(temporal_alone):
    def middle(r):
        rc, _, _, s = latest(r)
        assert (rc, s) == (0, 4)
        assert latest(r, PARAM_SETS[2])[0] == 0
    _assert_same_sequence(_temporal_sequence(middle), temporal_alone)


@pytest.mark.parametrize("k", [1, 2])
def test_failed_allocation_leaves_the_history(temporal_alone, k):
    """After a camera move the G-buffer goes into a guide set that no slot names: two allocations beside a valid history."""
    def middle(r):
        r.set_option("debug_fail_alloc", k)
        _refused(r, ENOMEM)
        r.set_option("debug_fail_alloc", 0)
        rc, _, _, s = latest(r)
        assert (rc, s) == (0, 4)
    _assert_same_sequence(_temporal_sequence(middle), temporal_alone)
