"""GPU tests of adaptive sampling (include/crt.h "Adaptive sampling"; run with -m gpu on an MI355X).

Sample s of pixel (x, y) depends on (x, y, s) only, so after every round each pixel holds the oracle's accumulator and
rgba8 at its tile's count, bit for bit; the counts and errors equal the numpy restatement (tests/adaptive_ref.py) of the
per-sample Y, which the oracle gives as orc.render(1, first_sample=s) into a zero accumulator."""
import numpy as np
import pytest

import adaptive_ref as ref
from conftest import bits

pytestmark = pytest.mark.gpu
F = np.float32
DEFAULTS = dict(pipeline=1, quantize=1, wf_width=4, wf_trace_form=2, wf_pipes=2, spp_per_launch=0)
FORMS = {"wavefront-bvh2": ("bvh2", {}), "wavefront-lbvh": ("lbvh", {}), "wf_pipes1": ("bvh2", dict(wf_pipes=1)),
         "pipeline0": ("bvh2", dict(pipeline=0)), "accel-none": ("none", {}),
         "batches-in-flight": ("bvh2", dict(spp_per_launch=2))}


def options(r, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        r.set_option(k, v)


class Truth:
    """The oracle's view of one context: full-frame renders cut to the context's pixels (rows: its global rows, in local
    order; cols: its columns), the per-sample Y and their running sums S, Q."""

    def __init__(self, orc, ps, rows=None, cols=None):
        self.sc = orc.Scene.from_packed(ps)
        W, H = self.sc.width, self.sc.height
        self.rows = np.arange(H) if rows is None else np.asarray(rows)
        self.cols = np.arange(W) if cols is None else np.asarray(cols)
        self.rect = (int(self.cols[0]), int(self.rows.min()), int(self.cols[-1]) + 1, int(self.rows.max()) + 1)
        self.exp_ = lambda x: orc.math_eval("exp", np.asarray(x, F))
        self._frames = {}
        self.S, self.Q = [np.zeros((len(self.rows), len(self.cols)), F)], [np.zeros((len(self.rows), len(self.cols)), F)]

    def _cut(self, a):
        return a[self.rows][:, self.cols]

    def frame(self, n):
        if n not in self._frames:
            acc, rgba, _ = self.sc.render(n, rect=self.rect)
            self._frames[n] = (self._cut(acc), self._cut(rgba))
        return self._frames[n]

    def sums(self, counts):
        """S, Q per pixel at its tile's count."""
        npx = ref.pixel_counts(counts, *self.S[0].shape)
        while len(self.S) <= int(npx.max()):
            acc, _, _ = self.sc.render(1, first_sample=len(self.S), rect=self.rect)
            s, q = ref.accumulate(self._cut(acc)[None, ..., 1], self.S[-1], self.Q[-1])
            self.S.append(s)
            self.Q.append(q)
        S, Q = np.stack(self.S), np.stack(self.Q)
        ii, jj = np.indices(npx.shape)
        return S[npx, ii, jj], Q[npx, ii, jj]

    def errors(self, counts):
        return ref.tile_errors(*self.sums(counts), counts, self.exp_)

    def check(self, r, counts):
        """accum and rgba8 of every pixel = the oracle at its tile's count; errors = the restatement."""
        acc, rgba = r.read_accum(), r.read_rgba8()
        npx = ref.pixel_counts(counts, *acc.shape[:2])
        for n in np.unique(npx):
            m = npx == n
            if n == 0:
                assert not bits(acc)[m][:, :3].any() and not rgba[m].any()
                continue
            acc_o, rgba_o = self.frame(int(n))
            bad = (bits(acc)[m][:, :3] != bits(acc_o)[m][:, :3]).any(-1)
            assert not bad.any(), f"{int(bad.sum())} accumulator pixels at count {n} differ"
            assert np.array_equal(rgba[m], rgba_o[m]), f"rgba8 at count {n} differs"
        _, errors = r.read_adaptive()
        want = self.errors(counts)
        assert np.array_equal(errors.view(np.uint32), want.view(np.uint32)), \
            f"{int((errors != want).sum())} tile errors differ from the restatement"


def run_rounds(r, truth, samples, min_samples, max_samples, rounds, first_threshold=None):
    """Rounds of trace_adaptive, each checked against the rule and the oracle.  The threshold is the median of the errors
    after the first round (tiles then retire at different rounds).  Returns the final counts."""
    thr = F(0.0) if first_threshold is None else F(first_threshold)
    counts, errors = np.zeros((0, 0), np.uint32), None
    for k in range(rounds):
        if k > 0:
            counts, errors = r.read_adaptive()
            if k == 1 and first_threshold is None:
                thr = F(np.median(errors[np.isfinite(errors)]))
            want = ref.active(counts, errors, min_samples, max_samples, thr)
        n = r.trace_adaptive(samples=samples, threshold=float(thr), min_samples=min_samples, max_samples=max_samples)
        after, _ = r.read_adaptive()
        if k == 0:
            want = np.ones(after.shape, bool)
            counts = np.zeros(after.shape, np.uint32)
        assert n == int(want.sum())
        assert np.array_equal(after, counts + samples * want.astype(np.uint32)), "the tiles that grew are not the rule's"
        truth.check(r, after)
        if n == 0:
            break
    return r.read_adaptive()[0], thr


# ------------------------------------------------------------------ 1 + 2. per tile, bit for bit, every form
@pytest.mark.parametrize("form", list(FORMS))
def test_rounds_bit_exact(renderer, orc, form):
    from computeraytracer_amd import cornell
    mode, opts = FORMS[form]
    ps = cornell(100, 76)                                     # ragged tiles on both edges
    truth = _truth(orc, ps)
    try:
        options(renderer, **opts)
        renderer.upload(ps).build_accel(mode)
        counts, thr = run_rounds(renderer, truth, 8, 8, 40, 6)
        assert len(np.unique(counts)) >= 3, "tiles should retire at different rounds"
    finally:
        renderer.reset()
        options(renderer)


_TRUTH = {}


def _truth(orc, ps, rows=None, cols=None):
    key = (ps.primitives.tobytes(), ps.camera.tobytes(), None if rows is None else tuple(rows), None if cols is None else tuple(cols))
    if key not in _TRUTH:
        _TRUTH[key] = Truth(orc, ps, rows, cols)
    return _TRUTH[key]


# ------------------------------------------------------------------ 3. triangles: a crop and row bands
def test_mesh_crop_and_row_bands(renderer, orc):
    from computeraytracer_amd.partition import band_rows
    from computeraytracer_amd.scenes_synth import mesh10k
    ps = mesh10k(128, 96)
    try:
        renderer.upload(ps).set_tile(30, 20, 94, 68).build_accel("bvh2")          # 64 x 48
        run_rounds(renderer, _truth(orc, ps, np.arange(20, 68), np.arange(30, 94)), 4, 4, 12, 4)
        renderer.set_row_bands(8, 3, 1)
        rows = band_rows(96, 3, 1, 8)
        run_rounds(renderer, _truth(orc, ps, rows, np.arange(128)), 4, 4, 12, 4)
    finally:
        renderer.set_tile(0, 0, 128, 96)
        renderer.reset()


# ------------------------------------------------------------------ 4. uniform equivalence
@pytest.mark.parametrize("pipeline", [1, 0])
def test_all_active_equals_uniform_frames(renderer, pipeline):
    from computeraytracer_amd import cornell
    ps = cornell(100, 76)
    try:
        options(renderer, pipeline=pipeline)
        renderer.upload(ps).build_accel("bvh2")
        for _ in range(3):
            assert renderer.trace_adaptive(samples=5, threshold=1e30, min_samples=1000, max_samples=0) == 13 * 10
        acc, rgba = renderer.read_accum(), renderer.read_rgba8()
        renderer.reset().frame(15).sync()
        assert np.array_equal(bits(acc)[..., :3], bits(renderer.read_accum())[..., :3])
        assert np.array_equal(rgba, renderer.read_rgba8())
    finally:
        renderer.reset()
        options(renderer)


# ------------------------------------------------------------------ 5. no wasted work
@pytest.mark.parametrize("pipeline", [1, 0])
def test_paths_counter_is_active_pixels_times_samples(renderer, pipeline):
    from computeraytracer_amd import cornell
    ps = cornell(100, 76)
    try:
        options(renderer, pipeline=pipeline)
        renderer.upload(ps).build_accel("bvh2")
        renderer.trace_adaptive(samples=8, threshold=1e30, min_samples=8)
        c0, e0 = renderer.read_adaptive()
        thr = float(np.median(e0))
        renderer.enable_counters(True).reset_counters()
        n = renderer.trace_adaptive(samples=4, threshold=thr, min_samples=8)
        c1, _ = renderer.read_adaptive()
        grew = ref.pixel_counts(c1, 76, 100) != ref.pixel_counts(c0, 76, 100)
        assert 0 < n < c0.size
        assert renderer.counters()["paths"] == int(grew.sum()) * 4
    finally:
        renderer.enable_counters(False)
        renderer.reset()
        options(renderer)


# ------------------------------------------------------------------ 6. converged
def test_converged_call_changes_nothing(renderer):
    from computeraytracer_amd import cornell
    ps = cornell(64, 48)
    try:
        renderer.upload(ps).build_accel("bvh2")
        rounds = 0
        while renderer.trace_adaptive(samples=8, threshold=0.05, min_samples=8, max_samples=48):
            rounds += 1
            assert rounds < 20
        counts, _ = renderer.read_adaptive()
        assert counts.max() <= 48 and counts.min() >= 8
        acc, rgba = renderer.read_accum(), renderer.read_rgba8()
        assert renderer.trace_adaptive(samples=8, threshold=0.05, min_samples=8, max_samples=48) == 0
        assert np.array_equal(bits(acc), bits(renderer.read_accum())) and np.array_equal(rgba, renderer.read_rgba8())
        assert np.array_equal(counts, renderer.read_adaptive()[0])
    finally:
        renderer.reset()


def test_nan_radiance_keeps_tiles_active_up_to_max(renderer, orc):
    """A NaN in the light's spectrum makes the paths that see the light NaN: such a pixel's e is NaN, its tile's E is
    +inf, and the rule keeps the tile active up to max_samples whatever the threshold, while tiles without a NaN pixel
    retire at min_samples.  After every round the accumulator equals crt_trace's at the tile's count (NaN for NaN), E is
    +inf exactly on the tiles with a NaN pixel, and elsewhere E equals the restatement of the oracle's samples.  (Where
    the oracle and crt_trace disagree about WHICH samples turn NaN -- a NaN spectrum is outside the bit-exact contract,
    which covers finite scenes -- only finite pixels are compared with the oracle.)"""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import PackedScene
    base = cornell(32, 24)
    lit = base.primitives["data4"][:, 2] == 1
    spectra = base.spectra.copy()
    spectra[int(base.primitives["data4"][lit][0, 0])] = np.nan
    ps = PackedScene(base.primitives, base.lights, base.camera, spectra, base.cie)
    truth = Truth(orc, ps)

    def same(a, o):
        return ((bits(a) == bits(o)) | (np.isnan(a) & np.isnan(o))).all()

    try:
        renderer.upload(ps).build_accel("bvh2")
        uniform = {}
        for c in (4, 8, 12):
            renderer.frame(4).sync()
            uniform[c] = renderer.read_accum()
        renderer.reset()
        counts = np.zeros((3, 4), np.uint32)
        for k in range(5):
            if k == 0:
                want = np.ones(counts.shape, bool)
            else:
                counts, errors = renderer.read_adaptive()
                want = ref.active(counts, errors, 4, 12, F(1e30))
            n = renderer.trace_adaptive(samples=4, threshold=1e30, min_samples=4, max_samples=12)
            assert n == int(want.sum())
            after, errors = renderer.read_adaptive()
            assert np.array_equal(after, counts + 4 * want.astype(np.uint32))
            acc = renderer.read_accum()
            npx = ref.pixel_counts(after, 24, 32)
            for c in np.unique(npx):
                m = npx == c
                assert same(acc[m][:, :3], uniform[int(c)][m][:, :3]), f"accumulator at count {c} differs from crt_trace's"
                a, o = acc[m][:, :3], truth.frame(int(c))[0][m][:, :3]
                fin = np.isfinite(a).all(-1) & np.isfinite(o).all(-1)
                assert np.array_equal(bits(a[fin]), bits(o[fin])), f"finite pixels at count {c} differ from the oracle"
            nan_px = np.isnan(acc[..., 1])
            nan_tile = np.zeros((3 * 8, 4 * 8), bool)
            nan_tile[:24, :32] = nan_px
            nan_tile = nan_tile.reshape(3, 8, 4, 8).any(axis=(1, 3))
            assert np.array_equal(np.isinf(errors), nan_tile), "E is +inf exactly on the tiles with a NaN pixel"
            want_E = truth.errors(after)
            agree = np.isinf(want_E) == nan_tile
            assert np.array_equal(errors[agree].view(np.uint32), want_E[agree].view(np.uint32))
            if n == 0:
                break
        assert n == 0
        assert nan_tile.any() and (after[nan_tile] == 12).all() and (after[~nan_tile] == 4).all()
    finally:
        renderer.reset()


def test_non_finite_camera_image_is_black_and_retires_at_min(renderer):
    """The reference renders a non-finite camera as a black image (every path misses): every pixel's e is 0, so with a
    threshold of 0 (E <= 0 holds) the tiles retire once they hold min_samples, below max_samples."""
    from computeraytracer_amd import cornell
    from computeraytracer_amd.scene import PackedScene
    ps = cornell(32, 24)
    cam = ps.camera.copy()
    cam[0] = np.nan
    try:
        renderer.upload(PackedScene(ps.primitives, ps.lights, cam, ps.spectra, ps.cie)).build_accel("bvh2")
        assert renderer.trace_adaptive(samples=4, threshold=0.0, min_samples=8, max_samples=16) == 12
        assert renderer.trace_adaptive(samples=4, threshold=0.0, min_samples=8, max_samples=16) == 12
        counts, errors = renderer.read_adaptive()
        assert (counts == 8).all() and (errors == 0).all()
        assert renderer.trace_adaptive(samples=4, threshold=0.0, min_samples=8, max_samples=16) == 0
        assert not renderer.read_accum()[..., :3].any()
    finally:
        renderer.reset()


# ------------------------------------------------------------------ 7. state
def test_state_rules(orc):
    """Every CRT_ESTATE / CRT_EINVAL case, on a context of its own (a failure part way leaves nothing behind for the
    other test files)."""
    import ctypes as C
    from computeraytracer_amd import Renderer, cornell
    from computeraytracer_amd._lib import AdaptiveParams, CrtError, adaptive_defaults
    ps = cornell(100, 76)
    with Renderer(0) as renderer:
        lib, h = renderer._lib, renderer._h
        with pytest.raises(CrtError, match="upload a scene first"):
            renderer.trace_adaptive()
        renderer.upload(ps)
        with pytest.raises(CrtError, match="crt_build_accel first"):
            renderer.trace_adaptive()
        renderer.build_accel("bvh2")
        with pytest.raises(CrtError, match="uniform state"):
            renderer.read_adaptive()
        renderer.frame(1).sync()
        with pytest.raises(CrtError) as e:
            renderer.trace_adaptive()
        assert e.value.code == -3 and "crt_reset" in str(e.value)
        renderer.reset()
        # bad parameters: CRT_EINVAL, nothing changes (still uniform, sample 0)
        for p in [AdaptiveParams(0, 8, 16, 0.1), AdaptiveParams(8, 8, 16, -0.5), AdaptiveParams(8, 8, 16, float("nan")),
                  AdaptiveParams(8, 8, 16, float("inf")), AdaptiveParams(8, 32, 16, 0.1)]:
            assert lib.crt_trace_adaptive(h, C.byref(p), None) == -1
        assert renderer.sample == 0
        d = adaptive_defaults()
        assert lib.crt_trace_adaptive(h, None, None) == 0                  # NULL = the defaults
        counts, _ = renderer.read_adaptive()
        assert (counts == max(d.samples, 1)).all()                         # (every tile starts below min_samples or at it)
        acc, rgba = renderer.read_accum(), renderer.read_rgba8()
        assert lib.crt_trace_adaptive(h, C.byref(AdaptiveParams(8, 8, 4, 0.1)), None) == -1
        assert np.array_equal(renderer.read_adaptive()[0], counts) and np.array_equal(bits(acc), bits(renderer.read_accum()))
        # refused in the adaptive state
        u, buf = C.c_uint32(), np.zeros((76, 100, 4), np.uint8)
        for rc in (lib.crt_trace(h, 1), lib.crt_sample_count(h, C.byref(u)), lib.crt_read_latest_rgba8(h, buf.ctypes.data, None),
                   lib.crt_latest_sample(h, C.byref(u)), lib.crt_read_sample_rgba8(h, 1, buf.ctypes.data),
                   lib.crt_denoise(h, None, None, buf.ctypes.data)):
            assert rc == -3
            assert "crt_read_adaptive" in lib.crt_last_error(h).decode()
        assert np.array_equal(rgba, renderer.read_rgba8())                 # reads keep working
        # a switch between the loop and a tree keeps the counts, and the next round is still exact
        truth = _truth(orc, ps)
        for mode in ("none", "bvh2"):
            renderer.build_accel(mode)
            assert np.array_equal(renderer.read_adaptive()[0], counts)
            counts = counts + 4 * renderer.trace_adaptive(samples=4, threshold=1e30, min_samples=1000) // counts.size
            assert np.array_equal(renderer.read_adaptive()[0], counts)
            truth.check(renderer, counts)
        renderer.reset()
        # everything that zeroes or replaces the accumulator returns to the uniform state
        leave = {"reset": lambda: renderer.reset(),
                 "upload": lambda: renderer.upload(ps).build_accel("bvh2"),
                 "write_accum": lambda: renderer.write_accum(np.zeros((76, 100, 4), F), 0),
                 "set_camera": lambda: renderer.set_camera(ps.camera),
                 "update_lights": lambda: renderer.update_lights(0, ps.lights),
                 "update_primitives": lambda: renderer.update_primitives(0, ps.primitives[:1]),
                 "set_tile": lambda: renderer.set_tile(0, 0, 100, 76),
                 "set_row_bands": lambda: renderer.set_row_bands(8, 2, 1)}
        for name, fn in leave.items():
            assert renderer.trace_adaptive(samples=2, min_samples=4) > 0, name
            fn()
            with pytest.raises(CrtError, match="uniform state"):
                renderer.read_adaptive()
            assert renderer.sample == 0, name
            if name == "update_primitives":
                with pytest.raises(CrtError, match="refit"):              # a stale tree: crt_trace's message
                    renderer.trace_adaptive(samples=2)
                renderer.refit_accel()
            renderer.frame(1).sync()
            assert renderer.sample == 1, name
            renderer.reset()
        renderer.set_tile(0, 0, 100, 76)
        # not under a communicator partition
        renderer.comm_init(Renderer.comm_unique_id(local=True), 0, 1)
        try:
            renderer.comm_partition(0)
            with pytest.raises(CrtError, match="crt_comm_partition"):
                renderer.trace_adaptive(samples=2)
        finally:
            renderer.comm_destroy()


# ------------------------------------------------------------------ 8. it pays
def test_adaptive_beats_uniform_at_equal_pixel_samples(renderer):
    """Cornell 128 x 128.  Adaptive: 16 samples everywhere, then rounds of 8 for the tiles above the median error, until
    the pixel-samples reach those of a 64-spp image.  The uniform control gets ceil(pixel-samples / pixels) spp (at least
    as many).  Against a 1024-spp render, the 95th percentile of the per-tile RMSE of the mean XYZ is lower for adaptive.
    (Deterministic: the RNG is.  Measured on an MI355X: 0.0433 adaptive, 0.0523 uniform at 64 spp, a ratio of 0.83; the
    margin asserted is 0.9.)"""
    from computeraytracer_amd import cornell
    ps = cornell(128, 128)
    npix = 128 * 128
    try:
        renderer.upload(ps).build_accel("bvh2")
        renderer.frame(1024).sync()
        ref_mean = renderer.read_accum()[..., :3] / F(1024)
        renderer.reset()
        renderer.trace_adaptive(samples=16, threshold=1e30, min_samples=16)
        while True:
            counts, errors = renderer.read_adaptive()
            ps_done = int(counts.sum()) * 64
            if ps_done >= 64 * npix:
                break
            assert renderer.trace_adaptive(samples=8, threshold=float(np.median(errors)), min_samples=16) > 0
        a_mean = renderer.read_accum()[..., :3] / ref.pixel_counts(counts, 128, 128)[..., None].astype(F)
        n_u = -(-ps_done // npix)
        renderer.reset().frame(n_u).sync()
        u_mean = renderer.read_accum()[..., :3] / F(n_u)

        def p95(mean):
            d2 = ((mean - ref_mean) ** 2).reshape(16, 8, 16, 8, 3).mean(axis=(1, 3, 4))
            return float(np.percentile(np.sqrt(d2), 95))
        pa, pu = p95(a_mean), p95(u_mean)
        print(f"p95 tile RMSE: adaptive {pa:.5f}, uniform {pu:.5f} at {n_u} spp")
        assert pa < 0.9 * pu, (pa, pu)
    finally:
        renderer.reset()
