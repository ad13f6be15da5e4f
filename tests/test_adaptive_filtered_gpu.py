"""GPU tests of crt_trace_adaptive_filtered / crt_read_adaptive_filtered (include/crt.h "Adaptive sampling judged by the
filtered preview"; run with -m gpu on an MI355X).

E' of a tile is a function of what crt_denoise_adaptive returns as var_out and of the counts alone, so it is checked bit
for bit against tests/adaptive_filtered_ref.py applied to that call's own output; the selection is the rule of
tests/adaptive_ref.py with E' in E's place, and the samples it enqueues are the oracle's, as for crt_trace_adaptive."""
import numpy as np
import pytest

import adaptive_filtered_ref as fref
import adaptive_ref as aref
import denoise_ref as ref
from conftest import bits
from test_adaptive_gpu import _truth, options, run_rounds
from test_adaptive_temporal_gpu import B, assert_pixels_are_the_oracles, offset_truth, tidy  # noqa: F401 (offset_truth: a fixture)

pytestmark = pytest.mark.gpu
F = np.float32
EINVAL, ESTATE, ENOMEM = -1, -3, -4
FILTERS = {"defaults": {}, "narrow": dict(iterations=3, sigma_variance=2.0, sigma_normal=0.25, sigma_plane=0.1),
           "iterations0": dict(iterations=0)}
RULE = dict(min_samples=8, max_samples=40)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def refused(fn, code, match=None):
    from computeraytracer_amd._lib import CrtError
    with pytest.raises(CrtError, match=match) as e:
        fn()
    assert e.value.code == code, str(e.value)


def mixed_counts(r, samples=8, rounds=3):
    """An adaptive state whose tiles hold at least three different counts: one round everywhere, then rounds for the
    tiles above the median raw error."""
    n = r.trace_adaptive(samples=samples, threshold=0.0, **RULE)
    e = r.read_adaptive()[1]
    assert n == e.size
    thr = float(F(np.median(e[np.isfinite(e)])))
    for _ in range(rounds):
        r.trace_adaptive(samples=samples, threshold=thr, **RULE)
    counts = r.read_adaptive()[0]
    assert len(np.unique(counts)) >= 3, np.unique(counts)
    return counts


def assert_errors_are_the_filters(r, **filt):
    counts, errors = r.read_adaptive_filtered(**filt)
    v = r.denoise_adaptive(var=True, **filt)[1]
    want = fref.tile_errors_filtered(v, counts)
    assert np.array_equal(u32(errors), u32(want)), f"{int((u32(errors) != u32(want)).sum())} tile errors differ from sqrt(max var_out)"
    assert np.array_equal(counts, r.read_adaptive()[0])
    assert np.isfinite(errors).all() and (errors > 0).any()
    return counts, errors


def filtered_round(r, samples, threshold=None, **filt):
    """One crt_trace_adaptive_filtered call checked against the rule: threshold None = the median of the finite E'.
    Returns (counts before, counts after, active mask, threshold)."""
    counts, errors = r.read_adaptive_filtered(**filt)
    thr = F(np.median(errors[np.isfinite(errors)])) if threshold is None else F(threshold)
    want = aref.active(counts, errors, RULE["min_samples"], RULE["max_samples"], thr)
    n = r.trace_adaptive_filtered(samples=samples, threshold=float(thr), **RULE, **filt)
    assert n == int(want.sum()), (n, int(want.sum()))
    r.sync()
    after = r.read_adaptive()[0]
    assert np.array_equal(after, counts + np.uint32(samples) * want.astype(np.uint32)), "the tiles that grew are not the rule's"
    return counts, after, want, thr


# ------------------------------------------------------------------ 1. E' is the filter's own variance
@pytest.mark.parametrize("filt", list(FILTERS))
def test_errors_are_the_root_of_the_filters_tile_maximum(renderer, filt):
    from computeraytracer_amd import cornell
    r = renderer
    try:
        options(r)
        r.upload(cornell(100, 76)).build_accel("bvh2")          # ragged tiles on both edges: 13 x 10
        mixed_counts(r)
        assert_errors_are_the_filters(r, **FILTERS[filt])
        r.set_tile(13, 7, 85, 68)                               # 72 x 61 at an odd offset: filtered and judged on its own
        counts = mixed_counts(r)
        assert counts.shape == (8, 9)
        assert_errors_are_the_filters(r, **FILTERS[filt])
    finally:
        r.set_tile(0, 0, 100, 76)
        r.reset()


def test_one_sample_per_tile_is_judged_infinite(renderer):
    from computeraytracer_amd import cornell
    r = renderer
    try:
        r.upload(cornell(100, 76)).build_accel("bvh2")
        assert r.trace_adaptive_filtered(samples=1, threshold=0.5, min_samples=1, max_samples=8) == 130
        counts, errors = r.read_adaptive_filtered()
        assert (counts == 1).all() and np.isposinf(errors).all()
        # ... so every tile is active whatever the threshold; at 2 samples E' is a number
        assert r.trace_adaptive_filtered(samples=1, threshold=1e30, min_samples=1, max_samples=8) == 130
        counts, errors = r.read_adaptive_filtered()
        assert (counts == 2).all() and np.isfinite(errors).all()
        assert r.trace_adaptive_filtered(samples=1, threshold=1e30, min_samples=1, max_samples=8) == 0
    finally:
        r.reset()


# ------------------------------------------------------------------ 2. the selection
@pytest.mark.parametrize("form", ["wavefront-bvh2", "accel-none"])
def test_selection_follows_the_rule_and_samples_are_the_oracles(renderer, orc, form):
    from computeraytracer_amd import cornell
    r = renderer
    ps = cornell(100, 76)
    truth = _truth(orc, ps)
    try:
        options(r)
        r.upload(ps).build_accel({"wavefront-bvh2": "bvh2", "accel-none": "none"}[form])
        mixed_counts(r)
        counts, after, want, _ = filtered_round(r, 4)
        assert 0 < int(want.sum()) < want.size                  # (neither everything nor nothing)
        truth.check(r, after)                                   # accumulator and rgba8: the oracle at each tile's own count
        _, after2, _, _ = filtered_round(r, 4, **FILTERS["narrow"])
        truth.check(r, after2)
    finally:
        r.reset()
        options(r)


def test_selection_under_adaptive_temporal_with_a_sample_offset(renderer, offset_truth):
    ps, sc, frame = offset_truth
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("adaptive_temporal", 1)
        r.set_sample_offset(B)
        assert r.trace_adaptive_filtered(samples=2, threshold=0.0, min_samples=2, max_samples=6) == 72
        for _ in range(2):
            counts, errors = r.read_adaptive_filtered()
            thr = F(np.median(errors[np.isfinite(errors)]))
            want = aref.active(counts, errors, 2, 6, thr)
            assert r.trace_adaptive_filtered(samples=2, threshold=float(thr), min_samples=2, max_samples=6) == int(want.sum())
            after = r.read_adaptive()[0]
            assert np.array_equal(after, counts + 2 * want.astype(np.uint32))
            assert_pixels_are_the_oracles(r, sc, frame, after)  # samples B + 1 .. B + n_t
        assert len(np.unique(after)) >= 2
    finally:
        tidy(r)


# ------------------------------------------------------------------ 3. entering the state
def test_entering_call_runs_no_filter_and_the_next_selects_by_the_filter():
    """A context of its own whose filter buffers and G-buffer were never allocated: with the next device allocation set to
    fail, the call that enters the adaptive state succeeds (it allocates nothing: the adaptive buffers exist from the
    state before the reset, the filter does not run), every tile is active, and the call after it selects by E'."""
    from computeraytracer_amd import Renderer, cornell
    with Renderer(0) as r:
        try:
            r.upload(cornell(100, 76)).build_accel("bvh2")
            assert r.trace_adaptive(samples=8, threshold=0.0, **RULE) == 130
            r.sync().reset()
            r.set_option("debug_fail_alloc", 1)
            assert r.trace_adaptive_filtered(samples=8, threshold=0.0, **RULE) == 130
            r.set_option("debug_fail_alloc", 0)
            assert (r.read_adaptive()[0] == 8).all()
            _, _, want, _ = filtered_round(r, 8)
            assert 0 < int(want.sum()) < want.size
        finally:
            r.set_option("debug_fail_alloc", 0)


# ------------------------------------------------------------------ 4. reads only
def test_read_adaptive_filtered_changes_nothing(renderer, orc):
    from computeraytracer_amd import cornell
    r = renderer
    ps = cornell(100, 76)
    truth = _truth(orc, ps)

    def everything():
        return (bits(r.read_accum()), r.read_rgba8()) + tuple(u32(a) for a in r.read_adaptive()) + (r.counters(),)
    try:
        options(r)
        r.upload(ps).build_accel("bvh2")
        r.enable_counters(True).reset_counters()
        mixed_counts(r)
        before = everything()
        r.read_adaptive_filtered()
        r.read_adaptive_filtered(**FILTERS["narrow"])
        after = everything()
        for a, b in zip(before[:-1], after[:-1]):
            assert np.array_equal(a, b)
        assert before[-1] == after[-1]
        _, counts, _, _ = filtered_round(r, 4)                  # ... and the following round is exact
        truth.check(r, counts)
    finally:
        r.enable_counters(False)
        r.reset()
        options(r)


def test_read_adaptive_filtered_leaves_the_temporal_history(renderer, offset_truth):
    ps, sc, frame = offset_truth
    r = renderer
    try:
        r.upload(ps).build_accel("bvh2").set_option("adaptive_temporal", 1)
        assert r.trace_adaptive_filtered(samples=4, threshold=0.0, min_samples=4, max_samples=4) == 72
        r.denoise_temporal()                                    # frame 0: the history of frame 1
        r.reset().set_sample_offset(B)
        assert r.trace_adaptive_filtered(samples=2, threshold=0.0, min_samples=2, max_samples=6) == 72
        h1 = r.denoise_temporal(history=True)[1]
        assert (h1 > 2).mean() > 0.5                            # (frame 0 is in it)
        counts, errors = r.read_adaptive_filtered()
        h2 = r.denoise_temporal(history=True)[1]
        assert np.array_equal(bits(h1), bits(h2))
        thr = F(np.median(errors[np.isfinite(errors)]))
        n = r.trace_adaptive_filtered(samples=2, threshold=float(thr), min_samples=2, max_samples=6)
        assert n == int(aref.active(counts, errors, 2, 6, thr).sum()) and 0 < n < 72
        h3 = r.denoise_temporal(history=True)[1]
        assert np.isfinite(h3).all()
        assert_pixels_are_the_oracles(r, sc, frame, r.read_adaptive()[0])
    finally:
        tidy(r)


# ------------------------------------------------------------------ 5. refusals, the context unchanged
def test_refusals_leave_the_context_as_it_was(orc):
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(100, 76)
    bad_filters = [dict(iterations=11), dict(sigma_variance=0.0), dict(sigma_normal=float("nan")), dict(sigma_plane=float("inf")),
                   dict(sigma_variance=-1.0)]
    with Renderer(0) as r:
        refused(lambda: r.trace_adaptive_filtered(), ESTATE, "upload a scene first")       # no scene
        refused(lambda: r.read_adaptive_filtered(), ESTATE)
        r.upload(ps).build_accel("bvh2")
        refused(lambda: r.read_adaptive_filtered(), ESTATE, "uniform state")
        for f in bad_filters:                                   # in the uniform state: it stays uniform, at sample 0
            refused(lambda: r.trace_adaptive_filtered(samples=4, **f), EINVAL)
            refused(lambda: r.read_adaptive_filtered(**f), EINVAL)
        refused(lambda: r.trace_adaptive_filtered(samples=0), EINVAL, "samples")
        assert r.sample == 0
        r.frame(1).sync()
        refused(lambda: r.trace_adaptive_filtered(), ESTATE, "crt_reset")                   # a uniform render holding samples
        r.reset()
        counts = mixed_counts(r)
        state = (bits(r.read_accum()), r.read_rgba8(), counts)

        def unchanged():
            now = (bits(r.read_accum()), r.read_rgba8(), r.read_adaptive()[0])
            return all(np.array_equal(a, b) for a, b in zip(state, now))
        for f in bad_filters:                                   # in the adaptive state: counts and accumulator stay
            refused(lambda: r.trace_adaptive_filtered(samples=4, threshold=0.0, **RULE, **f), EINVAL)
            refused(lambda: r.read_adaptive_filtered(**f), EINVAL)
        refused(lambda: r.trace_adaptive_filtered(samples=0, threshold=0.0, **RULE), EINVAL, "samples")
        assert unchanged()
        truth = _truth(orc, ps)
        _, after, _, _ = filtered_round(r, 4)                   # ... and the state still works
        truth.check(r, after)
        # a stale tree
        r.update_primitives(0, ps.primitives[:1])
        refused(lambda: r.trace_adaptive_filtered(samples=2), ESTATE, "refit")
        r.refit_accel()
        # row bands: crt_trace_adaptive works there, the filter does not
        r.set_row_bands(8, 2, 1)
        refused(lambda: r.trace_adaptive_filtered(samples=2, threshold=0.0, **RULE), ESTATE, "row-band")
        assert r.sample == 0                                    # (still uniform)
        assert r.trace_adaptive(samples=2, threshold=0.0, **RULE) > 0
        banded = r.read_adaptive()[0]
        refused(lambda: r.trace_adaptive_filtered(samples=2, threshold=0.0, **RULE), ESTATE, "row-band")
        refused(lambda: r.read_adaptive_filtered(), ESTATE, "row-band")
        assert np.array_equal(r.read_adaptive()[0], banded)
        r.set_tile(0, 0, 100, 76)


@pytest.mark.parametrize("k", [1, 6])
def test_out_of_memory_in_the_filter_enqueues_nothing(k):
    """The k-th device allocation of the first filtered selection fails (1: a colour buffer, 6: the G-buffer): CRT_ENOMEM,
    counts and accumulator as they were; the repeated call gives what a context without the failure gives."""
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(100, 76)
    got = []
    for fail in (0, k):
        with Renderer(0) as r:
            try:
                r.upload(ps).build_accel("bvh2")
                assert r.trace_adaptive_filtered(samples=8, threshold=0.0, **RULE) == 130
                r.sync()
                before = (bits(r.read_accum()), r.read_adaptive()[0])
                if fail:
                    r.set_option("debug_fail_alloc", fail)
                    refused(lambda: r.trace_adaptive_filtered(samples=8, threshold=0.02, **RULE), ENOMEM)
                    r.set_option("debug_fail_alloc", 0)
                    r.sync()
                    assert np.array_equal(before[0], bits(r.read_accum())) and np.array_equal(before[1], r.read_adaptive()[0])
                n = r.trace_adaptive_filtered(samples=8, threshold=0.02, **RULE)
                r.sync()
                got.append((n, r.read_adaptive()[0], bits(r.read_accum())))
            finally:
                r.set_option("debug_fail_alloc", 0)
    assert 0 < got[0][0] < 130
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])


# ------------------------------------------------------------------ 6. quality on the product
def test_filtered_rule_pays_on_the_product(renderer):
    """The protocol of tests/test_adaptive_filtered_cpu.py with the GPU's renders and filter (the renders are the oracle's
    bit for bit and the filter is within 1e-4 of its restatement: test_adaptive_gpu, test_denoise_adaptive_gpu), under
    the same assertion: not more samples, and MSE(new) / MSE(old) <= adaptive_filtered_ref.RATIO_MEASURED + 0.05."""
    from computeraytracer_amd import cornell
    r = renderer
    W = H = 96
    try:
        options(r)
        r.upload(cornell(W, H)).build_accel("bvh2")
        r.set_sample_offset(fref.TRUTH_FIRST - 1).frame(fref.TRUTH_SPP).sync()
        conv = ref.linear_rgb(r.read_accum(), fref.TRUTH_SPP)
        r.reset().set_sample_offset(0)
        out = {}
        for name, trace, tau in (("old", r.trace_adaptive, fref.TAU_RAW), ("new", r.trace_adaptive_filtered, fref.TAU_FILTERED)):
            rounds = 0
            while trace(samples=fref.STEP, threshold=tau, min_samples=fref.FIRST, max_samples=fref.CAP):
                rounds += 1
                assert rounds <= 64                             # (E' of a tile at rest moves with its neighbours: it may wake)
            counts = r.read_adaptive()[0]
            rgb = r.denoise_adaptive(rgb=True)[1][..., :3]
            out[name] = (float(counts.mean()), ref.mse_display(rgb, conv))
            r.reset()
        ratio = out["new"][1] / out["old"][1]
        print(f"old rule: {out['old'][0]:.2f} mean samples, MSE {out['old'][1]:.6f}; new rule: {out['new'][0]:.2f} mean samples, "
              f"MSE {out['new'][1]:.6f}; ratio {ratio:.4f}")
        assert out["new"][0] <= out["old"][0], out
        assert ratio <= fref.RATIO_MEASURED + fref.RATIO_MARGIN, ratio
    finally:
        r.reset().set_sample_offset(0)
        options(r)
