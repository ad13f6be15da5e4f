"""CPU tests of crt_trace_adaptive_filtered / crt_read_adaptive_filtered (include/crt.h "Adaptive sampling judged by the
filtered preview"): the interface at every layer, the float32 restatement of the tile error E'
(tests/adaptive_filtered_ref.py) on synthetic planes, and what the rule buys on oracle renders."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_filtered_ref as fref
import adaptive_ref as aref
import denoise_adaptive_ref as vref
import denoise_ref as ref
from conftest import ROOT

NODE = shutil.which("node")
F = np.float32
NEW = ("crt_trace_adaptive_filtered", "crt_read_adaptive_filtered")


# ------------------------------------------------------------------ 1. the interface
def test_header_and_library_have_the_calls():
    from test_abi import declared_symbols
    from computeraytracer_amd import _lib
    syms = declared_symbols()
    assert os.path.exists(_lib.LIB_PATH), "build libcrt.so first (__graft_entry__.build())"
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in syms, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 4, name
        assert hasattr(lib, name), name
    lib = _lib.load()
    assert lib.crt_trace_adaptive_filtered(None, None, None, None) == -1        # no context: CRT_EINVAL
    assert lib.crt_read_adaptive_filtered(None, None, None, None) == -1
    assert lib.crt_abi_version() == 2                                          # additive: the ABI version stays


def test_renderer_has_the_methods():
    import inspect
    from computeraytracer_amd import Renderer
    filt = ["iterations", "sigma_variance", "sigma_normal", "sigma_plane"]
    sig = inspect.signature(Renderer.trace_adaptive_filtered)
    assert list(sig.parameters)[1:] == ["samples", "threshold", "min_samples", "max_samples"] + filt
    assert all(p.default is None for p in list(sig.parameters.values())[1:])   # (the library's defaults)
    assert list(inspect.signature(Renderer.read_adaptive_filtered).parameters)[1:] == filt


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_the_calls():
    addon = os.path.join(ROOT, "addon", "crt_napi.node")
    assert os.path.exists(addon), "build the addon first (__graft_entry__.build())"
    js = ("const a=require(%r);for(const n of ['traceAdaptiveFiltered','readAdaptiveFiltered']) if(typeof a[n]!=='function') "
          "throw new Error(n);console.log('ok')" % addon)
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_command_line_flag_needs_adaptive():
    from computeraytracer_amd.__main__ import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(["--adaptive-filtered"])
    assert e.value.code == 2
    args = parse_args(["--adaptive", "0.02", "--adaptive-filtered", "--denoise", "3"])
    assert args.adaptive_filtered and args.adaptive == 0.02 and args.denoise == 3
    assert not parse_args(["--adaptive", "0.02"]).adaptive_filtered


# ------------------------------------------------------------------ 2. the restatement on synthetic planes
def test_tile_error_is_the_root_of_the_tile_maximum():
    th, tw = 19, 21                                          # ragged tiles on both edges: 3 x 3
    rng = np.random.default_rng(7)
    v = rng.gamma(0.5, 1e-3, (th, tw)).astype(F)
    counts = np.full((3, 3), 6, np.uint32)
    E = fref.tile_errors_filtered(v, counts)
    assert E.dtype == F and E.shape == (3, 3)
    for ty in range(3):
        for tx in range(3):
            blk = v[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]    # (the edge tiles: 3 rows, 5 columns)
            assert E[ty, tx].view(np.uint32) == np.sqrt(blk.max()).view(np.uint32), (ty, tx)
    # what lies outside the frame does not enter: the largest value of the plane moved to the last in-frame pixel
    v2 = v.copy()
    v2[18, 20] = F(4.0)
    E2 = fref.tile_errors_filtered(v2, counts)
    assert E2[2, 2] == F(2.0) and np.array_equal(E2.ravel()[:8], E.ravel()[:8])
    # order independence
    perm = rng.permutation(64)
    v8 = v[:8, :8].reshape(64)[perm].reshape(8, 8)
    assert fref.tile_errors_filtered(v8, np.array([[6]], np.uint32))[0, 0] == E[0, 0]
    assert fref.tile_errors_filtered(np.zeros((8, 8), F), np.array([[2]], np.uint32))[0, 0] == 0.0


def test_nan_and_small_counts_give_infinity():
    v = np.full((19, 21), 1e-4, F)
    v[17, 20] = F(np.nan)                                    # a NaN in the bottom-right (ragged) tile
    v[3, 9] = F(np.inf)
    counts = np.array([[6, 6, 1], [6, 0, 6], [2, 6, 6]], np.uint32)
    E = fref.tile_errors_filtered(v, counts)
    assert E[0, 2] == np.inf and E[1, 1] == np.inf           # n < 2, whatever the plane holds
    assert E[2, 2] == np.inf                                 # NaN -> +inf
    assert E[0, 1] == np.inf                                 # an infinite variance
    assert E[2, 0] == np.sqrt(F(1e-4))                       # n == 2 is judged
    assert not np.isnan(E).any()


def test_square_root_comes_after_the_maximum():
    """max then sqrt and sqrt then max agree as real numbers; in float32 only the first is one rounding of the maximum.
    The restatement equals sqrt(max) bit for bit for every tile of a random plane, and E'^2 brackets the maximum."""
    rng = np.random.default_rng(11)
    v = (rng.random((64, 64)) * 1e-3).astype(F)
    counts = np.full((8, 8), 16, np.uint32)
    E = fref.tile_errors_filtered(v, counts)
    m = v.reshape(8, 8, 8, 8).max(axis=(1, 3))
    assert np.array_equal(E.view(np.uint32), np.sqrt(m).astype(F).view(np.uint32))
    lo, hi = np.nextafter(E, F(0)).astype(np.float64) ** 2, np.nextafter(E, F(np.inf)).astype(np.float64) ** 2
    assert ((lo < m) & (m < hi)).all()
    # the rule with E' in E's place
    act = aref.active(counts, E, 8, 64, F(np.median(E)))
    assert 0 < act.sum() < act.size and np.array_equal(act, ~(E <= F(np.median(E))))


# ------------------------------------------------------------------ 3. it pays (oracle renders)
@pytest.fixture(scope="module")
def cornell_samples(orc):
    """The protocol's inputs on the Cornell box 96 x 96: per-sample sums S, Q and accumulators A after 0..128 samples,
    the truth, the G-buffer."""
    from computeraytracer_amd import cornell
    W = H = 96
    ps = cornell(W, H)
    sc = orc.Scene.from_packed(ps)
    conv = ref.linear_rgb(sc.render(fref.TRUTH_SPP, first_sample=fref.TRUTH_FIRST)[0], fref.TRUTH_SPP)
    g, _ = ref.oracle_gbuffer(orc, ps, (0, 0, W, H))
    S, Q, A = [np.zeros((H, W), F)], [np.zeros((H, W), F)], [np.zeros((H, W, 4), F)]
    for s in range(1, fref.CAP + 1):
        a = sc.render(1, first_sample=s)[0]
        s_, q_ = aref.accumulate(a[None, ..., 1], S[-1], Q[-1])
        S.append(s_)
        Q.append(q_)
        A.append((A[-1] + a).astype(F))
    return dict(ps=ps, conv=conv, g=g, S=np.stack(S), Q=np.stack(Q), A=np.stack(A),
                exp_=lambda x: orc.math_eval("exp", np.asarray(x, F)))


def test_filtered_rule_reaches_the_quality_with_fewer_samples(cornell_samples):
    """The protocol of DESIGN.md 6k (adaptive_filtered_ref: 16 samples everywhere, rounds of 16, 128 at most, truth 4096
    samples from index 100 001 on) with the float64 restatement of crt_denoise_adaptive at its defaults: today's rule at
    threshold 0.15 against E' at 0.02.  The new run may not take more samples, and its filtered image's MSE in display
    space, relative to the old run's, stays within 0.05 of the ratio measured with this restatement (the oracle is
    deterministic: the margin covers libm differences).

    Measured: old rule 30.67 mean samples, MSE 0.001021; new rule 30.11 mean samples, MSE 0.000763; ratio 0.748
    (adaptive_filtered_ref.RATIO_MEASURED)."""
    d = cornell_samples
    H, W = d["S"].shape[1:]
    ii, jj = np.indices((H, W))

    def state(counts):
        npx = aref.pixel_counts(counts, H, W)
        return npx, vref.linear_rgb(d["A"][npx, ii, jj], npx), vref.variance(d["S"][npx, ii, jj], d["Q"][npx, ii, jj], npx, d["exp_"])

    def filtered(counts):
        _, noisy, v = state(counts)
        return vref.atrous_var_gbuffer(noisy, v, d["g"], d["ps"].primitives)

    def raw_error(counts):
        npx = aref.pixel_counts(counts, H, W)
        return aref.tile_errors(d["S"][npx, ii, jj], d["Q"][npx, ii, jj], counts, d["exp_"])

    shape = ((H + 7) // 8, (W + 7) // 8)
    old = fref.rounds(raw_error, shape, fref.TAU_RAW)
    new = fref.rounds(lambda c: fref.tile_errors_filtered(filtered(c)[1].astype(F), c), shape, fref.TAU_FILTERED)
    mse_old = ref.mse_display(filtered(old)[0], d["conv"])
    mse_new = ref.mse_display(filtered(new)[0], d["conv"])
    ratio = mse_new / mse_old
    print(f"old rule: {old.mean():.2f} mean samples, MSE {mse_old:.6f}; new rule: {new.mean():.2f} mean samples, "
          f"MSE {mse_new:.6f}; ratio {ratio:.4f}")
    assert len(np.unique(new)) >= 3                          # (tiles retire at different rounds)
    assert new.mean() <= old.mean(), (new.mean(), old.mean())
    assert ratio <= fref.RATIO_MEASURED + fref.RATIO_MARGIN, ratio
