"""The numpy restatement of the temporal filters in the adaptive state (option "adaptive_temporal", include/crt.h "Temporal
reuse across camera moves"), in float64.  A helper module, not collected by pytest.

6i is 6e / 6f / 6g with one substitution: wherever n stands for pixel p it is n_p, the count of p's 8x8 tile.  The
restatement takes that literally: it runs denoise_svgf_ref.blend / variance -- which run denoise_temporal_ref's or
denoise_motion_ref's blend -- once per distinct count with that count as n, and keeps each result on the pixels that hold
that count.  So there is still one statement of which taps are accepted, and a frame whose tiles all hold the same count
is the uniform restatement itself."""
import numpy as np

import adaptive_ref
import denoise_adaptive_ref as aref
import denoise_svgf_ref as sref

DEFAULTS = sref.DEFAULTS
BLEND = sref.BLEND
FILTER = sref.FILTER
slot = sref.slot


def pixel_counts(counts, h, w):
    """The count of each pixel's 8x8 tile, (h, w), from the tile grid crt_read_adaptive returns."""
    return adaptive_ref.pixel_counts(np.asarray(counts), h, w)


def _per_count(npx, call):
    """call(n) -> a tuple of (h, w, ...) arrays for every distinct n of npx, each kept where npx == n."""
    npx = np.asarray(npx)
    assert npx.min() >= 1, "a tile without a sample has no mean to blend"
    out = None
    for n in np.unique(npx):
        got = call(float(n))
        if out is None:
            out = [np.array(a, copy=True) for a in got]
        m = npx == n
        for o, a in zip(out, got):
            o[m] = a[m]
    return tuple(out)


def blend(accum, npx, gbuf, key, frame, prev, W, H, x0=0, y0=0, prims_cur=None, **bp):
    """denoise_svgf_ref.blend with a count per pixel, npx (h, w): (c, Hw, mom, doubt).  c and Hw are also what
    crt_denoise_temporal leaves (its blend is the same one, without the moments)."""
    return _per_count(npx, lambda n: sref.blend(accum, n, gbuf, key, frame, prev, W, H, x0, y0, prims_cur, **bp))


def variance(mom, npx, min_frames=4.0):
    """denoise_svgf_ref.variance with F = Mw / n_p: (v, known)."""
    return _per_count(npx, lambda n: sref.variance(mom, n, min_frames))


def svgf(accum, npx, gbuf, key, frame, prev, W, H, x0=0, y0=0, prims_cur=None, **params):
    """crt_denoise_svgf of one adaptive frame: (filtered c (h, w, 3), variance left, blended c, Hw, mom, doubt)."""
    p = dict(DEFAULTS, **params)
    c, hw, mom, doubt = blend(accum, npx, gbuf, key, frame, prev, W, H, x0, y0, prims_cur, **{k: p[k] for k in BLEND})
    v, _ = variance(mom, npx, p["min_frames"])
    out, v_out = aref.atrous_var(c, v, gbuf[..., 1:4], gbuf[..., 4:7], key, **{k: p[k] for k in FILTER})
    return out, v_out, c, hw, mom, doubt
