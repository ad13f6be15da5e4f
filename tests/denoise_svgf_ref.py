"""The numpy restatement of crt_denoise_svgf (include/crt.h "Variance-guided temporal filter"), in float64:
the colour blend of 6e / 6f, the temporal moments of the luminance carried over the same taps, the variance they give,
and 6d's variance-guided passes on (c, v).  A helper module, not collected by pytest.

The moments ride on the blend's own taps and weights, and the restatement takes that literally: it runs the blend of
denoise_temporal_ref (or denoise_motion_ref) a second time with the slot's moments in place of its colour, so there is
one statement of which taps are accepted."""
import numpy as np

import denoise_adaptive_ref as aref
import denoise_motion_ref as mref
import denoise_ref as ref
import denoise_temporal_ref as tref

MISS = ref.MISS
EPS = aref.EPS
DEFAULTS = dict(iterations=5, sigma_variance=4.0, sigma_normal=0.5, sigma_plane=0.3, max_history=64.0, normal_tol=0.5,
                plane_tol=2.0, min_frames=4.0)
BLEND = tref.BLEND
FILTER = ("iterations", "sigma_variance", "sigma_normal", "sigma_plane")


def _blend(c_new, n, gbuf, key, frame, prev, prims_cur, W, H, x0, y0, **bp):
    """6e's blend, or 6f's where the frame's records prims_cur are given and the slot remembers its own."""
    if prims_cur is not None and prev is not None and prev.get("prims") is not None:
        return mref.blend(c_new, n, gbuf, key, frame, prev, prims_cur, prev["prims"], W, H, x0, y0, **bp)[:3]
    return tref.blend(c_new, n, gbuf[..., 1:4], gbuf[..., 4:7], key, frame, prev, W, H, x0, y0, **bp)


def blend(accum, n, gbuf, key, frame, prev, W, H, x0=0, y0=0, prims_cur=None, max_history=64.0, normal_tol=0.5, plane_tol=2.0):
    """The temporal half of one frame.  accum (h, w, >=3) XYZ sums of n samples; prev = None or a slot() of the previous
    frame.  Returns (c, Hw, mom, doubt): c, Hw, doubt are the colour blend's, mom (h, w, 3) = (m1, s, Mw)."""
    bp = dict(max_history=max_history, normal_tol=normal_tol, plane_tol=plane_tol)
    accum = np.asarray(accum, np.float64)
    c_new = ref.linear_rgb(accum, n)
    c, hw, doubt = _blend(c_new, n, gbuf, key, frame, prev, prims_cur, W, H, x0, y0, **bp)
    y = accum[..., 1] / n
    mom = np.stack([y, np.zeros_like(y), np.full_like(y, float(n))], -1)
    if prev is None or prev.get("mom") is None:
        return c, hw, mom, doubt
    # The same taps, the same weights: the slot's (m1', s') travel as its colour and Mw' as its weight.  A tap the colour
    # blend refuses for what it holds (Hw <= 0, a colour that is not finite) is refused here for the same reason, and a
    # frame whose colour is not finite takes no history here either (0 * c_new is NaN exactly where c_new is not finite).
    p_ok = (np.asarray(prev["hw"]) > 0) & np.isfinite(np.asarray(prev["c"], np.float64)[..., :3]).all(-1)
    pm = np.asarray(prev["mom"], np.float64)
    carried = np.where(p_ok[..., None], np.stack([pm[..., 0], pm[..., 1], np.zeros(p_ok.shape)], -1), np.nan)
    with np.errstate(all="ignore"):
        hm, mw, _ = _blend(c_new * 0.0, n, gbuf, key, frame, dict(prev, c=carried, hw=np.where(p_ok, pm[..., 2], 0.0)),
                           prims_cur, W, H, x0, y0, **bp)
    got = mw > n                                                # (Mw' >= its own n > 0, so an accepted tap always adds weight)
    mp = np.where(got, mw - n, 1.0)
    h1, hs = hm[..., 0] * mw / mp, hm[..., 1] * mw / mp          # undo (n * 0 + Mp * h) / Mw
    m1 = (n * y + mp * h1) / mw
    s = (mp / mw) * hs + (n * mp) * (y - h1) ** 2 / (mw * mw)
    mom = np.where(got[..., None], np.stack([m1, s, mw], -1), mom)
    return c, hw, mom, doubt


def variance(mom, n, min_frames=4.0):
    """v of the blended pixel in display units from its moments (h, w, >=3): g^2 s / (F - 1) with F = Mw / n and
    g = 2.2 exp(-2.2 max(m1, 0)) where F >= min_frames and the value is finite, 1 elsewhere.  F decides, so it is formed
    as the device forms it: one float32 division of the float32 Mw."""
    mom = np.asarray(mom)
    F = (mom[..., 2].astype(np.float32) / np.float32(n)).astype(np.float64)
    m1, s = mom[..., 0].astype(np.float64), mom[..., 1].astype(np.float64)
    with np.errstate(all="ignore"):
        g = 2.2 * np.exp(-2.2 * np.maximum(m1, 0.0))
        v = g * g * (s / (F - 1.0))
    known = (F >= min_frames) & np.isfinite(v) & (np.abs(v) <= np.finfo(np.float32).max)
    return np.where(known, v, 1.0), known


def slot(c, hw, mom, gbuf, key, frame, prims=None):
    """A history slot: denoise_temporal_ref.slot plus the moments (None: a slot crt_denoise_temporal wrote) and,
    for 6f, the records its frame was made against."""
    return dict(tref.slot(c, hw, gbuf, key, frame), mom=None if mom is None else np.asarray(mom, np.float64)[..., :3], prims=prims)


def svgf(accum, n, gbuf, key, frame, prev, W, H, x0=0, y0=0, prims_cur=None, **params):
    """crt_denoise_svgf of one frame: (filtered c (h, w, 3), variance left, blended c, Hw, mom, doubt)."""
    p = dict(DEFAULTS, **params)
    c, hw, mom, doubt = blend(accum, n, gbuf, key, frame, prev, W, H, x0, y0, prims_cur, **{k: p[k] for k in BLEND})
    v, _ = variance(mom, n, p["min_frames"])
    out, v_out = aref.atrous_var(c, v, gbuf[..., 1:4], gbuf[..., 4:7], key, **{k: p[k] for k in FILTER})
    return out, v_out, c, hw, mom, doubt
