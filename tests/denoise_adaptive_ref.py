"""The numpy restatement of crt_denoise_adaptive (include/crt.h "Denoised preview of an adaptive render", DESIGN.md
6d), in float64: the yardstick the GPU filter is checked against.  A helper module, not collected by pytest."""
import numpy as np

import adaptive_ref as aref
import denoise_ref as ref

MISS = ref.MISS
H = ref.H
G3 = np.array([0.25, 0.5, 0.25])
EPS = (0.5 / 255.0) ** 2
DEFAULTS = dict(iterations=5, sigma_variance=8.0, sigma_normal=0.5, sigma_plane=0.3)


def linear_rgb(accum, npx):
    """c = M (accum / n) per pixel with the pixel's own count npx (H, W), float64."""
    return (np.asarray(accum, np.float64)[..., :3] / np.asarray(npx, np.float64)[..., None]) @ ref.M.T


def linear_rgb_f32(accum, npx):
    """The same in the device's float32 operations and order (denoise_ref.linear_rgb_f32 per count)."""
    npx = np.asarray(npx)
    out = np.zeros(npx.shape + (3,), np.float32)
    for n in np.unique(npx):
        m = npx == n
        out[m] = ref.linear_rgb_f32(np.asarray(accum)[m], n)
    return out


def variance(S, Q, npx, exp_):
    """v per pixel, float32 as the device computes it: e * e with e = adaptive_ref.pixel_error at the pixel's count;
    1 ("nothing known") where the count is below 2 or e * e is not finite (e NaN or infinite, or the square overflows)."""
    npx = np.asarray(npx, np.uint32)
    e = aref.pixel_error(S, Q, np.maximum(npx, 2), exp_)
    with np.errstate(all="ignore"):
        ee = (e * e).astype(np.float32)
    return np.where((npx >= 2) & np.isfinite(ee), ee, np.float32(1.0)).astype(np.float32)


def _shift(hh, ww, oy, ox):
    """Slices (P, Q) of the pixels p and their taps q = p + (oy, ox) that lie inside the image."""
    P = (slice(max(0, -oy), hh - max(0, oy)), slice(max(0, -ox), ww - max(0, ox)))
    Q = (slice(max(0, oy), hh - max(0, -oy)), slice(max(0, ox), ww - max(0, -ox)))
    return P, Q


def blur_variance(v, key):
    """(1,2,1) x (1,2,1) / 16 of v at unit step over the taps inside the image with the centre's key, renormalised."""
    hh, ww = v.shape
    vs, vw = np.zeros((hh, ww)), np.zeros((hh, ww))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if abs(dy) >= hh or abs(dx) >= ww:
                continue
            P, Q = _shift(hh, ww, dy, dx)
            w = G3[dx + 1] * G3[dy + 1] * (key[P] == key[Q])
            vs[P] += w * v[Q]
            vw[P] += w
    return vs / vw


def atrous_var(c, v, pos, nrm, key, iterations=5, sigma_variance=8.0, sigma_normal=0.5, sigma_plane=0.3):
    """K iterations of the variance-guided a-trous filter on linear rgb c (H, W, 3) and variance v (H, W), guided by
    position, normal (H, W, 3) and key (H, W).  Taps, skipping rules, kernel, normal and plane terms and the key test
    are denoise_ref.atrous's; the colour term is |T(c_p) - T(c_q)|^2 / (sigma_variance^2 (v~_p + v~_q) + EPS) and the
    variance is carried along: v' = sum w^2 v_q / (sum w)^2 (a pixel whose colour is not finite keeps its v, so v stays
    finite).  Returns (c, v)."""
    c = np.asarray(c, np.float64)[..., :3].copy()
    v = np.asarray(v, np.float64).copy()
    pos = np.asarray(pos, np.float64)
    nrm = np.asarray(nrm, np.float64)
    key = np.asarray(key)
    hit = key != MISS
    hh, ww = c.shape[:2]
    for i in range(iterations):
        s = 1 << i
        t = ref.display(c)
        fin = np.isfinite(c).all(-1)
        vt = blur_variance(v, key)
        sw, sv, sc = np.zeros((hh, ww)), np.zeros((hh, ww)), np.zeros((hh, ww, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                if abs(oy) >= hh or abs(ox) >= ww:
                    continue
                P, Q = _shift(hh, ww, oy, ox)
                w0 = H[dx + 2] * H[dy + 2]
                if dx == 0 and dy == 0:
                    sw[P] += w0
                    sc[P] += w0 * c[P]
                    sv[P] += w0 * w0 * v[P]
                    continue
                ok = fin[Q] & (key[P] == key[Q])
                with np.errstate(invalid="ignore"):
                    d2 = ((t[P] - t[Q]) ** 2).sum(-1)
                    w = w0 * np.exp(-d2 / (sigma_variance ** 2 * (vt[P] + vt[Q]) + EPS))
                    d = pos[Q] - pos[P]
                    dl = np.sqrt((d * d).sum(-1))
                    sine = np.abs((nrm[P] * d).sum(-1)) / np.where(dl > 0, dl, 1.0)
                    w_n = np.exp(-((nrm[P] - nrm[Q]) ** 2).sum(-1) / sigma_normal ** 2)
                    w_x = np.where(dl > 0, np.exp(-sine / sigma_plane), 1.0)
                    w = w * np.where(hit[P], w_n * w_x, 1.0)
                w = np.where(ok, w, 0.0)
                sw[P] += w
                sc[P] += w[..., None] * np.where(ok[..., None], c[Q], 0.0)
                sv[P] += w * w * v[Q]
        c = sc / sw[..., None]
        with np.errstate(invalid="ignore"):
            v = np.where(fin, sv / sw ** 2, v)          # (a non-finite centre has NaN weights: it keeps its v)
    return c, v


def atrous_var_gbuffer(c, v, gbuf, primitives, **params):
    """atrous_var() guided by a G-buffer as crt_read_gbuffer returns it."""
    p = dict(DEFAULTS, **params)
    return atrous_var(c, v, gbuf[..., 1:4], gbuf[..., 4:7], ref.keys(gbuf, primitives), **p)
