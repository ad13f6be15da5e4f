"""The numpy restatement of crt_denoise_temporal (include/crt.h "Temporal reuse across camera moves"), in
float64 and line by line: the yardstick the GPU blend is checked against.  The a-trous passes that follow the blend are
denoise_ref.atrous.  A helper module, not collected by pytest."""
import numpy as np

import denoise_ref as ref

MISS = ref.MISS
GLASS = 2
DEFAULTS = dict(iterations=5, sigma_color=1.0, sigma_normal=0.5, sigma_plane=0.3, max_history=64.0, normal_tol=0.5,
                plane_tol=2.0)
BLEND = ("max_history", "normal_tol", "plane_tol")


def frame_parts(frame):
    """llc, hor, ver, eye of the 12 floats of camera_frame, float64."""
    f = np.asarray(frame, np.float64).reshape(12)
    return f[0:3], f[3:6], f[6:9], f[9:12]


def inverse_frame(frame):
    """M' = [hor' ver' (llc' - eye')]^-1."""
    llc, hor, ver, eye = frame_parts(frame)
    return np.linalg.inv(np.stack([hor, ver, llc - eye], axis=1))


def kappa(frame, W):
    """The pixel's footprint per unit distance: (|hor| / W) / |llc + hor/2 + ver/2 - eye|."""
    llc, hor, ver, eye = frame_parts(frame)
    return (np.linalg.norm(hor) / W) / np.linalg.norm(llc + hor / 2 + ver / 2 - eye)


def reproject(frame, pos, W, H, x0=0, y0=0):
    """World positions (..., 3) into the rectangle-local film coordinates (u, v) of the camera `frame`, and the depth
    coordinate c (reusable iff c > 0 and finite): primary_ray's film mapping inverted at the mean of sample 8's
    stratum."""
    _, _, _, eye = frame_parts(frame)
    abc = (np.asarray(pos, np.float64) - eye) @ inverse_frame(frame).T
    a, b, c = abc[..., 0], abc[..., 1], abc[..., 2]
    with np.errstate(all="ignore"):
        u = (a / c) * W - 17.0 / 32.0 - x0
        v = (H + 17.0 / 32.0 - (b / c) * H) - y0
    return u, v, c


def blend(c_new, n, pos, nrm, key, frame, prev, W, H, x0=0, y0=0, max_history=64.0, normal_tol=0.5, plane_tol=2.0):
    """The temporal blend of one frame.  c_new (h, w, 3) linear rgb of n samples with guides pos, nrm (h, w, 3), key
    (h, w) and camera `frame`; prev = None or a dict(c=(h, w, 3), hw=(h, w), pos=, nrm=, key=, frame=) of the previous
    slot.  Returns (c, Hw, doubt): doubt marks the pixels whose decisions float32 may take differently -- some tap's
    normal or plane test value within 1 % of its threshold, or u / v within 1e-4 of an integer."""
    c_new = np.asarray(c_new, np.float64)[..., :3]
    hh, ww = c_new.shape[:2]
    c_out = c_new.copy()
    hw_out = np.full((hh, ww), float(n))
    doubt = np.zeros((hh, ww), bool)
    if prev is None:
        return c_out, hw_out, doubt
    pos, nrm, key = np.asarray(pos, np.float64), np.asarray(nrm, np.float64), np.asarray(key)
    take = (key != MISS) & ((key.astype(np.uint64) >> np.uint64(24)) != GLASS) & np.isfinite(c_new).all(-1)
    u, v, c = reproject(prev["frame"], pos, W, H, x0, y0)
    with np.errstate(all="ignore"):
        take &= (c > 0) & np.isfinite(c) & np.isfinite(u) & np.isfinite(v)
        take &= (u >= -1) & (u < ww) & (v >= -1) & (v < hh)         # (beyond these no tap lies inside the rectangle)
    u, v = np.where(take, u, 0.0), np.where(take, v, 0.0)
    fu, fv = np.floor(u), np.floor(v)
    fx, fy = u - fu, v - fv
    doubt |= take & ((np.abs(u - np.round(u)) <= 1e-4) | (np.abs(v - np.round(v)) <= 1e-4))
    _, _, _, eye = frame_parts(frame)
    _, _, _, eye_p = frame_parts(prev["frame"])
    r_p = np.maximum(kappa(frame, W) * np.linalg.norm(pos - eye, axis=-1), kappa(prev["frame"], W) * np.linalg.norm(pos - eye_p, axis=-1))
    p_c, p_hw = np.asarray(prev["c"], np.float64)[..., :3], np.asarray(prev["hw"], np.float64)
    p_pos, p_nrm, p_key = np.asarray(prev["pos"], np.float64), np.asarray(prev["nrm"], np.float64), np.asarray(prev["key"])
    sw, sh, sc = np.zeros((hh, ww)), np.zeros((hh, ww)), np.zeros((hh, ww, 3))
    for dy in (0, 1):
        for dx in (0, 1):
            qx, qy = fu.astype(np.int64) + dx, fv.astype(np.int64) + dy
            ok = take & (qx >= 0) & (qx < ww) & (qy >= 0) & (qy < hh)
            qx, qy = np.clip(qx, 0, ww - 1), np.clip(qy, 0, hh - 1)
            ok &= p_key[qy, qx] == key
            ok &= (p_hw[qy, qx] > 0) & np.isfinite(p_c[qy, qx]).all(-1)
            with np.errstate(all="ignore"):
                dn2 = ((nrm - p_nrm[qy, qx]) ** 2).sum(-1)
                pl = np.abs((nrm * (p_pos[qy, qx] - pos)).sum(-1))
                lim = plane_tol * r_p
                doubt |= ok & ((np.abs(dn2 - normal_tol ** 2) <= 0.01 * normal_tol ** 2) | (np.abs(pl - lim) <= 0.01 * lim))
                ok &= (dn2 <= normal_tol ** 2) & (pl <= lim)
            w = np.where(ok, (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy), 0.0)
            sw += w
            sc += w[..., None] * np.where(ok[..., None], p_c[qy, qx], 0.0)
            sh += w * np.where(ok, p_hw[qy, qx], 0.0)
    got = sw > 0
    sws = np.where(got, sw, 1.0)
    h = sc / sws[..., None]
    hp = np.minimum(sh / sws, max_history)
    c_out = np.where(got[..., None], (n * c_new + hp[..., None] * h) / (n + hp)[..., None], c_new)
    hw_out = np.where(got, n + hp, float(n))
    return c_out, hw_out, doubt


def slot(c, hw, gbuf, key, frame):
    """A history slot from a blend's result and that frame's G-buffer (h, w, 8), keys and camera frame."""
    return dict(c=np.asarray(c, np.float64)[..., :3], hw=np.asarray(hw, np.float64), pos=gbuf[..., 1:4], nrm=gbuf[..., 4:7],
                key=key, frame=np.asarray(frame, np.float64))


def temporal(accum, n, gbuf, key, frame, prev, W, H, x0=0, y0=0, **params):
    """crt_denoise_temporal of one frame: (filtered (h, w, 3), blended c, Hw, doubt)."""
    p = dict(DEFAULTS, **params)
    c, hw, doubt = blend(ref.linear_rgb(accum, n), n, gbuf[..., 1:4], gbuf[..., 4:7], key, frame, prev, W, H, x0, y0,
                         **{k: p[k] for k in BLEND})
    out = ref.atrous(c, gbuf[..., 1:4], gbuf[..., 4:7], key, **{k: v for k, v in p.items() if k not in BLEND})
    return out, c, hw, doubt
