"""The numpy restatement of clipped history (include/crt.h "Clipped history", option "temporal_clip_pct"), in
float64 and line by line: the box of a pixel from the frame's own 7x7 neighbourhood, and 6e / 6f's blend with the
reprojected history clamped to it.  A helper module, not collected by pytest."""
import numpy as np

import denoise_motion_ref as mref
import denoise_ref as ref
import denoise_temporal_ref as tref

MISS = ref.MISS
RADIUS = 3
MIN_TAPS = 4
F32_MAX = float(np.finfo(np.float32).max)


def has_box(c_new, key):
    """The pixels 6l defines a box for: not a miss, not glass, their own c_new finite."""
    key = np.asarray(key)
    return (key != MISS) & ((key.astype(np.uint64) >> np.uint64(24)) != tref.GLASS) & np.isfinite(np.asarray(c_new)[..., :3]).all(-1)


def box(c_new, key, gamma):
    """The box of every pixel of the rectangle c_new (h, w, 3), key (h, w): (lo (h, w, 3), hi (h, w, 3), N (h, w), valid).
    Taps |dx|, |dy| <= 3 inside the rectangle with the centre's key and a finite colour, row-major; mu = sum / N, a second
    pass for S = sum (c - mu)^2, sigma = sqrt(S / N), lo / hi = mu -+ gamma sigma.  A pixel without a box has N = 0, valid
    False and zeros as bounds; valid iff N >= 4 and every bound is finite as a float32."""
    c = np.asarray(c_new, np.float64)[..., :3]
    key = np.asarray(key)
    hh, ww = key.shape
    fin = np.isfinite(c).all(-1)
    own = has_box(c, key)
    taps = []
    n_t = np.zeros((hh, ww))
    s1 = np.zeros((hh, ww, 3))
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            ys, xs = np.arange(hh) + dy, np.arange(ww) + dx
            inside = ((ys >= 0) & (ys < hh))[:, None] & ((xs >= 0) & (xs < ww))[None, :]
            qy, qx = np.clip(ys, 0, hh - 1)[:, None], np.clip(xs, 0, ww - 1)[None, :]
            ok = own & inside & (key[qy, qx] == key) & fin[qy, qx]
            cq = np.where(ok[..., None], c[qy, qx], 0.0)
            taps.append((ok, cq))
            n_t += ok
            s1 += cq
    n_s = np.where(own, n_t, 1.0)[..., None]
    mu = s1 / n_s
    s2 = np.zeros((hh, ww, 3))
    for ok, cq in taps:
        s2 += np.where(ok[..., None], (cq - mu) ** 2, 0.0)
    with np.errstate(all="ignore"):
        r = gamma * np.sqrt(s2 / n_s)
        lo, hi = mu - r, mu + r
        valid = own & (n_t >= MIN_TAPS) & (np.abs(lo) <= F32_MAX).all(-1) & (np.abs(hi) <= F32_MAX).all(-1)
    lo, hi = np.where(own[..., None], lo, 0.0), np.where(own[..., None], hi, 0.0)
    return lo, hi, np.where(own, n_t, 0.0), valid


def clamp(h, bx):
    """h' = min(max(h, lo), hi) per channel where the box bx = (lo, hi, N, valid) is valid; h elsewhere."""
    lo, hi, _, valid = bx
    return np.where(np.asarray(valid, bool)[..., None], np.minimum(np.maximum(h, lo), hi), h)


def blend(c_new, n, gbuf, key, frame, prev, W, H, x0=0, y0=0, box=None, prims_cur=None, prims_prev=None, max_history=64.0,
          normal_tol=0.5, plane_tol=2.0):
    """6e's blend (6f's with prims_prev: the records the slot `prev` saw, prims_cur those of this frame) with the clamp of
    6l: box = None, or (lo, hi, N, valid) as box() returns it (or as crt_debug_read_clip_box does).  Returns (c, Hw,
    doubt), doubt as in 6e: the clamp adds no decision float32 may take differently."""
    c_new = np.asarray(c_new, np.float64)[..., :3]
    hh, ww = c_new.shape[:2]
    c_out = c_new.copy()
    hw_out = np.full((hh, ww), float(n))
    doubt = np.zeros((hh, ww), bool)
    if prev is None:
        return c_out, hw_out, doubt
    g = np.asarray(gbuf, np.float32)
    pos, nrm, key = g[..., 1:4].astype(np.float64), g[..., 4:7].astype(np.float64), np.asarray(key)
    if prims_prev is None:
        x_t, n_t, ok = pos, nrm, np.ones((hh, ww), bool)
    else:
        x_t, n_t, ok, _ = mref.motion_map(g, prims_cur, prims_prev)
    x_f = x_t.astype(np.float32).astype(np.float64)             # x~ rounded to float: what the taps' tests see
    take = (key != MISS) & ((key.astype(np.uint64) >> np.uint64(24)) != tref.GLASS) & ok & np.isfinite(c_new).all(-1)
    u, v, c = tref.reproject(prev["frame"], x_t, W, H, x0, y0)
    with np.errstate(all="ignore"):
        take &= (c > 0) & np.isfinite(c) & np.isfinite(u) & np.isfinite(v)
        take &= (u >= -1) & (u < ww) & (v >= -1) & (v < hh)
    u, v = np.where(take, u, 0.0), np.where(take, v, 0.0)
    fu, fv = np.floor(u), np.floor(v)
    fx, fy = u - fu, v - fv
    doubt |= take & ((np.abs(u - np.round(u)) <= 1e-4) | (np.abs(v - np.round(v)) <= 1e-4))
    _, _, _, eye = tref.frame_parts(frame)
    _, _, _, eye_p = tref.frame_parts(prev["frame"])
    r_p = np.maximum(tref.kappa(frame, W) * np.linalg.norm(pos - eye, axis=-1),
                     tref.kappa(prev["frame"], W) * np.linalg.norm(x_f - eye_p, axis=-1))
    p_c, p_hw = np.asarray(prev["c"], np.float64)[..., :3], np.asarray(prev["hw"], np.float64)
    p_pos, p_nrm, p_key = np.asarray(prev["pos"], np.float64), np.asarray(prev["nrm"], np.float64), np.asarray(prev["key"])
    sw, sh, sc = np.zeros((hh, ww)), np.zeros((hh, ww)), np.zeros((hh, ww, 3))
    for dy in (0, 1):
        for dx in (0, 1):
            qx, qy = fu.astype(np.int64) + dx, fv.astype(np.int64) + dy
            okq = take & (qx >= 0) & (qx < ww) & (qy >= 0) & (qy < hh)
            qx, qy = np.clip(qx, 0, ww - 1), np.clip(qy, 0, hh - 1)
            okq &= p_key[qy, qx] == key
            okq &= (p_hw[qy, qx] > 0) & np.isfinite(p_c[qy, qx]).all(-1)
            with np.errstate(all="ignore"):
                dn2 = ((n_t - p_nrm[qy, qx]) ** 2).sum(-1)
                pl = np.abs((n_t * (p_pos[qy, qx] - x_f)).sum(-1))
                lim = plane_tol * r_p
                doubt |= okq & ((np.abs(dn2 - normal_tol ** 2) <= 0.01 * normal_tol ** 2) | (np.abs(pl - lim) <= 0.01 * lim))
                okq &= (dn2 <= normal_tol ** 2) & (pl <= lim)
            w = np.where(okq, (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy), 0.0)
            sw += w
            sc += w[..., None] * np.where(okq[..., None], p_c[qy, qx], 0.0)
            sh += w * np.where(okq, p_hw[qy, qx], 0.0)
    got = sw > 0
    sws = np.where(got, sw, 1.0)
    h = sc / sws[..., None]
    if box is not None:
        h = clamp(h, box)
    hp = np.minimum(sh / sws, max_history)
    c_out = np.where(got[..., None], (n * c_new + hp[..., None] * h) / (n + hp)[..., None], c_new)
    hw_out = np.where(got, n + hp, float(n))
    return c_out, hw_out, doubt


# ------------------------------------------------------------------ the light switch the CPU and GPU tests share
DIM = 16.0


def with_dim_row(ps):
    """(scene, dim lights): `ps` with one more emission row E / 16 for every row E a light names, and the light list
    that names those rows.  The primitives stay: crt_update_lights edits what the surfaces receive, and the emitter seen
    directly keeps its record."""
    from computeraytracer_amd.scene import PackedScene
    rows = sorted(set(int(e) for e in ps.lights["data4"][:, 0]))
    spectra = np.concatenate([ps.spectra, (ps.spectra[rows].astype(np.float64) / DIM).astype(np.float32)])
    dim = ps.lights.copy()
    for k, e in enumerate(rows):
        dim["data4"][ps.lights["data4"][:, 0] == e, 0] = len(ps.spectra) + k
    return PackedScene(ps.primitives, ps.lights, ps.camera, spectra, ps.cie, ps.patches, ps.spectrum_index), dim


def temporal(accum, n, gbuf, key, frame, prev, W, H, x0=0, y0=0, gamma=0.0, prims_cur=None, mapped=True, **params):
    """crt_denoise_temporal of one frame under "temporal_clip_pct" = 100 gamma (0: off): (filtered (h, w, 3), blended c,
    Hw, doubt).  prims_cur: the frame's records under "temporal_motion" (prev then carries its own, denoise_motion_ref.slot)."""
    p = dict(tref.DEFAULTS, **params)
    c_new = ref.linear_rgb(accum, n)
    bx = box(c_new, key, gamma) if gamma and prev is not None else None
    old = prev.get("prims") if prev is not None and prims_cur is not None and mapped else None
    c, hw, doubt = blend(c_new, n, gbuf, key, frame, prev, W, H, x0, y0, bx, prims_cur, old, **{k: p[k] for k in tref.BLEND})
    out = ref.atrous(c, gbuf[..., 1:4], gbuf[..., 4:7], key, **{k: v for k, v in p.items() if k not in tref.BLEND})
    return out, c, hw, doubt
