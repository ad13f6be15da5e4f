"""The numpy restatement of crt_denoise_svgf's spatial variance estimate (option "svgf_spatial_pct", include/crt.h
"Variance-guided temporal filter"), in float64, and the mini atrium its quality is measured on.  A helper
module, not collected by pytest.

6j changes one thing in 6g: the v of a pixel that is not `known` (denoise_svgf_ref.variance's own mask) and not excluded
comes from the precision-weighted spread of m1 over the 7x7 taps that share its key.  Blend, moments and passes are
denoise_svgf_ref's and denoise_adaptive_ref's, called as they are."""
import numpy as np

import denoise_adaptive_ref as aref
import denoise_ref as ref
import denoise_svgf_ref as sref
import denoise_temporal_adaptive_ref as atref
import denoise_temporal_ref as tref

MISS = ref.MISS
RADIUS = 3                  # the 7x7 window
A_MIN = 4.0                 # the least sum of weights an estimate is taken from
A_DOUBT = 4e-4              # |A - A_MIN| within this: float32 may decide A >= A_MIN the other way (49 additions into a sum <= 49
                            # carry at most 49 * 49 * 2^-24 = 1.4e-4 of rounding, the weights' own errors about 1e-6 each)
FLT_MAX = float(np.finfo(np.float32).max)


def holds(mom):
    """A pixel's moments can take part, as centre or as tap: m1 and Mw finite, Mw > 0."""
    mom = np.asarray(mom, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(mom[..., 0]) & np.isfinite(mom[..., 2]) & (mom[..., 2] > 0)


def eligible(mom, known, key):
    """The pixels that take the estimate: not known, a hit, not glass, moments that hold."""
    key = np.asarray(key).astype(np.uint64)
    return ~np.asarray(known, bool) & (key != np.uint64(MISS)) & ((key >> np.uint64(24)) != np.uint64(tref.GLASS)) & holds(mom)


def spatial_variance(mom, known, gbuf, key, b, sigma_normal=0.5, sigma_plane=0.3):
    """mom (h, w, >=3) = (m1, s, Mw) of the frame, known (h, w) = denoise_svgf_ref.variance's mask, gbuf (h, w, 8) and
    key (h, w) the frame's guides, b = P / 100.  Returns (v, A, doubt): v (h, w) is what a pixel that is not known
    carries (the estimate, or 1 where it is excluded, where A < 4 or where the value is not finite; 1 on known pixels
    too: the caller keeps 6g's v there), A the sum of weights (0 where no estimate runs), doubt the pixels whose A lies
    within A_DOUBT of the threshold."""
    mom = np.asarray(mom, np.float64)
    key = np.asarray(key).astype(np.uint64)
    pos, nrm = np.asarray(gbuf, np.float64)[..., 1:4], np.asarray(gbuf, np.float64)[..., 4:7]
    m1, mw = mom[..., 0], mom[..., 2]
    hh, ww = key.shape
    tap_ok = holds(mom)
    elig = eligible(mom, known, key)
    taps = []                                                   # per offset in row-major order: (P, Q, w over P, 0 where refused)
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            if abs(dy) >= hh or abs(dx) >= ww:
                continue
            P, Q = aref._shift(hh, ww, dy, dx)
            if dx == 0 and dy == 0:
                taps.append((P, Q, np.ones((hh, ww)), np.ones((hh, ww), bool)))
                continue
            ok = tap_ok[Q] & (key[P] == key[Q])
            with np.errstate(all="ignore"):
                d = pos[Q] - pos[P]
                dl = np.sqrt((d * d).sum(-1))
                e = ((nrm[P] - nrm[Q]) ** 2).sum(-1) / sigma_normal ** 2
                e = e + np.where(dl > 0, (np.abs((nrm[P] * d).sum(-1)) / np.where(dl > 0, dl, 1.0)) / sigma_plane, 0.0)
                w = np.exp(-e)
            taps.append((P, Q, w, ok))
    A, B, C, S = (np.zeros((hh, ww)) for _ in range(4))
    with np.errstate(all="ignore"):
        for P, Q, w, ok in taps:
            wm = w * np.where(ok, mw[Q], 0.0)
            A[P] += np.where(ok, w, 0.0)
            B[P] += np.where(ok, wm, 0.0)
            C[P] += np.where(ok, wm * np.where(ok, m1[Q], 0.0), 0.0)
        mu = C / B
        for P, Q, w, ok in taps:
            wm = w * np.where(ok, mw[Q], 0.0)
            d = np.where(ok, m1[Q], 0.0) - mu[P]
            S[P] += np.where(ok, wm * (d * d), 0.0)
        g = 2.2 * np.exp(-2.2 * np.maximum(mu, 0.0))
        t = b * ((g * g) * ((S / (A - 1.0)) / mw))
        take = elig & (A >= A_MIN) & np.isfinite(t) & (np.abs(t) <= FLT_MAX)
    v = np.where(take, t, 1.0)
    with np.errstate(invalid="ignore"):
        doubt = elig & (np.abs(A - A_MIN) <= A_DOUBT)
    return v, np.where(elig, A, 0.0), doubt


def svgf(accum, n, gbuf, key, frame, prev, W, H, x0=0, y0=0, prims_cur=None, spatial_pct=400, **params):
    """crt_denoise_svgf of one frame with option "svgf_spatial_pct" = spatial_pct (0: denoise_svgf_ref.svgf itself).  n is
    the frame's sample count, or (h, w) counts per pixel for the adaptive state (denoise_temporal_adaptive_ref).  Returns
    (filtered c, variance left, blended c, Hw, mom, doubt of the blend, v that entered the passes, doubt of the estimate)."""
    p = dict(sref.DEFAULTS, **params)
    src = atref if np.ndim(n) else sref
    c, hw, mom, doubt = src.blend(accum, n, gbuf, key, frame, prev, W, H, x0, y0, prims_cur, **{k: p[k] for k in sref.BLEND})
    v, known = src.variance(mom, n, p["min_frames"])
    doubt_s = np.zeros(known.shape, bool)
    if spatial_pct:
        vs, _, doubt_s = spatial_variance(mom, known, gbuf, key, spatial_pct / 100.0, p["sigma_normal"], p["sigma_plane"])
        v = np.where(known, v, vs)
    out, v_out = aref.atrous_var(c, v, gbuf[..., 1:4], gbuf[..., 4:7], key, **{k: p[k] for k in sref.FILTER})
    return out, v_out, c, hw, mom, doubt, v, doubt_s


# ------------------------------------------------------------------ the mini atrium
def mini_atrium(width=64, height=64):
    """A 710-primitive reduction of scenes_synth.atrium250k that a brute-force oracle can render: the six base patches, a
    heightfield of 9 x 9 vertices (128 triangles, five times the relief) and 16 columns of 6 segments x 4 rings (576
    triangles) on a 4 x 4 grid, with atrium250k's radii, heights, entasis and reflectance cycle."""
    from computeraytracer_amd import scenes_synth as ss
    base = ss._base(width, height)
    idx = base.spectrum_index
    g = np.arange(9) / 8.0
    gx, gz = np.meshgrid(g, g, indexing="ij")
    h = 0.65 * ss._value_noise(gx, gz, 4, ss.SEED_ATRIUM) + 0.35 * ss._value_noise(gx, gz, 8, ss.SEED_ATRIUM + 1)
    P = np.stack([1.0 + 553.0 * gx, 0.5 + 40.0 * h, 1.0 + 553.0 * gz], axis=-1)
    v0, v1, v2 = ss._grid_tris(P, False, False)
    refl = [np.full(len(v0), idx["white"])]
    V0, V1, V2 = [v0], [v1], [v2]
    ring = ss._circle(6, 0.5, 0.8660254037844386)                 # cos, sin of 60 degrees
    cycle = [idx["white"], idx["red"], idx["green"]]
    yy = np.arange(4) / 3.0
    for k in range(16):
        ci, cj = k % 4, k // 4
        cx, cz = 555.0 * (ci + 0.5) / 4.0, 555.0 * (cj + 0.5) / 4.0
        u = ss.counter_u01(ss.SEED_ATRIUM + 2, np.asarray([3 * k, 3 * k + 1, 3 * k + 2]))
        r0 = 9.0 + 5.0 * u[0]
        top = 380.0 + 160.0 * u[1]
        bulge = 0.15 + 0.25 * u[2]
        rad = r0 * (1.0 + bulge * (4.0 * yy * (1.0 - yy)) - 0.3 * yy)
        Pc = np.stack([cx + rad[None, :] * ring[:, 0][:, None],
                       0.0 * ring[:, 0][:, None] + (9.0 + (top - 9.0) * yy)[None, :],
                       cz + rad[None, :] * ring[:, 1][:, None]], axis=-1)
        a, b, c = ss._grid_tris(Pc, True, False)
        V0.append(a); V1.append(b); V2.append(c)
        refl.append(np.full(len(a), cycle[(k + 1) % 3]))
    return ss._with_triangles(base, np.concatenate(V0), np.concatenate(V1), np.concatenate(V2), np.concatenate(refl))
