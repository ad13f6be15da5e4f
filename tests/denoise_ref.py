"""The numpy restatement of crt_denoise (include/crt.h, DESIGN.md "Denoised preview"), in float64: the yardstick the
GPU filter is checked against.  A helper module, not collected by pytest."""
import numpy as np

MISS = 0xFFFFFFFF
H = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])
# the XYZ -> linear sRGB matrix of tonemap_rgba8 (crt_shade.h)
M = np.array([[3.2404542, -1.5371385, -0.4985314],
              [-0.9692660, 1.8760108, 0.0415560],
              [0.0556434, -0.2040259, 1.0572252]])
DEFAULTS = dict(iterations=5, sigma_color=1.0, sigma_normal=0.5, sigma_plane=0.3)


def linear_rgb(accum, n):
    """c = M (accum / n) per pixel, float64 (accum: (H, W, >=3) XYZ sums, n: the sample count)."""
    return (np.asarray(accum, np.float64)[..., :3] / float(n)) @ M.T


def linear_rgb_f32(accum, n):
    """The same in the device's float32 operations and order (a sum of three products, left to right, no fma)."""
    a = np.asarray(accum, np.float32)[..., :3] / np.float32(n)
    m = M.astype(np.float32)
    return np.stack([(m[r, 0] * a[..., 0] + m[r, 1] * a[..., 1]) + m[r, 2] * a[..., 2] for r in range(3)], -1)


def display(c):
    """T(c) = 1 - exp(-2.2 max(c, 0)) per channel: the exposure curve colour distances are measured in."""
    return 1.0 - np.exp(-2.2 * np.maximum(np.asarray(c, np.float64), 0.0))


def keys(gbuf, primitives):
    """Material key per pixel from a G-buffer (H, W, 8) and the scene's 80-byte records: material << 24 | reflectance
    index of the hit primitive (data4.z, data4.y), MISS where the ray left the scene."""
    idx = np.ascontiguousarray(gbuf[..., 7], np.float32).view(np.uint32)
    d4 = np.asarray(primitives)["data4"].astype(np.uint64)
    hit = idx != MISS
    k = np.full(idx.shape, MISS, np.uint64)
    k[hit] = (d4[idx[hit], 2] << np.uint64(24)) | d4[idx[hit], 1]
    return k


def atrous(c, pos, nrm, key, iterations=5, sigma_color=1.0, sigma_normal=0.5, sigma_plane=0.3, guides=True,
           magnitude=False):
    """K iterations of the edge-aware a-trous filter on linear rgb c (H, W, 3) with per-pixel position, normal
    (H, W, 3) and key (H, W).  guides=False: the same filter with colour weights only (no key, normal or plane
    weights).  Taps outside the image are skipped; so is a tap other than the centre with a non-finite colour.
    magnitude=True also returns |c| carried through the same weights: the scale of the weighted sums, which bounds
    what rounding them in float32 can change (the condition of the result)."""
    c = np.asarray(c, np.float64)[..., :3].copy()
    m = np.abs(c)
    pos = np.asarray(pos, np.float64)
    nrm = np.asarray(nrm, np.float64)
    key = np.asarray(key)
    hit = key != MISS
    hh, ww = c.shape[:2]
    for i in range(iterations):
        s = 1 << i
        t = display(c)
        fin = np.isfinite(c).all(-1)
        sw = np.zeros((hh, ww))
        sc = np.zeros((hh, ww, 3))
        sm = np.zeros((hh, ww, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                if abs(oy) >= hh or abs(ox) >= ww:
                    continue
                P = (slice(max(0, -oy), hh - max(0, oy)), slice(max(0, -ox), ww - max(0, ox)))
                Q = (slice(max(0, oy), hh - max(0, -oy)), slice(max(0, ox), ww - max(0, -ox)))
                w0 = H[dx + 2] * H[dy + 2]
                if dx == 0 and dy == 0:
                    sw[P] += w0
                    sc[P] += w0 * c[P]
                    sm[P] += w0 * m[P]
                    continue
                ok = fin[Q]
                w = w0 * np.exp(-((t[P] - t[Q]) ** 2).sum(-1) / (sigma_color ** 2 * 2.0 ** -i))
                if guides:
                    ok = ok & (key[P] == key[Q])
                    v = pos[Q] - pos[P]
                    vl = np.sqrt((v * v).sum(-1))
                    sine = np.abs((nrm[P] * v).sum(-1)) / np.where(vl > 0, vl, 1.0)
                    w_n = np.exp(-((nrm[P] - nrm[Q]) ** 2).sum(-1) / sigma_normal ** 2)
                    w_x = np.where(vl > 0, np.exp(-sine / sigma_plane), 1.0)
                    w = w * np.where(hit[P], w_n * w_x, 1.0)
                w = np.where(ok, w, 0.0)
                sw[P] += w
                sc[P] += w[..., None] * np.where(ok[..., None], c[Q], 0.0)
                sm[P] += w[..., None] * np.where(ok[..., None], m[Q], 0.0)
        c = sc / sw[..., None]
        m = sm / sw[..., None]
    return (c, m) if magnitude else c


def atrous_gbuffer(c, gbuf, primitives, guides=True, **params):
    """atrous() guided by a G-buffer as crt_read_gbuffer returns it."""
    p = dict(DEFAULTS, **params)
    return atrous(c, gbuf[..., 1:4], gbuf[..., 4:7], keys(gbuf, primitives), guides=guides, **p)


def to_rgba8(c):
    """The reference's colour tail (tonemap_rgba8 after the matrix): exposure, gamma with the G-channel bug, unorm8."""
    c = np.asarray(c, np.float64)[..., :3]
    t = 1.0 - np.exp(-c * 2.2)
    srgb = 1.055 * np.power(np.maximum(t, 1e-30), 1.0 / 2.4) - 0.055
    r = np.where(t < 0.0031308, t * 12.92, srgb)
    g = np.where(t < 0.0031308, t * (12.92 * t), srgb)
    out = np.stack([r[..., 0], g[..., 1], r[..., 2]], -1)
    out = np.where(out > 0, np.minimum(out, 1.0), 0.0)
    rgba = np.full(c.shape[:2] + (4,), 255, np.uint8)
    rgba[..., :3] = np.floor(out * 255.0 + 0.5).astype(np.uint8)
    return rgba


def mse_display(a, b):
    """Mean squared error in display space T, over every pixel and channel."""
    return float(((display(a) - display(b)) ** 2).mean())


def oracle_gbuffer(orc, ps, rect, full_log=True):
    """The oracle's G-buffer of rect = (x0, y0, tw, th): the first ray of ray_log(x, y, 8), its t, normal and hit index
    and orc.intersect's position.  full_log=False takes the camera ray from a scene without primitives (the ray depends
    on the camera only) and everything else from orc.intersect: the same record without tracing whole paths through a
    large scene on the CPU."""
    x0, y0, tw, th = rect
    sc = orc.Scene.from_packed(ps)
    cam = sc if full_log else orc.Scene(ps.primitives[:0], ps.lights, ps.spectra, ps.cie, ps.camera)
    out = np.zeros((th, tw, 8), np.float32)
    hit = np.zeros((th, tw), bool)
    for y in range(th):
        for x in range(tw):
            log = cam.ray_log(x0 + x, y0 + y, 8, cap=1)[0]
            of, ou = sc.intersect(log[0:3], log[3:6])
            if full_log:
                out[y, x, 0], out[y, x, 4:7], out[y, x, 7] = log[8], log[9:12], log[7]
                hit[y, x] = int(log[7:8].view(np.uint32)[0]) != MISS
            else:
                out[y, x, 0], out[y, x, 4:7] = of[0], of[4:7]
                out[y, x, 7:8] = np.uint32([ou[1] if ou[0] else MISS]).view(np.float32)
                hit[y, x] = bool(ou[0])
            out[y, x, 1:4] = of[1:4]
    return out, hit
