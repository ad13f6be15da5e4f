"""The restatement of crt_render_aovs and crt_spectrum_rgb (include/crt.h "Feature planes"): the camera rays
come from the CPU oracle, the sums are taken sequentially in float32.  A helper module, not collected by pytest."""
import numpy as np

MISS = 0xFFFFFFFF
F = np.float32
INF = F(2139095040.0)            # crt_shade.h CRT_INFINITY: the depth of a pixel none of whose rays hit
PLANES = ("hits", "alpha", "depth", "normal", "albedo")
# the XYZ -> linear sRGB matrix of the tone map (crt_shade.h xyz_to_linear_rgb), as doubles
M = ((3.2404542, -1.5371385, -0.4985314),
     (-0.9692660, 1.8760108, 0.0415560),
     (0.0556434, -0.2040259, 1.0572252))


def spectrum_rgb(spectrum, cie):
    """crt_spectrum_rgb in Python floats (binary64), k ascending: the reflectance under an equal-energy illuminant, white
    Y = 1, through M, each result rounded once to float32."""
    s = [float(v) for v in np.asarray(spectrum, F).reshape(301)]
    c = np.asarray(cie, F).reshape(3, 471)
    cx, cy, cz = ([float(v) for v in c[r]] for r in range(3))
    X = Y = Z = N = 0.0
    for k in range(301):
        X += s[k] * cx[k + 40]
        Y += s[k] * cy[k + 40]
        Z += s[k] * cz[k + 40]
        N += cy[k + 40]
    x, y, z = X / N, Y / N, Z / N
    return np.array([(m[0] * x + m[1] * y) + m[2] * z for m in M], F)


def albedo_table(spectra, cie):
    """One spectrum_rgb per spectra row: (nspectra, 3) float32."""
    return np.stack([spectrum_rgb(row, cie) for row in np.asarray(spectra, F).reshape(-1, 301)])


def camera_hits(orc, ps, rect, n, offset=0, full_log=True):
    """Per pixel of rect = (x0, y0, tw, th) and sample j = 1 .. n, the first hit of the camera ray of sample offset + j:
    (index (th, tw, n) uint32 with MISS, t (th, tw, n) float32, normal (th, tw, n, 3) float32) from ray_log(x, y,
    offset + j, cap=1)[0].  full_log=False takes the camera ray from a scene without primitives and the hit from
    orc.intersect (denoise_ref.oracle_gbuffer's route for a large scene)."""
    x0, y0, tw, th = rect
    sc = orc.Scene.from_packed(ps)
    cam = sc if full_log else orc.Scene(ps.primitives[:0], ps.lights, ps.spectra, ps.cie, ps.camera)
    index = np.full((th, tw, n), MISS, np.uint32)
    t = np.zeros((th, tw, n), F)
    nrm = np.zeros((th, tw, n, 3), F)
    for y in range(th):
        for x in range(tw):
            for j in range(n):
                log = cam.ray_log(x0 + x, y0 + y, offset + j + 1, cap=1)[0]
                if full_log:
                    index[y, x, j] = log[7:8].view(np.uint32)[0]
                    t[y, x, j], nrm[y, x, j] = log[8], log[9:12]
                else:
                    of, ou = sc.intersect(log[0:3], log[3:6])
                    if ou[0]:
                        index[y, x, j] = ou[1]
                    t[y, x, j], nrm[y, x, j] = of[0], of[4:7]
    return index, t, nrm


def planes(ps, index, t, nrm, table=None):
    """The five planes from camera_hits' arrays: sums from +0 in sample order, one float32 operation per step."""
    th, tw, n = index.shape
    table = albedo_table(ps.spectra, ps.cie) if table is None else table
    refl = np.asarray(ps.primitives)["data4"][:, 1].astype(np.int64)
    h = np.zeros((th, tw), np.uint32)
    st = np.zeros((th, tw), F)
    sn = np.zeros((th, tw, 3), F)
    sa = np.zeros((th, tw, 3), F)
    for j in range(n):
        hit = index[..., j] != MISS
        a = np.zeros((th, tw, 3), F)
        a[hit] = table[refl[index[..., j][hit]]]
        h = h + hit.astype(np.uint32)
        st = np.where(hit, st + t[..., j], st).astype(F)
        sn = np.where(hit[..., None], sn + nrm[..., j, :], sn).astype(F)
        sa = np.where(hit[..., None], sa + a, sa).astype(F)
    hf = h.astype(F)
    some = h > 0
    div = np.where(some, hf, F(1))
    out = dict(hits=h, alpha=(hf / F(n)).astype(F), depth=np.where(some, st / div, INF).astype(F),
               normal=np.zeros((th, tw, 4), F), albedo=np.zeros((th, tw, 4), F))
    out["normal"][..., :3] = np.where(some[..., None], sn / div[..., None], F(0))
    out["albedo"][..., :3] = np.where(some[..., None], sa / div[..., None], F(0))
    return out


def oracle_aovs(orc, ps, rect, n, offset=0, full_log=True):
    """(planes, index): the restatement of crt_render_aovs(ctx, n) on rect under sample offset `offset`."""
    index, t, nrm = camera_hits(orc, ps, rect, n, offset, full_log)
    return planes(ps, index, t, nrm), index


def distinct_primitives(index):
    """Per pixel: how many different primitives its camera rays hit."""
    out = np.zeros(index.shape[:2], np.int64)
    for y in range(index.shape[0]):
        for x in range(index.shape[1]):
            v = index[y, x]
            out[y, x] = len(np.unique(v[v != MISS]))
    return out


def assert_planes(got, want, what=""):
    """Bit for bit, plane by plane."""
    for p in PLANES:
        if p not in got:
            continue
        g, w = np.ascontiguousarray(got[p]), np.ascontiguousarray(want[p])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, p, g.shape, w.shape)
        bad = g.view(np.uint32) != w.view(np.uint32)
        assert not bad.any(), f"{what} {p}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0].tolist()}"
