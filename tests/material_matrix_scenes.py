"""Scenes that render the (category x material) pairs no other test scene holds: glass patches, glass triangles,
triangle lights, sphere lights, a scene without a patch and a scene of spheres only.  Built in code from cornell's
walls, camera, spectra and CIE table; index = array position everywhere.  A helper module, not collected by pytest;
tests/test_material_matrix_cpu.py asserts on the oracle that the scenes reach the pairs they are made for."""
import numpy as np

from computeraytracer_amd import scene as S

PATCH, SPHERE, TRI = S.CATEGORY["patch"], S.CATEGORY["sphere"], S.CATEGORY["triangle"]
DIFFUSE, LIGHT, GLASS = S.TYPE_INDEX["diffuse"], S.TYPE_INDEX["light"], S.TYPE_INDEX["glass"]
NAMES = ("tri", "sphere", "patch", "tri_only", "sphere_only")
WALLS = [0, 1, 3, 4, 5]                         # cornell's floor, ceiling, back, right (red) and left (green) wall


def _box_faces(origin, size):
    """(origin, e1, e2) of the six faces of an axis-aligned box."""
    o = np.asarray(origin, np.float64)
    sx, sy, sz = (float(v) for v in size)
    ex, ey, ez = [sx, 0, 0], [0, sy, 0], [0, 0, sz]
    return [(o, ex, ey), (o, ey, ez), (o, ez, ex),
            (o + [0, 0, sz], ex, ey), (o + [sx, 0, 0], ey, ez), (o + [0, sy, 0], ez, ex)]


def _as_triangles(quads):
    """Each parallelogram (o, e1, e2) as the triangles (o, e1, e2) and (o + e1 + e2, -e1, -e2)."""
    out = []
    for o, e1, e2 in quads:
        o, e1, e2 = (np.asarray(v, np.float64) for v in (o, e1, e2))
        out += [(o, e1, e2), (o + e1 + e2, -e1, -e2)]
    return out


def _records(category, geo, emission, reflectance, material):
    n = len(geo)
    one = lambda v: np.full(n, v, np.uint32) if np.isscalar(v) else np.asarray(v, np.uint32)
    return S.make_primitives(np.full(n, category, np.uint32), [g[0] for g in geo], [g[1] for g in geo], [g[2] for g in geo],
                             one(emission), one(reflectance), one(material))


def _pack(base, parts, camera=None):
    prims = np.zeros(sum(len(p) for p in parts), S.PRIM_DTYPE)       # (a fresh array keeps the 80-byte stride)
    prims[:] = np.concatenate(parts)
    prims["data4"][:, 3] = np.arange(len(prims))
    return S.PackedScene(prims, S.lights_of(prims), base.camera if camera is None else camera, base.spectra, base.cie,
                         spectrum_index=base.spectrum_index)


def _glass_tri_cube(idx):
    return _records(TRI, _as_triangles(_box_faces((330, 40, 200), (140, 140, 140))), idx["dark"], idx["white"], GLASS)


def matrix(w, h, light):
    """Cornell's walls, a glass box of six patches, a glass cube of twelve triangles, two diffuse triangles and
    light = "tri": two triangle lights of different emission spectra just under the ceiling (several lights: the
                   per-lane gather of the light record);
            "sphere": a sphere light followed by cornell's patch light (the area read through lights[emission index],
                   clamped to the last light, is then the patch's: the image stays finite);
            "patch": cornell's light alone -- the control."""
    c = S.cornell(w, h)
    idx = c.spectrum_index
    parts = [c.primitives[WALLS],
             _records(PATCH, _box_faces((60, 0.5, 120), (150, 200, 110)), idx["dark"], idx["white"], GLASS),
             _glass_tri_cube(idx),
             _records(TRI, [((250, 0.5, 60), (120, 0, 0), (60, 130, 40)), ((250, 0.5, 60), (60, 130, 40), (0, 0, 90))],
                      idx["dark"], [idx["green"], idx["white"]], DIFFUSE)]
    if light == "tri":
        parts.append(_records(TRI, [((213, 554, 227), (130, 0, 0), (0, 0, 105)), ((343, 554, 332), (-130, 0, 0), (0, 0, -105))],
                              [idx["light"], idx["lightAlt"]], idx["white"], LIGHT))
    elif light == "sphere":
        parts.append(_records(SPHERE, [((278, 480, 280), (40, 40, 40), (0, 0, 0))], idx["light"], idx["white"], LIGHT))
        parts.append(c.primitives[2:3])
    elif light == "patch":
        parts.append(c.primitives[2:3])
    else:
        raise ValueError(light)
    return _pack(c, parts)


def tri_only(w, h):
    """No patch and no sphere: the walls as triangle pairs, the glass triangle cube and ONE triangle light (the
    one-light scalar load of the light record holds a triangle)."""
    c = S.cornell(w, h)
    idx = c.spectrum_index
    walls = c.primitives[WALLS]
    quads = [(p["data1"], p["data2"], p["data3"]) for p in walls]
    parts = [_records(TRI, _as_triangles(quads), idx["dark"], np.repeat(walls["data4"][:, 1], 2), DIFFUSE),
             _glass_tri_cube(idx),
             _records(TRI, [((213, 554, 227), (130, 0, 0), (0, 0, 105))], idx["light"], idx["white"], LIGHT)]
    ps = _pack(c, parts)
    assert (ps.primitives["category"] == TRI).all() and len(ps.lights) == 1
    return ps


def sphere_only(w, h):
    """Four spheres: a huge diffuse floor, a diffuse sphere, a glass sphere and a sphere LIGHT.  The light record's
    data3 is 0, so its area is 0 and pdf_area is inf: the NEE term and the MIS weight are NaN wherever the light
    contributes (the contract; the oracle does the same).  The camera looks down at the group so that little is sky."""
    c = S.cornell(w, h)
    idx = c.spectrum_index
    R = 20000.0
    geo = [((278, -R, 280), (R, R, R), (0, 0, 0)),
           ((150, 90, 330), (90, 90, 90), (0, 0, 0)),
           ((420, 80, 200), (80, 80, 80), (0, 0, 0)),
           ((290, 290, 300), (140, 140, 140), (0, 0, 0))]
    prims = S.make_primitives([SPHERE] * 4, [g[0] for g in geo], [g[1] for g in geo], [g[2] for g in geo],
                              [idx["dark"], idx["dark"], idx["dark"], idx["light"]],
                              [idx["white"], idx["red"], idx["white"], idx["white"]], [DIFFUSE, DIFFUSE, GLASS, LIGHT])
    cam = c.camera.copy()
    cam[0:3] = (278, 600, -550)
    cam[4:7] = (278, 120, 280)
    return _pack(c, [prims], cam)


def build(name, w=96, h=96):
    if name in ("tri", "sphere", "patch"):
        return matrix(w, h, name)
    return {"tri_only": tri_only, "sphere_only": sphere_only}[name](w, h)
