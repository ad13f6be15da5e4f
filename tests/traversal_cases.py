"""Scenes and rays for the ray-level parity tests of the wavefront traversal kernels (test_traversal_rays_gpu.py runs
them on the GPU, test_traversal_cases_cpu.py checks the generators against the oracle).  Pure numpy.

A CASE is a small scene in free space (a few to a few thousand primitives) that is hard on a BVH: coincident,
grid-aligned, degenerate, flat, far from the origin, unbounded, or deep.  A ray CLASS is a family of rays aimed at what
a traversal kernel can get wrong: exact vertices and shared edges, axis-parallel directions whose zero components sit
around the 1e-20 clamp of the slab set-up, origins inside a primitive's plane, hits around t_min, exact ties.

Everything that judges the rays (hit rates, who wins a tie, visibility) is computed from a REFERENCE -- a callable
(o, d, exclude) -> (t float32, index uint32), the oracle's loop or the GPU's brute-force loop -- never from the kernel
under test."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

MAXU = 0xFFFFFFFF
F = np.float32
T_MIN = F(0.001)

# zero components of an axis-parallel direction: around the 1e-20 clamp of the slab set-up (|d| > 1e-20 ? d :
# copysign(1e-20, d)), both zeros, a tiny normal number, the smallest normal and the smallest denormal
TINY = np.array([0.0, -0.0, 1e-20, -1e-20, 0.99e-20, -0.99e-20, 1.01e-20, -1.01e-20, 1e-30, 1.17549435e-38, 1.4e-45,
                 -1.4e-45], np.float32)


@dataclass
class Case:
    name: str
    prims: np.ndarray                       # PRIM_DTYPE, index = position
    lights: list = field(default_factory=list)     # primitives that serve as the "light" of the shadow classes
    tie_lights: list = field(default_factory=list)  # (light, "higher" | "lower"): an occluder of that index order sits at exactly the light's t
    group: np.ndarray | None = None         # coincident cases: primitives with the same group id are the same geometry
    plane_y: float | None = None            # case 4: the triangles of the quad lie in y = plane_y
    flat: bool = False                      # every primitive in one plane: nothing can occlude, in-plane rays hit nothing
    shadow_close: float = 0.4               # share of the shadow rays that start between an occluder and the light, at any distance from it
    shadow_near: float = 4e-3               # ... and the least such distance (a few float32 steps of the coordinates at the very least)
    shadow_exclude: int | None = None       # the plain shadow class excludes this primitive on every second ray (else a random one):
                                            # where only a copy of the light can hide it, the copy is "the surface the ray leaves"
    eye: np.ndarray | None = None           # camera eye (sets the scene scale the origins stay inside)
    ps: object = None                       # a ready PackedScene (the baseline case), else packed() makes one


# ------------------------------------------------------------------ primitives
def _scene():
    from computeraytracer_amd import scene as S
    return S


def tris(v0, v1, v2, first_index=0):
    S = _scene()
    v0, v1, v2 = (np.asarray(v, np.float32).reshape(-1, 3) for v in (v0, v1, v2))
    n = len(v0)
    return S.make_primitives([2] * n, v0, v1 - v0, v2 - v0, [0] * n, [1] * n, [0] * n, first_index=first_index)


def patches(p0, e1, e2, first_index=0):
    S = _scene()
    p0 = np.asarray(p0, np.float32).reshape(-1, 3)
    n = len(p0)
    return S.make_primitives([0] * n, p0, e1, e2, [0] * n, [1] * n, [0] * n, first_index=first_index)


def spheres(c, r, first_index=0):
    S = _scene()
    c = np.asarray(c, np.float32).reshape(-1, 3)
    n = len(c)
    r = np.asarray(r, np.float32).reshape(n, 1).repeat(3, 1)
    return S.make_primitives([1] * n, c, r, np.zeros((n, 3)), [0] * n, [1] * n, [0] * n, first_index=first_index)


def join(*recs):
    S = _scene()
    out = np.zeros(sum(len(r) for r in recs), S.PRIM_DTYPE)      # (np.concatenate would repack the 80-byte records)
    k = 0
    for r in recs:
        out[k:k + len(r)] = r
        k += len(r)
    out["data4"][:, 3] = np.arange(len(out), dtype=np.uint32)
    return out


def grid_quad(n=16, sp=4.0, origin=(0.0, 0.0, 0.0)):
    """n x n cells of two triangles in the plane y = origin.y, power-of-two spacing: every coordinate is an exact float."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i, j = i.ravel().astype(np.float32), j.ravel().astype(np.float32)
    o = np.asarray(origin, np.float32)

    def p(a, b):
        return np.stack([o[0] + a * F(sp), np.full_like(a, o[1]), o[2] + b * F(sp)], 1).astype(np.float32)
    p00, p10, p01, p11 = p(i, j), p(i + 1, j), p(i, j + 1), p(i + 1, j + 1)
    v0 = np.stack([p00, p11], 1).reshape(-1, 3)
    v1 = np.stack([p10, p01], 1).reshape(-1, 3)
    v2 = np.stack([p01, p10], 1).reshape(-1, 3)
    return tris(v0, v1, v2)


def box_patches(lo, hi):
    """The six faces of an axis-aligned box as patches; face 3 is the top (y = hi.y)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    d = hi - lo
    ex, ey, ez = [d[0], 0, 0], [0, d[1], 0], [0, 0, d[2]]
    return patches([lo, lo, lo, [lo[0], hi[1], lo[2]], [hi[0], lo[1], lo[2]], [lo[0], lo[1], hi[2]]],
                   [ex, ey, ez, ex, ey, ex], [ey, ez, ex, ez, ez, ey])


def corners(prims):
    """Corner points (n, 4, 3) float32 (a triangle repeats its first corner, a sphere gives its box) -- the corners of
    crt_scene.cpp prim_corners."""
    d1, d2, d3 = prims["data1"], prims["data2"], prims["data3"]
    cat = prims["category"]
    c = np.stack([d1, d1 + d2, d1 + d3, np.where((cat == 0)[:, None], (d1 + d2) + d3, d1)], 1).astype(np.float32)
    sph = cat == 1
    if sph.any():
        r = np.abs(d2[sph, :1])
        c[sph] = np.stack([d1[sph] - r, d1[sph] + r, d1[sph] - r, d1[sph] + r], 1)
    return c


def scene_scale(prims, eye):
    with np.errstate(invalid="ignore"):
        c = np.abs(corners(prims)).reshape(-1)
        c = c[~np.isnan(c)]                                   # (the scene scale ignores a NaN coordinate; an infinite one counts)
    return F(max([F(0)] + [F(v) for v in (c.max() if len(c) else 0, *np.abs(np.asarray(eye, np.float32)))]))


def hit_pad(prims, eye):
    return F(scene_scale(prims, eye) * F(2.0 ** -17))


def finite_bounds(prims):
    c = corners(prims).reshape(-1, 3)
    c = c[np.isfinite(c).all(1)]
    return c.min(0), c.max(0)


def default_eye(prims):
    """An eye whose coordinates bound every origin the classes use (centre +- 1.5 extents): origins then stay inside
    the region hit_pad is scaled for."""
    lo, hi = finite_bounds(prims)
    c, R = 0.5 * (lo + hi), max(float((hi - lo).max()), 1.0)
    m = F(np.abs(c).max() + 2.0 * R)
    return np.array([m, m, m], np.float32)


def packed(case, prims=None):
    """The case as a PackedScene: the Cornell box's light record, spectra, CIE table; an 8 x 8 camera at case.eye."""
    if case.ps is not None and prims is None:
        return case.ps
    S = _scene()
    base = case.ps if case.ps is not None else S.cornell(8, 8)
    cam = base.camera.copy()
    if case.ps is None:
        cam[0:3] = case.eye
        cam[4:7] = 0.0
    return S.PackedScene(case.prims if prims is None else prims, base.lights, cam, base.spectra, base.cie)


def single(case, index, prims=None):
    """The scene of one primitive of the case alone (as index 0): what a shadow ray's own light gives it."""
    S = _scene()
    p = (case.prims if prims is None else prims)[index:index + 1].copy()
    p["data4"][:, 3] = 0
    return packed(case, join(p))


def quantisable(prims, eye):
    """quantize_bvh4's rule on the builders' primitive boxes (corner box + 2 hit_pad; a sphere's radial term; a patch
    whose edges do not span a plane, and any non-finite corner, are unbounded): True = 16-byte boxes."""
    pad = hit_pad(prims, eye)
    if not np.isfinite(pad):
        return False
    S = scene_scale(prims, eye)
    c = corners(prims)
    nc = np.where(prims["category"] == 0, 4, np.where(prims["category"] == 1, 2, 3))
    lo_c, hi_c = c[:, 0].copy(), c[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for k in range(1, 4):                                     # std::min / std::max in corner order: a later NaN is dropped
            use = (k < nc)[:, None]
            lo_c = np.where(use & (c[:, k] < lo_c), c[:, k], lo_c)
            hi_c = np.where(use & (c[:, k] > hi_c), c[:, k], hi_c)
    if not (np.isfinite(lo_c).all() and np.isfinite(hi_c).all()):
        return False
    cat = prims["category"]
    e1, e2 = prims["data2"].astype(np.float64), prims["data3"].astype(np.float64)
    g11, g22, g12 = (e1 * e1).sum(1), (e2 * e2).sum(1), (e1 * e2).sum(1)
    with np.errstate(invalid="ignore"):
        strip = (cat == 0) & ~(g11 * g22 - g12 * g12 > 1e-9 * g11 * g22)
    if strip.any():
        return False
    g = np.full(len(prims), F(2) * pad, np.float32)
    r = np.abs(prims["data2"][:, 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = np.where(r > 0, np.minimum(S * S * F(9.5367431640625e-07) / r, S), S).astype(np.float32)
    g = np.where(cat == 1, g + rad, g).astype(np.float32)
    lo = (lo_c - g[:, None]).min(0)
    hi = (hi_c + g[:, None]).max(0)
    ext = np.maximum(hi - lo, F(1e-3))
    mag = np.maximum(np.abs(lo), np.abs(hi))
    return bool((mag <= F(16) * ext).all())


# ------------------------------------------------------------------ the cases
def _finish(case):
    if case.eye is None:
        case.eye = default_eye(case.prims)
    return case


def case_baseline():
    from test_gpu_parity import _mixed_scene
    ps = _mixed_scene(64, 36)
    tri = np.flatnonzero(ps.primitives["category"] == 2)
    return Case("baseline", ps.primitives, lights=[int(tri[len(tri) // 2])], eye=ps.camera[0:3].copy(), ps=ps)


def _tiny_pool():
    return join(tris([[0, 0, 0]], [[8, 0, 0]], [[0, 8, 0]]), tris([[1, 1, 3]], [[9, 2, 3]], [[2, 9, 4]]),
                spheres([[4, 4, -6]], [3]), patches([[-2, -2, 8]], [[12, 0, 0]], [[0, 12, 0]]),
                tris([[3, 0, -2]], [[3, 8, -2]], [[3, 0, 6]]), tris([[0, 5, -3]], [[8, 5, -3]], [[0, 5, 7]]),
                tris([[6, 6, 1]], [[7, 6, 1]], [[6, 7, 2]]), spheres([[10, 2, 2]], [1.5]),
                tris([[-4, 3, 0]], [[-4, 9, 1]], [[-4, 3, 5]]))


def cases_tiny():
    pool = _tiny_pool()
    return [_finish(Case(f"tiny{n}", join(pool[:n]), lights=[0], shadow_close=0.15)) for n in (1, 2, 3, 4, 5, 8, 9)]


def cases_coincident():
    out = []
    t = ([[0, 0, 0]], [[16, 0, 2]], [[3, 12, 5]])
    for m in (2, 5, 300):
        p = join(*[tris(*t) for _ in range(m)])
        out.append(_finish(Case(f"coincident_tri{m}", p, lights=[m - 2], shadow_exclude=m - 1, tie_lights=[(m - 1, "lower"), (m // 2 - (m == 2), "higher")],
                                group=np.zeros(m, int), flat=True)))
    p = join(spheres([[0, 0, 0]], [5]), spheres([[0, 0, 0]], [5]), patches([[-8, -8, 9]], [[16, 0, 0]], [[0, 16, 0]]),
             patches([[-8, -8, 9]], [[16, 0, 0]], [[0, 16, 0]]))
    out.append(_finish(Case("coincident_sphere_patch", p, lights=[2], shadow_exclude=3, tie_lights=[(3, "lower"), (2, "higher")], group=np.array([0, 0, 1, 1]))))
    q = grid_quad()
    p = join(q, q)
    out.append(_finish(Case("coincident_quad", p, lights=[200], shadow_exclude=len(q) + 200, tie_lights=[(len(q) + 200, "lower"), (200, "higher")],
                            group=np.concatenate([np.arange(len(q)), np.arange(len(q))]), flat=True, plane_y=0.0)))
    return out


FREE_CELL = (12 * 16 + 12) * 2        # a triangle of the quad that nothing else touches


def _grid_prims(shift=(0.0, 0.0, 0.0)):
    s = np.asarray(shift, np.float32)
    q = grid_quad(origin=s)
    # the box's top face lies in the quad's plane over cells [4, 8) x [4, 8): patch and triangles tie exactly there
    b = box_patches(s + F([16, -24, 16]), s + F([32, 0, 32]))
    return join(q, b)


def case_grid(name="grid", shift=(0.0, 0.0, 0.0)):
    p = _grid_prims(shift)
    nq = 512
    cell = (5 * 16 + 5) * 2                                       # the first triangle of cell (5, 5): under the box's top face
    return _finish(Case(name, p, lights=[FREE_CELL], tie_lights=[(cell, "higher"), (nq + 3, "lower")], plane_y=float(np.float32(shift[1]))))


def _degenerate_extra():
    return [tris([[8, 4, 8]], [[8, 4, 8]], [[12, 6, 8]]),                 # e1 == 0
            tris([[20, 4, 8]], [[24, 4, 8]], [[28, 4, 8]]),               # e1 parallel to e2
            spheres([[40, 6, 40]], [0.0]),                                # zero radius
            tris([[0, 3, 0]], [[64, 3, 0]], [[0, 3, 64e-6]]),             # needles, aspect 1e6
            tris([[5, 2, 50]], [[5, 2 + 50e-6, 50]], [[5, 2, 0]]),
            tris([[30, 5, 30]], [[30 + 1e-4, 5, 30]], [[30, 5, 30 + 1e-4]]),   # 1e-4 across, beside
            tris([[-5000, 8, -5000]], [[5000, 8, -5000]], [[-5000, 8, 5000]])]  # one 1e4 across


def cases_degenerate():
    # (No patch with a zero edge: its unit normal is 0 / 0, so its t is NaN for every ray, and under the loop's
    # reject-form tests a NaN t is accepted and then never beaten by a later primitive.  With
    # patches([[10, 6, 10]], [[0, 0, 0]], [[0, 0, 6]]) as the LAST primitive of this case the oracle returns NaN for
    # 600 of 600 rays of every class; as the first, for 80-90 % of them.  A NaN best-t makes the result depend on the
    # visiting order, so no tree walk can be held to the loop there: NaN payloads are outside the contract.)
    a = join(_grid_prims(), *_degenerate_extra())
    return [_finish(Case("degenerate", a, lights=[FREE_CELL]))]


def cases_flat():
    out = []
    for c in (0.0, 100.0, 5000.0):
        # (one more triangle in the same plane, over most of the light's cell (5, 5): the only kind of occluder a flat scene has)
        p = join(grid_quad(origin=(0.0, c, 0.0)), tris([[21, c, 16]], [[44, c, 16]], [[21, c, 44]]))
        out.append(_finish(Case(f"flat_y{int(c)}", p, lights=[170], flat=True, plane_y=c)))
    # the grid case moved along x to either side of quantize_bvh4's "mag > 16 * ext" rule (the eye fixed, so that the
    # pad is the same on both sides): the x extent is 64 + 4 pad, so a shift of 14.5 / 15.5 extents puts mag at 15.5 / 16.5
    eye = np.array([2200.0, 2200.0, 2200.0], np.float32)
    for name, k in (("grid_inside_16ext", 14.5), ("grid_outside_16ext", 15.5)):
        c = case_grid(name, (64.0 * k, 0.0, 0.0))
        c.eye = eye
        out.append(c)
    return out


def cases_unbounded():
    g = _grid_prims()
    # (the NaN in the FIRST corner: the builders' corner box starts there and std::min / std::max drop a NaN that comes
    # later -- such a triangle keeps the box of its finite corners, which is sound: no ray can hit it)
    nan = join(g, tris([[np.nan, 3, 8]], [[8, 3, 8]], [[8, 3, 12]]))
    inf = join(g, tris([[8, 3, 8]], [[np.inf, 3, 8]], [[8, 3, 12]]))
    return [_finish(Case("unbounded_nan_vertex", nan, lights=[FREE_CELL])), _finish(Case("unbounded_inf_vertex", inf, lights=[FREE_CELL]))]


def case_deep(n=4096):
    """An LBVH that is a chain: box centres in the Morton cells 1 << (29 - k) (one code bit each: 30 splits on the code
    bits), the primitives at positions 0, 1, 2, 4, 8, ... in cell 0 (a chain on the index bits), the rest in the last
    cell; three triangles per chain cell, every triangle so large that its box holds the region around the origin --
    a ray from there enters every sibling of every level."""
    rng = np.random.default_rng(8)
    cell = np.full((n, 3), 1023, np.int64)
    chain = [i for i in range(n) if i & (i - 1) == 0]             # 0 and the powers of two
    cell[chain] = 0
    rest = [i for i in range(n) if i & (i - 1) != 0]
    for k in range(30):
        j, axis = (29 - k) // 3, 2 - (29 - k) % 3                 # bit 2 of a triplet is x, bit 0 is z
        for i in rest[3 * k:3 * k + 3]:
            cell[i] = 0
            cell[i, axis] = 1 << j
    c = cell.astype(np.float64) + 0.5
    h = rng.integers(1100, 1500, (n, 3)).astype(np.float64)       # half extents: whole numbers, so the box centre is exact
    sx, sz = rng.choice([-1.0, 1.0], (2, n))
    v0 = c + np.stack([-h[:, 0], -h[:, 1], -sz * h[:, 2]], 1)
    v1 = c + np.stack([h[:, 0], -h[:, 1], sz * h[:, 2]], 1)
    v2 = c + np.stack([sx * 0.0, h[:, 1], 0.0 * sz], 1)
    return _finish(Case("deep_lbvh", tris(v0, v1, v2), lights=[rest[40]], shadow_close=0.9))


CHAIN_J = 8                           # case_chain: index bits of its chain below the 30 code bits


def chain_levels(J=CHAIN_J):
    """(cell (n, 3), chain level (n,)) of case_chain's primitives; level -1: the filler in the last cell."""
    n = (1 << J) + 3
    cell = np.full((n, 3), 1023, np.int64)
    level = np.full(n, -1, np.int64)
    zero = {0: 29 + J, 1: 29 + J, 2: 29 + J, 3: 29 + J}           # cell 0: the index -> its chain level
    for j in range(2, J + 1):
        for m in range(3):
            zero[(1 << j) + m] = 30 + (J - j)
    for i, lv in zero.items():
        cell[i], level[i] = 0, lv
    rest = [i for i in range(n) if i not in zero]
    for k in range(30):
        j, axis = (29 - k) // 3, 2 - (29 - k) % 3                 # bit 2 of a triplet is x, bit 0 is z
        for i in rest[3 * k:3 * k + 3]:
            cell[i] = 0
            cell[i, axis] = 1 << j
            level[i] = k
    return cell, level


def case_chain(J=CHAIN_J, shadow_close=0.5):
    """An LBVH that is a chain like case_deep's -- 30 splits on the code bits, then J - 1 on the index bits (cell 0 holds
    the primitives 2^j, 2^j + 1, 2^j + 2 for j = J .. 2 and 0 .. 3) -- whose WIDE tree is as deep as the chain: at
    every chain level the sibling subtree holds three triangles with one and the same box, a cube of half edge
    60 000 - 1 000 x level around its cell, larger than the box of the whole rest of the chain (the cells lie within
    [0, 1024), the next level's cubes are 2 000 narrower).  The collapse opens the larger child first, so a 4-wide node
    takes the three triangles and the rest of the chain: one wide level per BVH2 level, 30 + J levels, and 3 x depth
    passes the 16 + 96 stack entries the default overflow area gives k_wf_trace2.  The primitives left over (all of
    level-0 size) fill the last cell, which also pins the box of the centres to [0.5, 1023.5]."""
    cell, level = chain_levels(J)
    n = len(cell)
    rng = np.random.default_rng(9)
    c = cell.astype(np.float64) + 0.5
    h = np.repeat((60000.0 - 1000.0 * np.maximum(level, 0))[:, None], 3, 1)   # whole numbers: the box centre is exact
    sx, sz = rng.choice([-1.0, 1.0], (2, n))
    v0 = c + np.stack([-h[:, 0], -h[:, 1], -sz * h[:, 2]], 1)
    v1 = c + np.stack([h[:, 0], -h[:, 1], sz * h[:, 2]], 1)
    v2 = c + np.stack([sx * 0.0, h[:, 1], 0.0 * sz], 1)
    # (the triangles lie in two families of parallel planes, z - x = const and z + x = const; a filler triangle of the
    # second family is its outermost plane and can be seen from beyond it -- any other is hidden from nearly everywhere)
    light = int(np.flatnonzero((level == -1) & (sz < 0))[-1])      # (its copies tie with it exactly: the last one wins)
    return _finish(Case("chain_lbvh", tris(v0, v1, v2), lights=[light], shadow_close=shadow_close, shadow_near=16.0))


def all_cases():
    return ([case_baseline()] + cases_tiny() + cases_coincident() + [case_grid()] + cases_degenerate() + cases_flat()
            + cases_unbounded() + [case_deep()])


def edited(case, rng):
    """A third of the primitives moved and shrunk (the refit sub-case): (first, records) runs for update_primitives and
    the edited primitive array.  Shrinking towards the scene's middle keeps the scene box, so a tree that could be
    quantised still can."""
    p = case.prims.copy()
    lo, hi = finite_bounds(p)
    mid = (0.5 * (lo + hi)).astype(np.float32)
    sel = np.zeros(len(p), bool)
    sel[rng.permutation(len(p))[: max(1, len(p) // 3)]] = True
    s = F(0.75)
    d1 = p["data1"][sel]
    p["data1"][sel] = (mid + (d1 - mid) * s).astype(np.float32)
    sph = p["category"][sel] == 1
    p["data2"][sel] = (p["data2"][sel] * s).astype(np.float32)
    p["data3"][sel] = np.where(sph[:, None], p["data3"][sel], p["data3"][sel] * s).astype(np.float32)
    idx = np.flatnonzero(sel)
    runs, start = [], 0
    for k in range(1, len(idx) + 1):
        if k == len(idx) or idx[k] != idx[k - 1] + 1:
            runs.append((int(idx[start]), p[idx[start]:idx[k - 1] + 1]))
            start = k
    return runs, p


# ------------------------------------------------------------------ rays
def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def feature_points(prims):
    """(vertices, edge midpoints, diagonal points, normal axis) of the finite primitives, float32 arithmetic (exact on
    the grids); point k of each array belongs to finite primitive k % len(normal axis), whose normal is that axis
    (-1: not axis-aligned)."""
    d1, d2, d3 = prims["data1"], prims["data2"], prims["data3"]
    ok = np.isfinite(d1).all(1) & np.isfinite(d2).all(1) & np.isfinite(d3).all(1)
    d1, d2, d3, cat = d1[ok], d2[ok], d3[ok], prims["category"][ok]
    nrm = np.cross(d2.astype(np.float64), d3.astype(np.float64))
    naxis = np.where(((nrm != 0).sum(1) == 1) & (cat != 1), np.abs(nrm).argmax(1), -1)
    sph = (cat == 1)[:, None]
    r = d2[:, :1]
    ax, ay, az = F([1, 0, 0]), F([0, 1, 0]), F([0, 0, 1])
    h = F(0.5)
    vert = np.concatenate([np.where(sph, d1 + r * ax, d1), np.where(sph, d1 - r * ay, d1 + d2), np.where(sph, d1 + r * az, d1 + d3)])
    edge = np.concatenate([np.where(sph, d1 - r * ax, d1 + h * d2), np.where(sph, d1 + r * ay, d1 + h * d3),
                           np.where(sph, d1 - r * az, (d1 + h * d2) + h * d3)])
    q = F(0.25)
    diag = np.concatenate([np.where(sph, d1, (d1 + q * d2) + q * d3), np.where(sph, d1, (d1 + h * d2) + q * d3)])
    return vert.astype(np.float32), edge.astype(np.float32), diag.astype(np.float32), naxis, np.flatnonzero(ok)


class Rays:
    def __init__(self, case, prims=None, seed=0):
        self.case = case
        self.prims = case.prims if prims is None else prims
        self.rng = np.random.default_rng(seed)
        self.pad = hit_pad(self.prims, case.eye)
        self.lo, self.hi = finite_bounds(self.prims)
        self.c = 0.5 * (self.lo + self.hi)
        self.R = max(float((self.hi - self.lo).max()), 1.0)
        self.M = float(scene_scale(self.prims, case.eye)) if np.isfinite(scene_scale(self.prims, case.eye)) else float(np.abs(case.eye).max())
        self.vert, self.edge, self.diag, self.naxis, self.finite = feature_points(self.prims)

    def origins(self, n, spread=1.5):
        o = self.c + self.rng.uniform(-spread * self.R, spread * self.R, (n, 3))
        return np.clip(o, -self.M, self.M).astype(np.float32)

    def targets(self, n, with_axis=False):
        k = self.rng.integers(0, 4, n)                            # a quarter vertices, a quarter edge midpoints, half diagonal points
        iv, ie, idg = (self.rng.integers(0, len(a), n) for a in (self.vert, self.edge, self.diag))
        t = np.where((k == 0)[:, None], self.vert[iv], np.where((k == 1)[:, None], self.edge[ie], self.diag[idg])).astype(np.float32)
        if not with_axis:
            return t
        return t, self.naxis[np.where(k == 0, iv, np.where(k == 1, ie, idg)) % len(self.naxis)]

    def away(self, o, d, share=0.15):
        """Turn a share of the rays into sure misses: from outside the scene's bounding sphere, pointing away from it."""
        n = len(o)
        m = self.rng.random(n) < share
        u = _unit(self.rng.normal(size=(n, 3)))
        o2 = np.clip(self.c + u.astype(np.float64) * 1.45 * self.R, -self.M, self.M).astype(np.float32)
        o[m], d[m] = o2[m], u[m]
        return o, d

    def aimed(self, n, jitter):
        tgt = self.targets(n)
        if jitter:
            tgt = (tgt + self.rng.uniform(-4, 4, (n, 3)) * float(self.pad if np.isfinite(self.pad) else 1e-3)).astype(np.float32)
        o = self.origins(n)
        v = tgt.astype(np.float64) - o
        v[np.linalg.norm(v, axis=1) == 0] = [0.0, 1.0, 0.0]
        return self.away(o, _unit(v))

    def axis(self, n):
        tgt, na = self.targets(n, True)
        a = self.rng.integers(0, 3, n)
        a = np.where((na >= 0) & (self.rng.random(n) < 0.7), na, a)      # mostly along the target's own normal (else the ray runs in its plane)
        s = self.rng.choice(F([-1, 1]), n)
        d = TINY[self.rng.integers(0, len(TINY), (n, 3))].copy()
        d[np.arange(n), a] = s
        dist = np.floor(self.rng.uniform(1, 0.9 * self.R + 1, n)).astype(np.float32)     # whole numbers: origins stay on the grid
        o = tgt.copy()
        o[np.arange(n), a] = np.clip(tgt[np.arange(n), a] - s * dist, -self.M, self.M)
        return self.away(o, d, 0.12)

    def in_plane(self, n):
        """Origins exactly in a triangle's / patch's plane (on it, on its edges, beside it), direction in that plane."""
        p = self.prims
        ok = np.flatnonzero((p["category"] != 1) & np.isfinite(p["data1"]).all(1) & np.isfinite(p["data2"]).all(1) & np.isfinite(p["data3"]).all(1))
        k = ok[self.rng.integers(0, len(ok), n)]
        d1, d2, d3 = p["data1"][k], p["data2"][k], p["data3"][k]
        a = (self.rng.integers(-8, 13, (n, 1)) * F(0.25)).astype(np.float32)        # quarters: exact, and 0 / 1 put the origin on an edge
        b = (self.rng.integers(-8, 13, (n, 1)) * F(0.25)).astype(np.float32)
        o = ((d1 + a * d2) + b * d3).astype(np.float32)
        m = self.rng.integers(0, 4, (n, 1))
        sg = self.rng.choice(F([-1, 1]), (n, 1))
        d = sg * np.where(m == 0, d2, np.where(m == 1, d3, np.where(m == 2, d2 + d3, d2 - d3)))
        nz = np.linalg.norm(d.astype(np.float64), axis=1) > 0
        d = np.where(nz[:, None], d, F([1, 0, 0])).astype(np.float32)
        mx = np.abs(d).max(1, keepdims=True)
        return np.clip(o, -self.M, self.M).astype(np.float32), (d / mx).astype(np.float32)   # (largest component 1: exact on the grids)

    def near_tmin(self, n):
        """From just off a surface point back onto it: the hit sits just below, at and just above t_min = 0.001."""
        tgt = self.diag[self.rng.integers(0, len(self.diag), n)]
        d = _unit(self.rng.normal(size=(n, 3)))
        t = (T_MIN * self.rng.choice(F([0.999, 0.9999, 0.99999, 1.0, 1.00001, 1.0001, 1.001, 0.5, 2.0]), (n, 1))).astype(np.float32)
        return np.clip(tgt - d * t, -self.M, self.M).astype(np.float32), d

    def inside(self, n):
        """Origins inside the scene's boxes: just off a primitive's own diagonal point, any direction."""
        tgt = self.diag[self.rng.integers(0, len(self.diag), n)]
        off = _unit(self.rng.normal(size=(n, 3))) * F(8) * (self.pad if np.isfinite(self.pad) else F(1e-3))
        return np.clip(tgt + off, -self.M, self.M).astype(np.float32), _unit(self.rng.normal(size=(n, 3)))

    def inside_many(self, n):
        """Origins inside many boxes at once: within 2 hit_pad of the plane of the grid-built cases' quad (every leaf box
        of the quad there, all their ancestors, and over the patch box's top face that box's too), any direction."""
        lo, hi = self.lo, self.hi
        o = np.stack([self.rng.uniform(lo[0], hi[0], n), self.case.plane_y + self.rng.uniform(-2, 2, n) * float(self.pad),
                      self.rng.uniform(lo[2], hi[2], n)], 1)
        return np.clip(o, -self.M, self.M).astype(np.float32), _unit(self.rng.normal(size=(n, 3)))

    def box_plane(self, n):
        """Origins exactly in a plane of a primitive's box as the builders make it (corner box -/+ 2 hit_pad, in float32:
        crt_scene.cpp upload_geometry) -- a quarter of them in a plane of the scene box, the extreme primitive's -- running
        along that plane: the direction component on the plane's axis comes from TINY (both signs, both sides of the
        1e-20 clamp), the other two aim past the primitive at the rest of the scene."""
        p = self.prims
        ok = np.flatnonzero((p["category"] == 2) & np.isfinite(p["data1"]).all(1) & np.isfinite(p["data2"]).all(1) & np.isfinite(p["data3"]).all(1))
        c = corners(p[ok])[:, :3]
        g = F(2) * self.pad
        lo_p, hi_p = (c.min(1) - g).astype(np.float32), (c.max(1) + g).astype(np.float32)
        a = self.rng.integers(0, 3, n)
        side = self.rng.integers(0, 2, n)
        k = self.rng.integers(0, len(ok), n)
        ext = self.rng.random(n) < 0.25                             # the scene box's plane: the extreme primitive's
        k = np.where(ext, np.where(side == 0, lo_p.argmin(0)[a], hi_p.argmax(0)[a]), k)
        plane = np.where(side == 0, lo_p[k, a], hi_p[k, a])
        tgt = self.targets(n)
        d = _unit(self.rng.normal(size=(n, 3))).astype(np.float32)
        d[np.arange(n), a] = 0
        nz = np.abs(d).sum(1) > 0
        d[~nz] = F([1, 1, 1])
        d[np.arange(n), a] = 0
        d = (d / np.abs(d).max(1, keepdims=True)).astype(np.float32)
        dist = self.rng.uniform(0.05, 0.9, (n, 1)) * self.R
        o = (tgt - d * dist).astype(np.float32)
        o = np.clip(o, -self.M, self.M).astype(np.float32)
        o[np.arange(n), a] = plane
        d[np.arange(n), a] = TINY[self.rng.integers(0, len(TINY), n)]
        assert (np.abs(o) <= self.M).all()
        return o, d

    def miss_box(self, n):
        o, d = self.origins(n), _unit(self.rng.normal(size=(n, 3)))
        return self.away(o, d, 1.0)

    def classes(self, n):
        """[(name, o, d, exclude mode)]: exclude 'none', 'closest' (the reference's closest hit: the runner-up must
        come back) or 'random'."""
        out = [("aimed", *self.aimed(n, False), "none"), ("aimed_jitter", *self.aimed(n, True), "none"),
               ("aimed_excl_closest", *self.aimed(n, False), "closest"), ("aimed_excl_random", *self.aimed(n, True), "random"),
               ("axis", *self.axis(n), "none"), ("axis_excl_closest", *self.axis(n), "closest"),
               ("in_plane", *self.in_plane(n), "none"), ("near_tmin", *self.near_tmin(n), "none"),
               ("near_tmin_excl_closest", *self.near_tmin(n), "closest"),
               ("inside", *self.inside(n), "none"), ("miss_box", *self.miss_box(n), "none")]
        # (an infinite vertex makes every box plane infinite; the class takes the planes of triangles' boxes)
        if np.isfinite(self.pad) and (self.prims["category"][self.finite] == 2).any():
            out.append(("box_plane", *self.box_plane(n), "none"))
        if self.case.plane_y is not None:
            out.append(("inside_many", *self.inside_many(n), "none"))
        if self.case.name in ("deep_lbvh", "chain_lbvh"):         # from the region every box holds
            o = self.rng.uniform(-40, 40, (n, 3)).astype(np.float32)
            out.append(("deep_centre", o, _unit(self.rng.normal(size=(n, 3))), "none"))
        return out

    # -- shadow rays
    def light_points(self, L, n):
        p = self.prims[L]
        hi = 0.9 if p["category"] == 0 else 0.45
        a = self.rng.uniform(0.08, hi, (n, 1)).astype(np.float32)
        b = self.rng.uniform(0.08, hi, (n, 1)).astype(np.float32)
        return ((p["data1"] + a * p["data2"]) + b * p["data3"]).astype(np.float32)

    def shadow(self, L, n):
        """Rays towards points on primitive L: from random points, from behind a point q on another primitive (q is
        in front of the light), and from between q and the light (q is behind the origin)."""
        tgt = self.light_points(L, n).astype(np.float64)
        p = self.prims[L]
        nrm = np.cross(p["data2"].astype(np.float64), p["data3"].astype(np.float64))
        nrm /= np.linalg.norm(nrm)
        other = np.flatnonzero(self.finite[np.arange(len(self.diag)) % len(self.finite)] != L)    # points on the other primitives,
        off = np.abs(((self.diag[other].astype(np.float64) - p["data1"]) * nrm).sum(1)) > 1e-3 * self.R   # off the light's plane if there are any
        other = other[off] if off.any() else other
        close = self.case.shadow_close
        m = self.rng.choice(3, (n, 1), p=[(1 - close) / 2, (1 - close) / 2, close]) if len(other) else np.zeros((n, 1), int)
        q = self.diag[other[self.rng.integers(0, len(other), n)]].astype(np.float64) if len(other) else tgt
        s = self.rng.uniform(0.15, 0.9, (n, 1))
        # (close to the light too, from 0.004 units up: a dense scene blocks every long ray)
        near = self.case.shadow_near
        far = np.maximum(0.9 * np.linalg.norm(q - tgt, axis=1, keepdims=True), 2 * near)
        s2 = np.exp(self.rng.uniform(np.log(near), np.log(far))) / np.maximum(np.linalg.norm(q - tgt, axis=1, keepdims=True), 1e-30)
        o = np.where(m == 0, self.origins(n, 1.0), np.where(m == 1, q + (q - tgt) * s, tgt + (q - tgt) * s2))
        h = ((o - tgt) * nrm).sum(1)
        graze = np.abs(h) < 0.2 * np.linalg.norm(o - tgt, axis=1)               # (nearly) in the light's plane, e.g. a coplanar q: lift it
        lift = self.rng.choice([-1.0, 1.0], n) * self.rng.uniform(0.3, 1.0, n) * np.maximum(np.linalg.norm(o - tgt, axis=1), 1e-2 * self.R)
        o = np.where(graze[:, None], o + nrm * lift[:, None], o)
        o = np.clip(o, -self.M, self.M).astype(np.float32)
        o[np.linalg.norm(tgt - o, axis=1) < 3e-3] = (self.c + 1.2 * self.R).astype(np.float32)      # (the light must lie beyond t_min)
        return o, _unit(tgt - o)

    def shadow_tie(self, L, n):
        """Axis-parallel rays with exact coordinates onto L (the coincident and the grid cases): every occluder that
        shares L's plane there sits at exactly L's t."""
        p = self.prims[L]
        hi = 7 if p["category"] == 0 else 3
        a = (self.rng.integers(1, hi, (n, 1)) * F(0.125)).astype(np.float32)
        b = (self.rng.integers(1, hi, (n, 1)) * F(0.125)).astype(np.float32)
        tgt = ((p["data1"] + a * p["data2"]) + b * p["data3"]).astype(np.float32)
        nrm = np.cross(p["data2"].astype(np.float64), p["data3"].astype(np.float64))
        if p["category"] == 1 or np.count_nonzero(nrm) != 1:      # not axis-aligned: aim along the normal from exact multiples of it
            return None
        ax = int(np.flatnonzero(nrm)[0])
        s = self.rng.choice(F([-1, 1]), n)
        o = tgt.copy()
        o[:, ax] = tgt[:, ax] + s * self.rng.integers(1, 33, n).astype(np.float32)
        d = np.zeros((n, 3), np.float32)
        d[:, ax] = -s
        return np.clip(o, -self.M, self.M).astype(np.float32), d


WALK_N = 500                          # rays per class of the chain case in test_single_ray_walks_gpu.py and its CPU side
WALK_SEED = 10


def state_rays(case, n, seed, prims=None):
    """The rays test_traversal_rays_gpu.State(case, prims, ..., seed, n) makes, draw for draw: [(class name, o, d, light)]
    -- the extension classes (light None), then one shadow class per light and per tie light."""
    R = Rays(case, prims, seed=seed)
    out = [(cname, o, d, None) for cname, o, d, _ in R.classes(n)]
    for L, cname, kind in [(L, "shadow", None) for L in case.lights] + [(L, f"shadow_tie_{k}", k) for L, k in case.tie_lights]:
        od = R.shadow_tie(L, n // 2) if kind else R.shadow(L, n)
        o, d = od if od is not None else R.shadow(L, n // 2)
        out.append((f"{cname}[light {L}]", o, d, L))
    return out


# ------------------------------------------------------------------ judged by a reference
def resolve_exclude(ref, rng, nprim, o, d, mode):
    ex = np.full(len(o), MAXU, np.uint32)
    if mode == "closest":
        ex = ref(o, d, ex)[1].astype(np.uint32)
    elif mode == "random":
        ex = rng.integers(0, nprim, len(o)).astype(np.uint32)
    return ex


def shadow_excludes(case, L, n, nprim, rng):
    """Exclude indices of the plain shadow class of light L: none on every second ray, else case.shadow_exclude or a
    random primitive other than L."""
    ex = np.full(n, MAXU, np.uint32)
    if case.shadow_exclude is not None:
        ex[::2] = case.shadow_exclude
    elif nprim > 1:
        ex[::2] = (L + 1 + rng.integers(0, nprim - 1, len(ex[::2]))) % nprim
    return ex


def shadow_expect(ref_scene, ref_light, L, o, d, ex):
    """(t_light, light-only hit mask, expected visibility, tie with a higher index, tie with a lower index) of shadow
    rays towards primitive L.  ref_light is the reference of single(case, L); visible <=> the closest hit of the
    reference loop (equal t -> later primitive) is L."""
    t_l, i_l = ref_light(o, d, np.full(len(o), MAXU, np.uint32))
    own = (i_l == 0) & (ex != L)
    t, i = ref_scene(o, d, ex)
    vis = own & (i == L)
    t2, i2 = ref_scene(o, d, np.where(ex == MAXU, np.uint32(L), ex).astype(np.uint32))
    tb, t2b, tlb = t.view(np.uint32), t2.view(np.uint32), t_l.view(np.uint32)
    tie_hi = own & (i != L) & (i != MAXU) & (tb == tlb)
    tie_lo = own & (i == L) & (ex == MAXU) & (i2 != MAXU) & (t2b == tlb)
    return t_l, own, vis, tie_hi, tie_lo


def oracle_reference(orc, ps):
    sc = orc.Scene.from_packed(ps)

    def ref(o, d, ex):
        t = np.zeros(len(o), np.float32)
        idx = np.full(len(o), MAXU, np.uint32)
        for k in range(len(o)):
            of, ou = sc.intersect(o[k], d[k], int(ex[k]))
            if ou[0]:
                t[k], idx[k] = of[0], ou[1]
        return t, idx
    return ref
