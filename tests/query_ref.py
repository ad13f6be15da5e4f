"""The expectation of the ray queries (include/crt.h "Ray queries"), built from the oracle alone.  Pure
numpy + fractions; test_query_cpu.py checks it without a GPU, test_query_gpu.py holds crt_query_rays / crt_pick to it.

Closest hit.  The oracle's loop gives (t*, i*) and the hit's position and normal per ray, without a limit.  Every
primitive's candidate t is a function of the ray and the primitive alone -- t_max only decides whether the candidate is
accepted -- so under a limit L the loop accepts exactly the candidates t <= L, and its result is (t*, i*) when
i* != MAXU and t* <= L (compared as floats: a NaN L gives a miss), and a miss otherwise.  A miss reports the ray's own
t_max bit for bit, prim = id = 0xFFFFFFFF and zeros everywhere else.

uv.  The surface coordinates the hit test computes (crt_shade.h hit_test_rec / hit_uv_rec) are restated here operation by
operation: +, -, *, / are numpy float32 operations (single IEEE roundings), and every fma is exact -- the product and the
sum formed as Fractions and rounded ONCE to binary32, ties to even (round_f32)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import traversal_cases as TC
from traversal_cases import MAXU

F = np.float32
NO_LIMIT = F(2139095040.0)            # CRT_INFINITY of the kernels
SEED = 41
N_PER_CLASS = 100


# ------------------------------------------------------------------ one rounding
def round_f32(x: Fraction) -> np.float32:
    """The binary32 nearest to the exact x, ties to even; overflow gives an infinity, the subnormal range is exact steps of
    2^-149.  x == 0 gives +0 (the caller decides the sign of an exact zero)."""
    if x == 0:
        return F(0.0)
    s, a = (-1.0, -x) if x < 0 else (1.0, x)
    e = a.numerator.bit_length() - a.denominator.bit_length()       # 2^(e-1) <= a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1                                                      # 2^e <= a < 2^(e+1)
    q = max(e, -126) - 23                                           # the spacing of binary32 at a: 2^q
    n = a / (Fraction(2) ** q)
    r = n.numerator // n.denominator
    rem = n - r
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (r & 1)):
        r += 1
    with np.errstate(over="ignore"):
        return F(s * math.ldexp(float(r), q))                       # r <= 2^24: exact; 2^128 and above become inf


def fma32(a, b, c) -> np.float32:
    """fma(a, b, c) of binary32 values: exact product and sum, one rounding.  A non-finite operand, and the sign of an
    exact zero, are IEEE's (binary64 holds a binary32 product exactly, so its sum has the right sign when it is zero)."""
    a, b, c = F(a), F(b), F(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return F(np.float64(a) * np.float64(b) + np.float64(c))
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return F(float(a) * float(b) + float(c))
    return round_f32(x)


def dot32(a, b):
    """crt_math.h dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    with np.errstate(over="ignore", invalid="ignore"):
        return fma32(a[2], b[2], fma32(a[1], b[1], F(a[0]) * F(b[0])))


def cross32(a, b):
    """crt_math.h cross: (fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x)))."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array([fma32(a[1], b[2], -(F(a[2]) * F(b[1]))), fma32(a[2], b[0], -(F(a[0]) * F(b[2]))),
                         fma32(a[0], b[1], -(F(a[1]) * F(b[0])))], np.float32)


def ray_at32(o, d, t):
    return np.array([fma32(t, d[0], o[0]), fma32(t, d[1], o[1]), fma32(t, d[2], o[2])], np.float32)


def uv_one(prim, o, d, t, cw, dw):
    """(u, v) of a hit of the record `prim` (PRIM_DTYPE) by ray (o, d) at t; cw, dw: the record's C.w and D.w as they lie on
    the device (patches only)."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    cat = int(prim["category"])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if cat == 2:
            v0, e1, e2 = prim["data1"], prim["data2"], prim["data3"]
            pvec = cross32(d, e2)
            inv = F(1.0) / dot32(e1, pvec)
            tvec = (o - v0).astype(np.float32)
            u = dot32(tvec, pvec) * inv
            v = dot32(d, cross32(tvec, e1)) * inv
            return F(u), F(v)
        if cat == 0:
            m = (ray_at32(o, d, F(t)) - prim["data1"]).astype(np.float32)
            return F(dot32(m, prim["data2"]) / F(dw)), F(dot32(m, prim["data3"]) / F(cw))
    return F(0.0), F(0.0)


def patch_denominators(prims):
    """(C.w, D.w) per primitive in array order as crt_prim.h prim_record computes them: dot(data3, data3) and
    dot(data2, data2) of a patch, 0 elsewhere (the test compares them with the device's before it uses either)."""
    cw, dw = np.zeros(len(prims), np.float32), np.zeros(len(prims), np.float32)
    for k in np.flatnonzero(prims["category"] == 0):
        cw[k], dw[k] = dot32(prims["data3"][k], prims["data3"][k]), dot32(prims["data2"][k], prims["data2"][k])
    return cw, dw


def device_denominators(accel, n):
    """(C.w, D.w) per primitive in array order from Renderer.debug_read_accel(): the PRIM part's float 11 and the PRIMD
    part's float 3 of the primitive's slot; D.w None where the part is not live (CRT_ACCEL_NONE keeps no PRIMD copy there)."""
    slot = accel["slot_of_index"][:n]
    cw = accel["prim"][slot, 11].astype(np.float32)
    dw = accel["primD"][slot, 3].astype(np.float32) if len(accel["primD"]) else None
    return cw, dw


# ------------------------------------------------------------------ the oracle's loop, every output
def oracle_full(orc, ps):
    """(o, d, exclude) -> (t* float32, i* uint32, position (n, 3), normal (n, 3)) of the oracle's loop: what
    traversal_cases.oracle_reference returns, from the same call, plus the hit's attributes (zeros at a miss)."""
    sc = orc.Scene.from_packed(ps)

    def ref(o, d, ex):
        n = len(o)
        t, idx = np.zeros(n, np.float32), np.full(n, MAXU, np.uint32)
        pos, nrm = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        for k in range(n):
            of, ou = sc.intersect(o[k], d[k], int(ex[k]))
            if ou[0]:
                t[k], idx[k], pos[k], nrm[k] = of[0], ou[1], of[1:4], of[4:7]
        return t, idx, pos, nrm
    return ref


# ------------------------------------------------------------------ the rays of a case
# Extra rays where the classes alone leave a case short of the conditions test_query_cpu.py asserts (a quarter of the
# rays hit, a tenth miss, without a limit): (aimed, miss_box) rays added per case.
EXTRA = {"tiny1": (200, 0)}          # one triangle: the four exclude classes and the in-plane rays cannot hit it


def class_mode(name):
    return "closest" if name.endswith("excl_closest") else "random" if name.endswith("excl_random") else "none"


class CaseRays:
    """The extension classes of traversal_cases.state_rays(case, N_PER_CLASS, SEED) with their exclude modes resolved
    against the oracle, extras appended, and the oracle's answer for every ray."""

    def __init__(self, case, orc, prims=None, seed=SEED):
        self.case = case
        self.ps = TC.packed(case, prims)
        self.prims = self.ps.primitives
        full = oracle_full(orc, self.ps)
        rng = np.random.default_rng(seed + 1)

        def ti(o, d, ex):
            return full(o, d, ex)[:2]
        o, d, ex, lab, self.names = [], [], [], [], []
        sets = [(c, co, cd) for c, co, cd, light in TC.state_rays(case, N_PER_CLASS, seed, prims) if light is None]
        aimed, missing = EXTRA.get(case.name, (0, 0))
        R = TC.Rays(case, prims, seed=seed + 2)
        if aimed:
            sets.append(("extra_aimed", *R.aimed(aimed, False)))
        if missing:
            sets.append(("extra_miss_box", *R.miss_box(missing)))
        for cname, co, cd in sets:
            o.append(co); d.append(cd); ex.append(TC.resolve_exclude(ti, rng, len(self.prims), co, cd, class_mode(cname)))
            lab.append(np.full(len(co), len(self.names))); self.names.append(cname)
        self.o, self.d, self.ex, self.lab = (np.concatenate(x) for x in (o, d, ex, lab))
        self.t, self.i, self.pos, self.nrm = full(self.o, self.d, self.ex)
        self.hit = self.i != MAXU
        self._uv = {}

    def uv(self, cw, dw):
        """(n, 2) float32, zeros at a miss; cached per (C.w, D.w) pair (every builder leaves the same values)."""
        key = (cw.tobytes(), dw.tobytes())
        if key not in self._uv:
            out = np.zeros((len(self.o), 2), np.float32)
            for k in np.flatnonzero(self.hit):
                i = int(self.i[k])
                out[k] = uv_one(self.prims[i], self.o[k], self.d[k], self.t[k], cw[i], dw[i])
            self._uv[key] = out
        return self._uv[key]


LIMITS = ("none", "at", "below", "above", "nan", "negative")


def limits(cr, kind):
    """t_max per ray of a CaseRays for a limit class: no limit; exactly t*; the float below it (a miss); the float above
    it; a NaN; a negative number.  A ray that misses without a limit takes a finite 1.0 in the three t* classes."""
    n = len(cr.o)
    base = np.where(cr.hit, cr.t, F(1.0)).astype(np.float32)
    if kind == "none":
        return np.full(n, NO_LIMIT, np.float32)
    if kind == "at":
        return base
    if kind == "below":
        return np.nextafter(base, F(0.0)).astype(np.float32)
    if kind == "above":
        return np.nextafter(base, F(np.inf)).astype(np.float32)
    if kind == "nan":
        return np.full(n, np.nan, np.float32)
    if kind == "negative":
        return np.full(n, -1.0, np.float32)
    raise ValueError(kind)


def expect(cr, t_max, uv, table=None):
    """The planes crt_query_rays must return for the rays of `cr` under the limits t_max (n,): a dict as
    Renderer.query_rays returns it.  uv: cr.uv(cw, dw); table: the id table (None: the identity)."""
    t_max = np.asarray(t_max, np.float32)
    with np.errstate(invalid="ignore"):
        hit = cr.hit & (cr.t <= t_max)                            # (a NaN limit compares false)
    n = len(hit)
    z4 = np.zeros((n, 4), np.float32)
    pos, nrm = z4.copy(), z4.copy()
    pos[hit, :3], nrm[hit, :3] = cr.pos[hit], cr.nrm[hit]
    prim = np.where(hit, cr.i, np.uint32(MAXU)).astype(np.uint32)
    ids = prim.copy()
    if table is not None:
        ids[hit] = np.asarray(table, np.uint32)[cr.i[hit]]
    return dict(hit=hit.astype(np.uint32), prim=prim, id=ids, t=np.where(hit, cr.t, t_max).astype(np.float32), position=pos, normal=nrm,
                uv=np.where(hit[:, None], uv, F(0.0)).astype(np.float32))


def differences(got, want):
    """{plane: indices of the rays whose bits differ} for the planes of `got`."""
    out = {}
    for p, a in got.items():
        shape = (len(a), int(np.prod(np.shape(a)[1:])))
        g, w = np.ascontiguousarray(a).view(np.uint32).reshape(shape), np.ascontiguousarray(want[p]).view(np.uint32).reshape(shape)
        bad = np.flatnonzero((g != w).any(1))
        if len(bad):
            out[p] = bad
    return out
