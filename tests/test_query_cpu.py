"""CPU-only tests of the ray queries (include/crt.h "Ray queries"): the three symbols are declared, exported
and bound, crt_ray is 32 bytes, a NULL context is refused, the command line takes --pick; the exact fma of
tests/query_ref.py rounds as worked out by hand; and the ray sets test_query_gpu.py uses are worth querying on the
reference alone -- in every case at least a quarter of the rays hit and a tenth miss without a limit, and the three limit
classes around t* do what they are there for."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import query_ref as Q
import traversal_cases as TC
from conftest import ROOT, bits
from traversal_cases import MAXU

SYMBOLS = ("crt_query_rays", "crt_query_rays_device", "crt_pick")
F = np.float32


def test_symbols_are_declared_exported_and_bound():
    from computeraytracer_amd import _lib
    from computeraytracer_amd import renderer as R
    text = open(os.path.join(ROOT, "include", "crt.h")).read()
    assert 0 < text.index("- ID mattes") < text.index("- Ray queries") < text.index("- Scene edits")
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/crt.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert re.search(r"enum\s*\{\s*CRT_QUERY_CLOSEST\s*=\s*0\s*,\s*CRT_QUERY_ANY\s*=\s*1\s*\}", header)
    assert (_lib.QUERY_CLOSEST, _lib.QUERY_ANY) == (0, 1) and R.QUERY_MODES == {"closest": 0, "any": 1}
    assert [f[0] for f in _lib.QueryPlanes._fields_] == list(R.QUERY_PLANES) == ["hit", "prim", "id", "t", "position", "normal", "uv"]
    assert C.sizeof(_lib.QueryPlanes) == 7 * C.sizeof(C.c_void_p)
    assert _lib.load().crt_abi_version() == 2
    # the statements the header owes its reader
    flat = " ".join(text[text.index("- Ray queries"):text.index("- Scene edits")].split())
    for phrase in ("never walked", "hipFree waits for the device", "must have finished its queries", "do NOT flush"):
        assert phrase in flat, phrase


def test_crt_ray_is_32_bytes(tmp_path):
    from computeraytracer_amd import _lib
    from computeraytracer_amd import renderer as R
    assert C.sizeof(_lib.Ray) == 32 and R.RAY_DTYPE.itemsize == 32
    assert [(n, R.RAY_DTYPE.fields[n][1]) for n in ("o", "t_max", "d", "exclude")] == [("o", 0), ("t_max", 12), ("d", 16), ("exclude", 28)]
    assert [(n, getattr(_lib.Ray, n).offset) for n in ("o", "t_max", "d", "exclude")] == [("o", 0), ("t_max", 12), ("d", 16), ("exclude", 28)]
    src = tmp_path / "ray.c"
    src.write_text('#include <stddef.h>\n#include "crt.h"\n'
                   '_Static_assert(sizeof(crt_ray) == 32, "size");\n'
                   '_Static_assert(offsetof(crt_ray, t_max) == 12 && offsetof(crt_ray, d) == 16 && offsetof(crt_ray, exclude) == 28, "layout");\n'
                   '_Static_assert(sizeof(crt_query_planes) == 7 * sizeof(void *), "planes");\n')
    out = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_pack_rays():
    from computeraytracer_amd import renderer as R
    r = R.pack_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [0, 1, 0]])
    raw = r.view(np.float32).reshape(2, 8)
    assert raw[0].tolist()[:3] == [1, 2, 3] and raw[1].tolist()[4:7] == [0, 1, 0]
    assert (bits(raw[:, 3]) == 0x4EFF0000).all() and (raw.view(np.uint32)[:, 7] == MAXU).all()      # 2139095040.0f, nothing excluded
    r = R.pack_rays(np.zeros((3, 3)), np.ones((3, 3)), t_max=[1.5, np.inf, np.nan], exclude=7)
    assert r["t_max"][0] == F(1.5) and np.isinf(r["t_max"][1]) and np.isnan(r["t_max"][2]) and (r["exclude"] == 7).all()
    with pytest.raises(ValueError):
        R.pack_rays(np.zeros((3, 3)), np.ones((2, 3)))
    assert float(Q.NO_LIMIT) == R.QUERY_NO_LIMIT


def test_null_context_and_unknown_arguments():
    from computeraytracer_amd import _lib
    from computeraytracer_amd import renderer as R
    lib = _lib.load()
    rays, hit = R.pack_rays([[0, 0, 0]], [[0, 0, 1]]), np.zeros(1, np.uint32)
    planes = _lib.QueryPlanes(hit=hit.ctypes.data)
    xy = np.zeros(2, np.uint32)
    assert lib.crt_query_rays(None, rays.ctypes.data, 1, 0, C.byref(planes)) == -1
    assert lib.crt_query_rays_device(None, rays.ctypes.data, 1, 0, C.byref(planes), None) == -1
    assert lib.crt_pick(None, xy.ctypes.data, 1, C.byref(planes)) == -1
    with pytest.raises(ValueError, match="unknown mode"):
        R.Renderer._query_planes("nearest", None)
    with pytest.raises(ValueError, match="unknown planes"):
        R.Renderer._query_planes("closest", ("hit", "depth"))
    assert R.Renderer._query_planes("any", None) == (1, ["hit"])
    assert R.Renderer._query_planes("closest", None) == (0, list(R.QUERY_PLANES))
    assert R.Renderer._query_planes(0, ("uv", "t")) == (0, ["t", "uv"])


def test_the_new_argument_parses():
    from computeraytracer_amd.__main__ import parse_args
    assert parse_args([]).pick is None
    assert parse_args(["--pick", "12,7", "--spp", "4"]).pick == (12, 7)
    assert parse_args(["--adaptive", "0.05", "--pick", "0,0"]).pick == (0, 0)
    for bad in (["--pick", "12"], ["--pick", "1,2,3"], ["--pick", "a,b"], ["--pick", "-1,4"], ["--pick", "1,2", "--orbit", "2"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2


# ------------------------------------------------------------------ the rounding, against hand-worked cases
def f(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def b(x):
    return int(np.float32(x).view(np.uint32))


def test_round_f32_hand_cases():
    e = Fraction(1, 2 ** 23)                                      # the spacing of binary32 in [1, 2)
    cases = [(Fraction(1), 0x3F800000), (Fraction(1) + e / 2, 0x3F800000),          # a tie: to the even neighbour, down
             (Fraction(1) + e + e / 2, 0x3F800002),                                # a tie: to the even neighbour, up
             (Fraction(1) + e / 2 + Fraction(1, 2 ** 60), 0x3F800001),             # just above a tie
             (Fraction(1) + e / 2 - Fraction(1, 2 ** 60), 0x3F800000),             # just below it
             (Fraction(1, 3), 0x3EAAAAAB), (Fraction(-1, 3), 0xBEAAAAAB), (Fraction(1, 10), 0x3DCCCCCD),
             (Fraction(2) - e / 4, 0x40000000),                                    # rounds up across a binade
             (Fraction(2 ** 24 + 1), 0x4B800000), (Fraction(2 ** 24 + 3), 0x4B800002),
             (Fraction(1, 2 ** 149), 0x00000001), (Fraction(1, 2 ** 150), 0x00000000),     # the smallest subnormal; half of it ties to even
             (Fraction(3, 2 ** 150), 0x00000002), (Fraction(1, 2 ** 126) - Fraction(1, 2 ** 150), 0x00800000),
             (Fraction(2 ** 128) - Fraction(2 ** 104), 0x7F7FFFFF),                # the largest finite
             (Fraction(2 ** 128) - Fraction(2 ** 103), 0x7F800000),                # half a step above it: to infinity
             (-Fraction(2 ** 128), 0xFF800000), (Fraction(0), 0x00000000)]
    for x, want in cases:
        assert b(Q.round_f32(x)) == want, (x, hex(want), hex(b(Q.round_f32(x))))


def test_fma32_hand_cases():
    a = f(0x3F800002)                                             # 1 + 2^-22
    # (1 + e)^2 - 1 = 2e + e^2 = 2^-21 (1 + 2^-23) exactly: representable; a product rounded first loses the e^2
    assert b(Q.fma32(a, a, F(-1.0))) == b(Q.round_f32(Fraction(1, 2 ** 21) + Fraction(1, 2 ** 44))) == 0x35000001
    assert b(F(a * a) - F(1.0)) == 0x35000000
    a = f(0x3F800001)                                             # 1 + 2^-23: 2^-22 (1 + 2^-24), a tie, to even
    assert b(Q.fma32(a, a, F(-1.0))) == 0x34800000
    # 3 * (1/3 rounded) - 1: the exact residual of the rounding
    third = f(0x3EAAAAAB)
    assert Q.fma32(F(3.0), third, F(-1.0)) == F(2.0 ** -25)
    # signs of an exact zero
    assert b(Q.fma32(F(2.0), F(3.0), F(-6.0))) == 0x00000000
    assert b(Q.fma32(F(-0.0), F(3.0), F(-0.0))) == 0x80000000
    assert b(Q.fma32(F(0.0), F(3.0), F(-0.0))) == 0x00000000
    # non-finite operands are IEEE's
    assert np.isinf(Q.fma32(F(np.inf), F(2.0), F(1.0))) and np.isnan(Q.fma32(F(np.inf), F(0.0), F(1.0))) and np.isnan(Q.fma32(F(1.0), F(1.0), F(np.nan)))
    # overflow in the sum alone
    big = f(0x7F7FFFFF)
    assert np.isinf(Q.fma32(big, F(2.0), F(0.0))) and Q.fma32(big, F(2.0), -big) == big
    # against binary64 where that is exact: small integers
    rng = np.random.default_rng(5)
    for x, y, z in rng.integers(-2000, 2000, (200, 3)):
        assert Q.fma32(F(x), F(y), F(z)) == F(float(x) * float(y) + float(z))
    # dot and cross are the chains of crt_math.h
    v, w = F([1, 2, 3]), F([4, 5, 6])
    assert Q.dot32(v, w) == F(32.0) and Q.cross32(v, w).tolist() == [-3.0, 6.0, -3.0]


def test_uv_on_exact_geometry():
    tri = TC.tris([[0, 0, 0]], [[8, 0, 0]], [[0, 8, 0]])[0]
    u, v = Q.uv_one(tri, F([2, 1, 5]), F([0, 0, -1]), F(5.0), F(0), F(0))
    assert (u, v) == (F(0.25), F(0.125))
    u, v = Q.uv_one(tri, F([0, 0, 5]), F([0, 0, -2]), F(2.5), F(0), F(0))     # a vertex; d not normalised
    assert b(u) in (0x0, 0x80000000) and b(v) in (0x0, 0x80000000)
    pat = TC.patches([[-2, -2, 8]], [[12, 0, 0]], [[0, 12, 0]])[0]
    cw, dw = Q.patch_denominators(np.array([pat]))
    assert (cw[0], dw[0]) == (F(144.0), F(144.0))
    u, v = Q.uv_one(pat, F([1, 4, 0]), F([0, 0, 1]), F(8.0), cw[0], dw[0])
    assert (u, v) == (F(0.25), F(0.5))
    sph = TC.spheres([[4, 4, -6]], [3])[0]
    assert [b(x) for x in Q.uv_one(sph, F([4, 4, 0]), F([0, 0, -1]), F(3.0), F(0), F(0))] == [0, 0]


# ------------------------------------------------------------------ the ray sets, on the reference alone
CASES = {c.name: c for c in TC.all_cases() + [TC.case_chain()]}
_RAYS = {}


def case_rays(name, orc):
    if name not in _RAYS:
        _RAYS.clear()
        _RAYS[name] = Q.CaseRays(CASES[name], orc)
    return _RAYS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_ray_sets_are_worth_querying(orc, name):
    cr = case_rays(name, orc)
    n, h = len(cr.o), int(cr.hit.sum())
    per = {c: (int((cr.lab == k).sum()), int(cr.hit[cr.lab == k].sum())) for k, c in enumerate(cr.names)}
    print(f"{name}: {n} rays, {h} hit; per class (rays, hits): {per}")
    assert np.isfinite(cr.o).all() and np.isfinite(cr.d).all()
    assert 4 * h >= n, f"{name}: {h} of {n} rays hit without a limit: fewer than a quarter"
    assert 10 * (n - h) >= n, f"{name}: {n - h} of {n} rays miss without a limit: fewer than a tenth"
    assert not np.isnan(cr.t[cr.hit]).any() and (cr.t[cr.hit] >= TC.T_MIN).all()
    # (t*, i*) are traversal_cases.oracle_reference's, from the same oracle call
    k = np.linspace(0, n - 1, 60).astype(int)
    t2, i2 = TC.oracle_reference(orc, cr.ps)(cr.o[k], cr.d[k], cr.ex[k])
    assert np.array_equal(i2, cr.i[k]) and np.array_equal(bits(t2), bits(cr.t[k]))
    # the exclude modes took effect: an excluded primitive is never the answer
    assert not (cr.hit & (cr.i == cr.ex)).any()
    assert (cr.ex != MAXU).sum() > N_EXCLUDED_MIN, (name, int((cr.ex != MAXU).sum()))
    # the limit classes: L = t* hits, the float below misses, the float above hits -- on every ray that hits at all
    uv = np.zeros((n, 2), np.float32)
    for kind, want in (("none", True), ("at", True), ("below", False), ("above", True), ("nan", False), ("negative", False)):
        L = Q.limits(cr, kind)
        e = Q.expect(cr, L, uv)
        assert (e["hit"][cr.hit] == (1 if want else 0)).all(), (name, kind)
        assert (e["hit"][~cr.hit] == 0).all(), (name, kind)
        miss = e["hit"] == 0
        assert np.array_equal(bits(e["t"][miss]), bits(L[miss])), (name, kind)           # a miss reports the ray's own t_max
        assert (e["prim"][miss] == MAXU).all() and not e["position"][miss].any() and not e["normal"][miss].any()
        assert np.array_equal(bits(e["t"][~miss]), bits(cr.t[~miss]))
    below = Q.limits(cr, "below")[cr.hit]
    assert (below < cr.t[cr.hit]).all() and (Q.limits(cr, "above")[cr.hit] > cr.t[cr.hit]).all()


N_EXCLUDED_MIN = Q.N_PER_CLASS                                      # the "random" class, and the hits of the three "closest" ones


def test_expect_carries_the_id_table(orc):
    cr = case_rays("tiny9", orc)
    table = (np.arange(len(cr.prims), dtype=np.uint32) * 7 + 100).astype(np.uint32)
    e = Q.expect(cr, Q.limits(cr, "none"), np.zeros((len(cr.o), 2), np.float32), table)
    assert (e["id"][cr.hit] == table[cr.i[cr.hit]]).all() and (e["id"][~cr.hit] == MAXU).all()
    assert (e["prim"][cr.hit] == cr.i[cr.hit]).all()
