"""CPU-only: the scenes of material_matrix_scenes.py do what they claim, measured on the oracle -- which (category,
material) pairs their paths reach and how often, that the images are finite and lit (NaN exactly where a sphere light
of area 0 contributes), and what lights_of packs for a light that is no patch.  These conditions keep
test_material_matrix_gpu.py from passing on scenes that never run the paths it is written for."""
import numpy as np
import pytest

import material_matrix_scenes as MM
from computeraytracer_amd import scene as S

W = H = 96
SPP = 4
FLOOR = 100                                     # path vertices per required pair and scene
MISS = 0xFFFFFFFF

# (category, material) pairs each scene has to reach: 0 patch, 1 sphere, 2 triangle x 0 diffuse, 1 light, 2 glass
REQUIRED = {"tri": [(0, 2), (2, 2), (2, 1), (2, 0)],
            "sphere": [(1, 1), (0, 2), (2, 2)],
            "patch": [(0, 1), (0, 2), (2, 2)],
            "tri_only": [(2, 0), (2, 1), (2, 2)],
            "sphere_only": [(1, 0), (1, 1), (1, 2)]}

_CACHE = {}


def measured(orc, name):
    """Pair counts over every pixel and samples 1..4, and the 4-sample oracle frame, once per scene."""
    if name not in _CACHE:
        ps = MM.build(name, W, H)
        sc = orc.Scene.from_packed(ps)
        cat, mat = ps.primitives["category"], ps.primitives["data4"][:, 2]
        hits = []
        for y in range(H):
            for x in range(W):
                for s in range(1, SPP + 1):
                    t = sc.trace_pixel(x, y, s)
                    hits.append(np.asarray(t.hits[:t.n_hits], np.uint32))
        hits = np.concatenate(hits)
        hits = hits[hits != MISS]
        pair, count = np.unique(np.stack([cat[hits], mat[hits]], 1), axis=0, return_counts=True)
        pairs = {(int(c), int(m)): int(k) for (c, m), k in zip(pair, count)}
        acc, _, cnt = sc.render(SPP)
        a = acc[..., :3]
        nan, inf, zero = np.isnan(a).any(-1), np.isinf(a).any(-1), (a == 0).all(-1)
        shares = dict(nan=float(nan.mean()), inf=float(inf.mean()), zero=float(zero.mean()),
                      lit=float((np.isfinite(a).all(-1) & ~zero).mean()), shadow=int(cnt[4]))
        print(f"{name}: pairs {dict(sorted(pairs.items()))} shares {shares}")        # (pytest -s shows it, once per scene)
        _CACHE[name] = (ps, pairs, shares)
    return _CACHE[name]


@pytest.mark.parametrize("name", MM.NAMES)
def test_pair_coverage(orc, name):
    _, pairs, _ = measured(orc, name)
    for p in REQUIRED[name]:
        assert pairs.get(p, 0) >= FLOOR, (name, p, pairs)


def test_the_scenes_together_reach_every_missing_pair(orc):
    reached = set()
    for name in ("tri", "sphere", "tri_only"):
        reached |= {p for p, k in measured(orc, name)[1].items() if k >= FLOOR}
    assert {(0, 2), (2, 2), (2, 1), (1, 1)} <= reached
    assert set(measured(orc, "tri_only")[1]) == {(2, 0), (2, 1), (2, 2)}          # nothing but triangles is ever hit
    assert set(measured(orc, "sphere_only")[1]) == {(1, 0), (1, 1), (1, 2)}


@pytest.mark.parametrize("name", ["tri", "sphere", "patch", "tri_only"])
def test_finite_and_lit(orc, name):
    _, _, sh = measured(orc, name)
    assert sh["nan"] == 0.0 and sh["inf"] == 0.0, sh
    assert sh["zero"] < 0.25 and sh["shadow"] > 0, sh


def test_sphere_only_is_nan_where_the_light_contributes(orc):
    _, _, sh = measured(orc, "sphere_only")
    assert 0.10 <= sh["nan"] <= 0.90, sh
    assert sh["lit"] >= 0.05 and sh["shadow"] > 0, sh


def test_scene_shapes():
    for name in ("tri", "sphere", "patch"):
        ps = MM.build(name, W, H)
        cat, mat = ps.primitives["category"], ps.primitives["data4"][:, 2]
        assert np.array_equal(ps.primitives["data4"][:, 3], np.arange(len(ps.primitives)))
        assert ((cat == 0) & (mat == 2)).sum() == 6 and ((cat == 2) & (mat == 2)).sum() == 12 and ((cat == 2) & (mat == 0)).sum() == 2
        assert (ps.width, ps.height) == (W, H)
    t, s = MM.build("tri_only", W, H), MM.build("sphere_only", W, H)
    assert (t.primitives["category"] == 2).all() and len(t.primitives) == 10 + 12 + 1 and len(t.lights) == 1
    assert (s.primitives["category"] == 1).all() and len(s.primitives) == 4 and len(s.lights) == 1
    assert [len(MM.build(n, W, H).lights) for n in ("tri", "sphere", "patch")] == [2, 2, 1]
    # the triangle walls cover the patch walls: same reflectance, each parallelogram's two halves
    c = S.cornell(W, H)
    for k, w in enumerate(c.primitives[MM.WALLS]):
        a, b = t.primitives[2 * k], t.primitives[2 * k + 1]
        assert a["data4"][1] == b["data4"][1] == w["data4"][1]
        assert np.array_equal(a["data1"], w["data1"]) and np.array_equal(b["data1"], w["data1"] + w["data2"] + w["data3"])
        assert np.array_equal(b["data2"], -w["data2"]) and np.array_equal(b["data3"], -w["data3"])


def test_non_patch_light_records():
    """lights_of writes category 0 and leaves data1..3 as they are: a triangle light keeps v0, e1, e2 (sampled as the
    parallelogram v0 + u e1 + v e2), a sphere light keeps (centre, r r r, 0 0 0) (sampled on a segment, area 0)."""
    ps = MM.build("tri", W, H)
    src = ps.primitives[ps.primitives["data4"][:, 2] == 1]
    assert (src["category"] == 2).all() and (ps.lights["category"] == 0).all()
    for f in ("data1", "data2", "data3", "data4"):
        assert np.array_equal(ps.lights[f], src[f])
    words = ps.lights.view(np.uint8).reshape(2, 80).view("<u4")
    f = lambda v: int(np.float32(v).view(np.uint32))
    assert words.tolist() == [
        [0, 0, 0, 0, f(213), f(554), f(227), 0, f(130), 0, 0, 0, 0, 0, f(105), 0, 3, 0, 1, 25],
        [0, 0, 0, 0, f(343), f(554), f(332), 0, f(-130), 0, 0, 0, 0, 0, f(-105), 0, 5, 0, 1, 26]]
    assert [f(213), f(554), f(227), f(130), f(105), f(-130)] == [0x43550000, 0x440A8000, 0x43630000, 0x43020000, 0x42D20000, 0xC3020000]
    for name, at in (("sphere", 0), ("sphere_only", 0)):
        ps = MM.build(name, W, H)
        src = ps.primitives[ps.primitives["data4"][:, 2] == 1][at]
        L = ps.lights[at]
        assert src["category"] == 1 and L["category"] == 0
        assert np.array_equal(L["data1"], src["data1"]) and np.array_equal(L["data2"], src["data2"])
        assert not L["data3"].any() and L["data2"][0] == L["data2"][1] == L["data2"][2] > 0
    ps = MM.build("sphere", W, H)
    assert ps.lights["data4"][:, 3].tolist() == [25, 26] and ps.primitives["category"][[25, 26]].tolist() == [1, 0]
    assert ps.lights["data4"][0, 0] >= len(ps.lights) - 1     # lights[emission index] clamps to the LAST light: the patch
