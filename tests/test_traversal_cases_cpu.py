"""CPU-only: the scenes and rays of traversal_cases.py judged by the oracle, so that the GPU parity test
(test_traversal_rays_gpu.py) cannot pass on rays that test nothing.  Per case and ray class, from the oracle alone:

  * aimed classes (aimed, aimed_jitter, axis) of every case: at least half of the rays hit the case's geometry, at
    least a tenth miss (the scenes stand in free space: there is no backdrop, a hit is a hit on the case).
  * coincident cases: every hit is won by the highest index of the duplicates (100 %), and with the winner excluded
    by the second highest.
  * grid case: the in-plane rays hit no triangle of the plane and do hit what lies behind (the box's walls).
  * shadow classes: every ray hits its own light (it is a shadow ray the shade kernel would emit); of the plain
    shadow class of each light between 20 % and 80 % are visible -- in every case but tiny1, whose only primitive is
    the light.  (The flat cases hold a coplanar triangle over the light; where every primitive is a copy of the light,
    the ray excludes the one later copy on every second ray, as a ray leaving that surface would.)  At least 100 rays
    per exact-tie sub-class, all of them decided by the index order.
  * no NaN t comes out of the oracle for any ray."""
import numpy as np
import pytest

import traversal_cases as TC
from traversal_cases import MAXU

N = 600            # rays per class here (the GPU test uses more of the same generators)


def _cases():
    return TC.all_cases()


CASES = {c.name: c for c in _cases()}


def test_cases_are_what_they_claim():
    q = {n: TC.quantisable(c.prims, c.eye) for n, c in CASES.items()}
    assert q["grid"] and q["flat_y0"] and q["degenerate"] and q["deep_lbvh"] and q["baseline"]
    # flat and far from the origin on the flat axis, non-finite corners: 32-byte boxes
    assert not q["flat_y100"] and not q["flat_y5000"]
    assert not q["unbounded_nan_vertex"] and not q["unbounded_inf_vertex"]
    assert q["grid_inside_16ext"] and not q["grid_outside_16ext"]
    assert np.isinf(TC.hit_pad(CASES["unbounded_inf_vertex"].prims, CASES["unbounded_inf_vertex"].eye))
    assert np.isfinite(TC.hit_pad(CASES["unbounded_nan_vertex"].prims, CASES["unbounded_nan_vertex"].eye))
    for c in CASES.values():
        assert np.array_equal(c.prims["data4"][:, 3], np.arange(len(c.prims)))
        lo, hi = TC.finite_bounds(c.prims)
        assert (np.abs(c.eye) >= np.maximum(np.abs(lo), np.abs(hi)).max()).all() or c.ps is not None
    g = CASES["grid"].prims                                     # exact floats: multiples of 4 well inside the 24-bit mantissa
    assert np.array_equal(g["data1"], np.round(g["data1"] / 4) * 4)


def test_the_pad_is_the_oracles(orc):
    for c in CASES.values():
        assert TC.hit_pad(c.prims, c.eye) == np.float32(orc.Scene.from_packed(TC.packed(c)).hit_pad()), c.name


def test_deep_case_is_a_chain():
    """The Morton codes of the deep case as crt_lbvh.hip computes them: one code bit per chain cell."""
    c = CASES["deep_lbvh"]
    cn = TC.corners(c.prims)
    ctr = 0.5 * cn.min(1) + 0.5 * cn.max(1)
    lo, hi = ctr.min(0), ctr.max(0)
    q = np.clip(((ctr - lo) * (1024.0 / (hi - lo))).astype(np.int64), 0, 1023)

    def expand(v):
        out = np.zeros_like(v)
        for b in range(10):
            out |= ((v >> b) & 1) << (3 * b)
        return out
    m = (expand(q[:, 0]) << 2) | (expand(q[:, 1]) << 1) | expand(q[:, 2])
    codes = set(int(v) for v in m)
    assert {1 << k for k in range(30)} <= codes and 0 in codes and (1 << 30) - 1 in codes and len(codes) == 32
    zero = np.flatnonzero(m == 0)
    assert all(int(i) & (int(i) - 1) == 0 for i in zero) and len(zero) >= 12
    assert all((m == (1 << k)).sum() == 3 for k in range(30))


@pytest.mark.parametrize("name", list(CASES))
def test_ray_classes_against_the_oracle(orc, name):
    case = CASES[name]
    ps = TC.packed(case)
    ref = TC.oracle_reference(orc, ps)
    R = TC.Rays(case, seed=1)
    rng = np.random.default_rng(2)
    n = N if len(case.prims) < 5000 else 250
    rows = []
    for cname, o, d, mode in R.classes(n):
        assert np.isfinite(o).all() and np.isfinite(d).all()
        assert (np.abs(o) <= R.M).all(), "origins stay inside the region hit_pad is scaled for"
        ex = TC.resolve_exclude(ref, rng, len(case.prims), o, d, mode)
        t, i = ref(o, d, ex)
        assert not np.isnan(t).any(), (name, cname)
        hit = i != MAXU
        rows.append(f"{cname}: hit {hit.mean():.2f}")
        if cname in ("aimed", "aimed_jitter", "axis"):
            assert hit.mean() >= 0.5 and (~hit).mean() >= 0.1, (name, cname, hit.mean())
        if cname == "miss_box":
            assert not hit.any()
        if case.group is not None:
            grp = case.group
            top = np.array([np.flatnonzero(grp == g).max() for g in range(grp.max() + 1)])
            if mode == "none":
                assert (i[hit] == top[grp[i[hit]]]).all(), (name, cname)
                assert hit.sum() >= n // 4 or not cname.startswith("aimed"), (name, cname)
            if mode == "closest":                               # the winner excluded: the runner-up at the same t -- the next copy of
                t0, i0 = ref(o, d, np.full(len(o), MAXU, np.uint32))     # that geometry, or (on a shared edge) the top copy of a neighbour
                both = (i0 != MAXU)
                second = np.array([np.sort(np.flatnonzero(grp == g))[-2] for g in range(grp.max() + 1)])
                same = grp[i[both]] == grp[i0[both]]
                assert (i[both] == np.where(same, second[grp[i0[both]]], top[grp[i[both]]])).all(), (name, cname)
                assert (t[both].view(np.uint32) == t0[both].view(np.uint32)).all(), (name, cname)
        if cname == "box_plane":                               # the origin sits exactly in the builders' box plane, in float32
            assert len(o) == n
        if cname == "in_plane" and name == "grid":
            assert not (i[hit] < 512).any(), "an edge-on triangle is never hit"
            assert hit.mean() > 0.05, "the box's walls behind"
        if cname == "in_plane" and case.flat:
            assert not hit.any()
    # shadow rays
    vis_all, lines = [], []
    for L in case.lights:
        o, d = R.shadow(L, n)
        ex = TC.shadow_excludes(case, L, n, len(case.prims), rng)
        t_l, own, vis, hi_, lo_ = TC.shadow_expect(ref, TC.oracle_reference(orc, TC.single(case, L)), L, o, d, ex)
        assert own.all(), (name, L, int((~own).sum()))
        assert not np.isnan(t_l).any()
        lines.append(f"shadow L={L}: visible {vis.mean():.2f}")
        if len(case.prims) > 1:
            assert 0.2 <= vis.mean() <= 0.8, (name, L, vis.mean())
        vis_all.append(vis)
    for L, kind in case.tie_lights:
        od = R.shadow_tie(L, 400)
        o, d = od if od is not None else R.shadow(L, 400)
        ex = np.full(len(o), MAXU, np.uint32)
        t_l, own, vis, hi_, lo_ = TC.shadow_expect(ref, TC.oracle_reference(orc, TC.single(case, L)), L, o, d, ex)
        assert own.all(), (name, L)
        tie = hi_ if kind == "higher" else lo_
        lines.append(f"tie {kind} L={L}: {int(tie.sum())} ties, visible {vis.mean():.2f}")
        assert tie.sum() >= 100, (name, L, kind, int(tie.sum()))
        assert (vis[tie] == (kind == "lower")).all()
        vis_all.append(vis)
    v = np.concatenate(vis_all)
    print(name, "; ".join(rows), f"; shadow visible {v.mean():.2f}", "; ".join(lines))
