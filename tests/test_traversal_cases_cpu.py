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
  * no NaN t comes out of the oracle for any ray.

And the reference side of the fallback floors of test_single_ray_walks_gpu.py: the first descent of traverse4q
(crt_shade.h) restated on the restated LBVH, its collapse and its quantised boxes -- on the chain case it needs more
than the kStackDepth entries of the single-ray stack for (nearly) every ray from inside the boxes, on the deep case for
none."""
import numpy as np
import pytest

import accel_ref as AR
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


# ------------------------------------------------------------------ the first descent of traverse4q, restated
K_STACK = 64                       # crt_device.h kStackDepth: entries per lane of the single-ray walks' stack
T_INIT = np.float32(2139095040.0)  # crt_shade.h CRT_INFINITY: an extension ray's initial t_max
NO_BOX = np.float32(3.0e38)


def wide_tree_4q(case):
    """The quantised 4-wide tree of the case's restated LBVH: (qlo, qhi (nw, 4, 3) uint16 -- an empty slot is the
    inverted box --, child (nw, 4) int: a wide node, or -1 for a leaf / an empty slot), base, scale, depth)."""
    pad = TC.hit_pad(case.prims, case.eye)
    lo, hi, unb = AR.prim_bounds(case.prims, pad)
    assert not unb.any()
    base, scale = AR.grid(lo, hi)
    _, refs, _, boxes = AR.lbvh(case.prims, pad)
    levels, depth = AR.collapse(refs, boxes, 0, 4)
    wid = {b: k for k, b in enumerate(b for level in levels for b, _, _ in level)}
    qlo = np.full((len(wid), 4, 3), AR.Q_EMPTY[0], np.uint16)
    qhi = np.full((len(wid), 4, 3), AR.Q_EMPTY[1], np.uint16)
    child = np.full((len(wid), 4), -1, np.int64)
    for level in levels:
        for b, rs, bx in level:
            for i, (r, box) in enumerate(zip(rs, bx)):
                qlo[wid[b], i], qhi[wid[b], i] = AR.quantize(box[0], box[1], base, scale)
                child[wid[b], i] = wid[r] if r >= 0 else -1
    return qlo, qhi, child, base, scale, depth


def first_descent_need(tree, o, d, t_max):
    """Stack entries traverse4q holds when its first descent ends (at a leaf, or where no child box is hit), per ray:
    at every node the boxes hit but the nearest are pushed.  The kernel's arithmetic: planes base + q * scale folded
    into one fma per plane, the 1.0000005 slab test, the five strict-< compare-exchanges in its order."""
    qlo, qhi, child, base, scale, _ = tree
    f = np.float32
    o, d = np.asarray(o, f), np.asarray(d, f)
    tiny = f(1.0e-20)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        idv = (f(1.0) / np.where(np.abs(d) > tiny, d, np.copysign(tiny, d))).astype(f)
        neg = idv < 0
        oid = AR.fma32(np.broadcast_to(base, o.shape), idv, -(o * idv).astype(f))
        idq = (scale[None, :] * idv).astype(f)
    n = len(o)
    t_max = np.broadcast_to(np.asarray(t_max, f), (n,))
    node = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    sp = np.zeros(n, np.int64)
    while live.any():
        a = np.flatnonzero(live)
        lo, hi = qlo[node[a]].astype(f), qhi[node[a]].astype(f)          # (m, 4, 3)
        g = neg[a][:, None, :]
        with np.errstate(over="ignore", invalid="ignore"):
            tn3 = AR.fma32(np.where(g, hi, lo), np.broadcast_to(idq[a][:, None, :], lo.shape), np.broadcast_to(oid[a][:, None, :], lo.shape))
            tf3 = AR.fma32(np.where(g, lo, hi), np.broadcast_to(idq[a][:, None, :], lo.shape), np.broadcast_to(oid[a][:, None, :], lo.shape))
            tn = np.fmax(np.fmax(tn3[..., 0], tn3[..., 1]), np.fmax(tn3[..., 2], T_MIN_F))
            tf = np.fmin(np.fmin(tf3[..., 0], tf3[..., 1]), np.fmin(tf3[..., 2], t_max[a][:, None]))
            k = np.where(tn <= (tf * f(1.0000005)).astype(f), tn, NO_BOX).astype(f)
        r = child[node[a]].copy()
        for i, j in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):           # CRT_CAS1, in traverse4q's order: swap on kb < ka only
            sw = k[:, j] < k[:, i]
            k[:, i], k[:, j] = np.where(sw, k[:, j], k[:, i]), np.where(sw, k[:, i], k[:, j])
            r[:, i], r[:, j] = np.where(sw, r[:, j], r[:, i]), np.where(sw, r[:, i], r[:, j])
        hit = k < NO_BOX
        sp[a] += np.where(hit[:, 0], hit[:, 1:].sum(1), 0)
        go = hit[:, 0] & (r[:, 0] >= 0)                                   # the nearest is an inner node: one level down
        node[a] = np.where(go, r[:, 0], 0)
        live[a] = go
    return sp


T_MIN_F = np.float32(0.001)


def chain_floor_counts(orc, case, n, seed):
    """{class: (rays, rays whose first descent needs more than K_STACK entries)} for the rays of State(case, seed, n)."""
    tree = wide_tree_4q(case)
    out = {}
    for cname, o, d, L in TC.state_rays(case, n, seed):
        t_max = T_INIT
        if L is not None:                                         # a shadow ray walks with the light's own t
            t_max, i_l = TC.oracle_reference(orc, TC.single(case, L))(o, d, np.full(len(o), MAXU, np.uint32))
            assert (i_l == 0).all(), (case.name, cname)
        out[cname] = (len(o), int((first_descent_need(tree, o, d, t_max) > K_STACK).sum()))
    return out, tree[5]


def test_the_chain_case_overflows_the_single_ray_stack_and_the_deep_case_does_not(orc):
    """The floors test_single_ray_walks_gpu.py sets for the fallback of traverse4q are conditions on the kernel; here
    the reference alone meets them, twice over: with that test's rays (WALK_N per class, seed WALK_SEED) the first
    descent on the chain case passes kStackDepth for every ray of near_tmin, inside and deep_centre and for half of the
    plain shadow rays at the least; on the deep case (15 levels, 45 entries at most) for no ray at all."""
    chain = TC.case_chain()
    got, depth = chain_floor_counts(orc, chain, TC.WALK_N, TC.WALK_SEED)
    print("chain_lbvh first descent > 64 entries:", got)
    assert depth == 30 + TC.CHAIN_J and 3 * depth > K_STACK
    for cname in ("near_tmin", "inside", "deep_centre"):
        assert got[cname] == (TC.WALK_N, TC.WALK_N), (cname, got[cname])                    # 2 x "at least half"
    sh = got[f"shadow[light {chain.lights[0]}]"]
    assert sh[0] == TC.WALK_N and 2 * sh[1] >= sh[0], sh                                    # 2 x "at least a quarter"
    got, depth = chain_floor_counts(orc, CASES["deep_lbvh"], 2000, 10)                      # the rays of the shared fresh State
    print("deep_lbvh first descent > 64 entries:", got)
    assert 3 * depth <= K_STACK
    assert all(over == 0 for _, over in got.values()), got
