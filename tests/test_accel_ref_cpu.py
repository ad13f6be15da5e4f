"""CPU-only: accel_ref.py, the restatement the structural GPU tests (test_accel_structure_gpu.py) hold the trees to, is
itself held to the reference loop and to hand-worked examples.

  * prim_bounds against the oracle: for every case of traversal_cases.py and every ray class, the point o + t d
    (float64) of every oracle hit (t, index) lies inside the restated box of that primitive.  No tolerance: the box
    carries 2 hit_pad, the margin the rule claims.  Primitives the restatement marks unbounded are exempt (their box
    is +-3e38), and they are fewer than 1 % of any case that is not about them.
  * hierarchy, box unions, collapse, grid and quantiser on inputs small enough to work out by hand; the expected
    values are written here.
  * properties of the restated LBVH of every case: every primitive in exactly one leaf, n - 1 inner nodes, at most 62
    levels.
  * the chain case (case_chain): its restated 4-wide tree is as deep as the test of the larger stack overflow area
    needs, and an 8-wide tree deep enough for the SAH fallback is out of any test's reach."""
import numpy as np
import pytest

import accel_ref as AR
import traversal_cases as TC
from traversal_cases import MAXU

F = np.float32
N = 300
CASES = {c.name: c for c in TC.all_cases()}
ABOUT_UNBOUNDED = {c.name for c in TC.cases_unbounded() + TC.cases_degenerate()}
L = AR.leaf_ref                                               # L(slot): the reference of a one-primitive leaf


def test_leaf_references():
    assert [L(0), L(1), L(2), L(4), L(0, 4), L(5, 2)] == [-1, -9, -17, -33, -4, -42]
    f, c = AR.leaf_range(np.array([-1, -9, -4, -42]))
    assert f.tolist() == [0, 1, 0, 5] and c.tolist() == [1, 1, 4, 2]


# ------------------------------------------------------------------ prim_bounds == what the loop accepts
@pytest.mark.parametrize("name", list(CASES))
def test_every_oracle_hit_lies_inside_the_restated_box(orc, name):
    case = CASES[name]
    ref = TC.oracle_reference(orc, TC.packed(case))
    pad = TC.hit_pad(case.prims, case.eye)
    assert pad == F(orc.Scene.from_packed(TC.packed(case)).hit_pad())
    lo, hi, unb = AR.prim_bounds(case.prims, pad)
    assert not np.isnan(lo).any() and not np.isnan(hi).any()
    if name not in ABOUT_UNBOUNDED:
        assert unb.mean() < 0.01, (name, int(unb.sum()))
    R = TC.Rays(case, seed=3)
    rng = np.random.default_rng(4)
    n = N if len(case.prims) < 5000 else 120
    hits = 0
    for cname, o, d, mode in R.classes(n):
        ex = TC.resolve_exclude(ref, rng, len(case.prims), o, d, mode)
        t, i = ref(o, d, ex)
        hit = (i != MAXU) & ~unb[np.minimum(i, len(unb) - 1)]
        p = o[hit].astype(np.float64) + t[hit].astype(np.float64)[:, None] * d[hit].astype(np.float64)
        k = i[hit]
        inside = ((p >= lo[k].astype(np.float64)) & (p <= hi[k].astype(np.float64))).all(1)
        if not inside.all():
            b = int(np.flatnonzero(~inside)[0])
            pytest.fail(f"{name} / {cname}: {int((~inside).sum())} of {len(k)} hit points lie outside their primitive's box; first: primitive "
                        f"{int(k[b])} point {p[b].tolist()} box {lo[k[b]].tolist()} .. {hi[k[b]].tolist()} (hit_pad {pad!r})")
        hits += int(hit.sum())
    assert hits >= n or len(case.prims) == 1, (name, hits)


def test_prim_bounds_by_hand():
    """hit_pad 0.25 (S = 32768): g = 0.5 for triangles and patches; a sphere of radius r adds min(S^2 2^-20 / r, S)."""
    p = TC.join(TC.tris([[1, 2, 3]], [[5, 2, 3]], [[1, 8, 4]]),
                TC.spheres([[10, 20, 30]], [4]),                                   # radial: 32768^2 2^-20 / 4 = 256
                TC.spheres([[0, 0, 0]], [0.0]),                                    # r = 0: the radial term is S
                TC.patches([[0, 0, 0]], [[4, 0, 0]], [[0, 0, 2]]),                 # e1 perpendicular to e2: the corner box
                TC.patches([[0, 0, 0]], [[4, 0, 0]], [[4, 4, 0]]),                 # sheared: the accepted region is wider
                TC.patches([[0, 0, 0]], [[4, 0, 0]], [[8, 0, 0]]),                 # edges parallel: unbounded
                TC.tris([[np.nan, 0, 0]], [[1, 0, 0]], [[0, 1, 0]]),               # NaN in the first corner: x unbounded
                TC.tris([[0, 0, 0]], [[np.inf, 1, 0]], [[0, 1, 1]]))
    lo, hi, unb = AR.prim_bounds(p, F(0.25))
    assert unb.tolist() == [False, False, False, False, False, True, True, True]
    assert lo[0].tolist() == [0.5, 1.5, 2.5] and hi[0].tolist() == [5.5, 8.5, 4.5]
    assert lo[1].tolist() == [10 - 4 - 256.5, 20 - 4 - 256.5, 30 - 4 - 256.5] and hi[1].tolist() == [10 + 4 + 256.5, 20 + 4 + 256.5, 30 + 4 + 256.5]
    assert lo[2].tolist() == [-32768.5] * 3 and hi[2].tolist() == [32768.5] * 3
    # the four points of the region coincide with the corners; nextafter widens each plane by one ulp before the -+ g
    up, dn = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))
    assert lo[3].tolist() == [dn(0) - F(0.5), dn(0) - F(0.5), dn(0) - F(0.5)] and hi[3].tolist() == [up(4) + F(0.5), up(0) + F(0.5), up(2) + F(0.5)]
    # e1 = (4,0,0), e2 = (4,4,0): g11 = 16, g22 = 32, g12 = 16, det = 256.  The region's points: m.e1 = a, m.e2 = b for
    # (a, b) in {0, 16} x {0, 32}: (0,0) -> 0; (16,0) -> al = 2, be = -1: (4,-4,0); (0,32) -> al = -2, be = 2: (0,8,0);
    # (16,32) -> al = 0, be = 1: (4,4,0).  With the corners (0,0) (4,0) (4,4) (8,4): x in [0, 8], y in [-4, 8]
    assert lo[4].tolist() == [dn(0) - F(0.5), dn(-4) - F(0.5), dn(0) - F(0.5)] and hi[4].tolist() == [8.5, up(8) + F(0.5), up(0) + F(0.5)]
    assert (lo[5] == -AR.BIG).all() and (hi[5] == AR.BIG).all()
    assert lo[6].tolist() == [-AR.BIG, -0.5, -0.5] and hi[6].tolist() == [AR.BIG, 1.5, 0.5]
    assert lo[7].tolist() == [-AR.BIG, -0.5, -0.5] and hi[7].tolist() == [AR.BIG, 1.5, 1.5]


# ------------------------------------------------------------------ hierarchy
HIER = {
    # keys -> child references of nodes 0 .. n-2 (node g / g + 1 for a split after position g; the root is node 0)
    "2": ([5, 9], [[L(0), L(1)]]),
    "3": ([0b001, 0b010, 0b100], [[1, L(2)], [L(0), L(1)]]),
    "4": ([0, 1, 2, 3], [[1, 2], [L(0), L(1)], [L(2), L(3)]]),
    "5": ([0, 1, 2, 3, 4], [[3, L(4)], [L(0), L(1)], [L(2), L(3)], [1, 2]]),
    "5 chain": ([0, 1, 2, 4, 8], [[3, L(4)], [L(0), L(1)], [1, L(2)], [2, L(3)]]),
    "8": (list(range(8)), [[3, 4], [L(0), L(1)], [L(2), L(3)], [1, 2], [5, 6], [L(4), L(5)], [L(6), L(7)]]),
    "9": (list(range(9)), [[7, L(8)], [L(0), L(1)], [L(2), L(3)], [1, 2], [5, 6], [L(4), L(5)], [L(6), L(7)], [3, 4]]),
    "high bits": ([(1 << 32) | 7, 1 << 61, (1 << 61) | 1], [[L(0), 1], [L(1), L(2)]]),
}
DEPTH = {"2": 1, "3": 2, "4": 2, "5": 3, "5 chain": 4, "8": 3, "9": 4, "high bits": 2}


@pytest.mark.parametrize("name", list(HIER))
def test_hierarchy_by_hand(name):
    keys, want = HIER[name]
    refs = AR.hierarchy(np.array(keys, np.uint64))
    assert refs.tolist() == want
    t = AR.Tree2(refs, 0, len(keys), max_leaf=1)
    assert t.n2 == len(keys) - 1 and t.depth == DEPTH[name]
    assert sorted(AR.leaf_range(t.leaves)[0].tolist()) == list(range(len(keys)))


def test_morton_keys_by_hand():
    # equal centres: every code is 0 and the key is the index -- the chain on the index bits
    lo = np.array([[0, 0, 0], [-1, -1, -1], [-2, -3, -4]], np.float32)
    assert AR.morton_keys(lo, -lo).tolist() == [0, 1, 2]
    # centres x = 0, 1, 0.5 (y, z equal): cells 0, 1023 (1024 clamped), 512; x takes bit 2 of every triplet
    lo = np.array([[-1, 0, 0], [0, 0, 0], [-0.5, 0, 0]], np.float32)
    hi = np.array([[1, 2, 2], [2, 2, 2], [1.5, 2, 2]], np.float32)
    assert AR.morton_keys(lo, hi).tolist() == [0, (0x24924924 << 32) | 1, (1 << 61) | 2]
    # z takes bit 0, y bit 1; a centre outside +-1e30 does not widen the box of the centres and lands in a clamped cell
    lo = np.array([[0, 0, 0], [0, 2, 4], [-3e38, -3e38, -3e38]], np.float32)
    hi = np.array([[0, 0, 0], [0, 2, 4], [-3e38, -3e38, -3e38]], np.float32)
    assert AR.morton_keys(lo, hi).tolist() == [0, (0x12492492 | 0x09249249) << 32 | 1, 2]


def test_tree_checks_notice_a_broken_topology():
    good = [[1, 2], [L(0), L(1)], [L(2), L(3)]]
    AR.Tree2(good, 0, 4, max_leaf=1)
    for bad, msg in (([[1, 1], [L(0), L(1)], [L(2), L(3)]], "twice"), ([[1, 3], [L(0), L(1)], [L(2), L(3)]], "past the node array"),
                     ([[1, L(3)], [L(0), L(1)], [L(2), L(3)]], "not reached"), ([[1, 2], [L(0), L(1)], [L(1), L(3)]], "no leaf or in two"),
                     ([[1, 2], [L(0), L(2)], [L(1), L(3)]], "contiguous"), ([[1, 2], [L(0), L(1)], [L(2, 2), L(4)]], "leaf counts")):
        with pytest.raises(AssertionError, match=msg):
            AR.Tree2(bad, 0, 5 if msg == "leaf counts" else 4, max_leaf=1)


# ------------------------------------------------------------------ unions and collapse
def _cubes(xs):
    lo = np.array([[x, 0, 0] for x in xs], np.float32)
    return lo, (lo + F(1)).astype(np.float32)


def test_boxes_and_collapse_by_hand_balanced():
    """Eight unit cubes at x = 0..3 and 10..13 under the balanced hierarchy "8".  Surfaces (dx dy + dy dz + dz dx):
    a pair 2 + 1 + 2 = 5, a quadruple 4 + 1 + 4 = 9."""
    refs = np.array(HIER["8"][1], np.int32)
    lo, hi = _cubes([0, 1, 2, 3, 10, 11, 12, 13])
    t = AR.Tree2(refs, 0, 8, max_leaf=1)
    b = t.boxes(lo, hi)
    assert b[0].tolist() == [[[0, 0, 0], [4, 1, 1]], [[10, 0, 0], [14, 1, 1]]]
    assert b[3].tolist() == [[[0, 0, 0], [2, 1, 1]], [[2, 0, 0], [4, 1, 1]]]
    assert b[6].tolist() == [[[12, 0, 0], [13, 1, 1]], [[13, 0, 0], [14, 1, 1]]]
    assert AR.surface(b[0, 0, 0], b[0, 0, 1]) == 9 and AR.surface(b[3, 0, 0], b[3, 0, 1]) == 5
    # 4-wide: [n3, n4] tie at 9, the first wins: [n1, n4, n2]; then n4 (9 > 5): [n1, n5, n2, n6]
    lv, depth = AR.collapse(refs, b, 0, 4)
    assert depth == 2 and [[(n, r) for n, r, _ in level] for level in lv] == [
        [(0, [1, 5, 2, 6])], [(1, [L(0), L(1)]), (5, [L(4), L(5)]), (2, [L(2), L(3)]), (6, [L(6), L(7)])]]
    assert np.array(lv[0][0][2]).tolist() == [[[0, 0, 0], [2, 1, 1]], [[10, 0, 0], [12, 1, 1]], [[2, 0, 0], [4, 1, 1]], [[12, 0, 0], [14, 1, 1]]]
    # 8-wide: on from there, all at 5, the first maximum each time: n1, n5, n2, n6 in slot order
    lv, depth = AR.collapse(refs, b, 0, 8)
    assert depth == 1 and [(n, r) for n, r, _ in lv[0]] == [(0, [L(0), L(4), L(2), L(6), L(1), L(5), L(3), L(7)])]
    # the larger surface wins whatever its position: with the second quadruple spread out, n4 opens first
    lo, hi = _cubes([0, 1, 2, 3, 10, 12, 14, 16])
    lv, depth = AR.collapse(refs, t.boxes(lo, hi), 0, 4)
    assert [(n, r) for n, r, _ in lv[0]] == [(0, [1, 5, 6, 2])]


def test_collapse_by_hand_chain():
    """The chain "5 chain": only one inner child at a time, so the surfaces do not matter; the opened child's first
    half takes its slot, the second half goes to the end."""
    refs = np.array(HIER["5 chain"][1], np.int32)
    lo, hi = _cubes([0, 1, 2, 4, 8])
    t = AR.Tree2(refs, 0, 5, max_leaf=1)
    assert t.depth == 4
    b = t.boxes(lo, hi)
    lv, depth = AR.collapse(refs, b, 0, 4)
    assert depth == 2 and [[(n, r) for n, r, _ in level] for level in lv] == [[(0, [1, L(4), L(3), L(2)])], [(1, [L(0), L(1)])]]
    lv, depth = AR.collapse(refs, b, 0, 8)
    assert depth == 1 and [(n, r) for n, r, _ in lv[0]] == [(0, [L(0), L(4), L(3), L(2), L(1)])]
    assert AR.collapse(refs, b, L(0), 4) == ([], 0)              # the root is a leaf: no wide node, depth 0
    # two and three leaves: one wide node
    for name in ("2", "3"):
        r = np.array(HIER[name][1], np.int32)
        n = len(HIER[name][0])
        lo, hi = _cubes(range(n))
        lv, depth = AR.collapse(r, AR.Tree2(r, 0, n, max_leaf=1).boxes(lo, hi), 0, 4)
        assert depth == 1 and len(lv[0]) == 1 and sorted(lv[0][0][1]) == sorted(L(k) for k in range(n))


# ------------------------------------------------------------------ grid and quantiser
def test_grid_by_hand():
    base, scale = AR.grid([[-100, 0, 0]], [[65433, 131066, 32766.5]])       # extents 65533, 2 x 65533, 65533 / 2
    assert base.tolist() == [-100, 0, 0] and scale.tolist() == [1.0, 2.0, 0.5]
    base, scale = AR.grid([[0, 0, 0], [1, 1, 1]], [[0, 0, 0], [1, 2, 1]])   # the union of the boxes
    assert base.tolist() == [0, 0, 0] and scale.tolist() == [F(1) / F(65533), F(2) / F(65533), F(1) / F(65533)]
    base, scale = AR.grid([[0, 0, 0]], [[0, 0, 0]])                          # no extent: 1e-3
    assert scale.tolist() == [F(1e-3) / F(65533)] * 3
    # the refusals: a plane at or beyond +-1e30; bounds farther from the origin than 16 extents (96 = 16 x 6 passes)
    assert AR.grid([[-1e30, 0, 0]], [[1, 1, 1]]) is None and AR.grid([[0, 0, 0]], [[1, 1e30, 1]]) is None
    assert AR.grid([[-3e38, 0, 0]], [[3e38, 1, 1]]) is None
    assert AR.grid([[90, 0, 0]], [[96, 1, 1]]) is not None and AR.grid([[96, 0, 0]], [[102, 1, 1]]) is None
    assert AR.grid([[0, -102, 0]], [[1, -96, 1]]) is None and AR.grid([[0, -96, 0]], [[1, -90, 1]]) is not None


def test_quantiser_by_hand():
    base, scale = np.array([-100, 0, 0], np.float32), np.array([1.0, 2.0, 0.5], np.float32)
    # x: a box coplanar with the grid's low plane: floor(0) - 1 = -1 clamps to 0; at the high plane 65533 + 1 = 65534.
    # y (scale 2): 5 -> floor(2.5) - 1 = 1, ceil(2.5) + 1 = 4.  z (scale 0.5): on a grid line, 5 -> 10 - 1 = 9, 10 + 1 = 11
    ql, qh = AR.quantize([[-100, 5, 5], [65433, 0, 0]], [[-100, 5, 5], [65433, 131066, 32766.5]], base, scale)
    assert ql.tolist() == [[0, 1, 9], [65532, 0, 0]] and qh.tolist() == [[1, 4, 11], [65534, 65534, 65534]]
    # between grid lines: -99.5 -> floor(0.5) - 1 = -1 -> 0, ceil(0.5) + 1 = 2;  0.5 -> 100.5: 99, 102
    ql, qh = AR.quantize([[-99.5, 0, 0], [0.5, 0, 0]], [[-99.5, 0, 0], [0.5, 0, 0]], base, scale)
    assert ql[:, 0].tolist() == [0, 99] and qh[:, 0].tolist() == [2, 102]
    # extent 1: the float32 scale 1 / 65533 rounds down, the high plane lands at 65533.0001 and ceil + 1 gives 65535
    # without the clamp; a plane past the grid (none exists in a tree: the grid is the union) clamps to 65535 / 0
    b1, s1 = AR.grid([[0, 0, 0]], [[1, 1, 1]])
    assert float(F(1)) / float(s1[0]) > 65533
    ql, qh = AR.quantize([[0, 0, 0], [1, 1, 1], [-1, 2, 0.5]], [[1, 1, 1], [1, 1, 1], [2, 3, 0.5]], b1, s1)
    assert ql.tolist() == [[0, 0, 0], [65532, 65532, 65532], [0, 65535, 32765]] and qh.tolist() == [[65535] * 3, [65535] * 3, [65535, 65535, 32768]]
    assert AR.Q_EMPTY == (65535, 0)


def test_wide_layouts_by_hand():
    """crt_bvh.h: planes lo.x lo.y lo.z hi.x hi.y hi.z with one entry per child each, then the child references."""
    f = np.arange(32, dtype=np.float32)
    f[24:28] = np.array([3, L(0), 0, L(5, 2)], np.int32).view(np.float32)
    lo, hi, refs = AR.wide_split(f[None], 4, False)
    assert lo[0].tolist() == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11]] and hi[0, 1].tolist() == [13, 17, 21]
    assert refs.tolist() == [[3, -1, 0, -42]]
    q = np.arange(24, dtype=np.uint32)                           # two 16-bit coordinates per dword, the even child in the low half
    d = np.concatenate([q[0::2] | (q[1::2] << 16), np.array([1, 2, -1, 0], np.int32).view(np.uint32)])
    lo, hi, refs = AR.wide_split(d[None], 4, True)
    assert lo[0].tolist() == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11]] and hi[0, 3].tolist() == [15, 19, 23]
    assert refs.tolist() == [[1, 2, -1, 0]]
    q = np.arange(48, dtype=np.uint32)
    d = np.concatenate([q[0::2] | (q[1::2] << 16), np.arange(8, dtype=np.uint32)])
    lo, hi, refs = AR.wide_split(d[None], 8, True)
    assert lo[0, 0].tolist() == [0, 8, 16] and lo[0, 7].tolist() == [7, 15, 23] and hi[0, 1].tolist() == [25, 33, 41]
    assert refs.tolist() == [list(range(8))]


# ------------------------------------------------------------------ properties of the restated LBVH of every case
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if len(c.prims) >= 2] + ["chain_lbvh"])
def test_restated_lbvh_properties(name):
    case = CASES[name] if name in CASES else TC.case_chain()
    n = len(case.prims)
    order, refs, t, boxes = AR.lbvh(case.prims, TC.hit_pad(case.prims, case.eye))
    assert sorted(order.tolist()) == list(range(n))             # every primitive in exactly one leaf (Tree2 checks the slots)
    assert t.n2 == n - 1 and len(t.leaves) == n and 1 <= t.depth <= 62
    for width in (4, 8):
        lv, depth = AR.collapse(refs, boxes, 0, width)
        assert -(-t.depth // (width - 1)) <= depth <= t.depth      # a wide node takes in at most width - 1 BVH2 levels
        assert sorted(r for level in lv for _, rs, _ in level for r in rs if r < 0) == sorted(t.leaves.tolist())


def test_restated_depths_are_the_documented_ones():
    """DESIGN.md 3 (the stack table): BVH2 / 4-wide / 8-wide levels of the LBVH of the mixed scene and the deep case."""
    got = {}
    for name in ("baseline", "deep_lbvh"):
        c = CASES[name]
        _, refs, t, boxes = AR.lbvh(c.prims, TC.hit_pad(c.prims, c.eye))
        got[name] = (t.depth, AR.collapse(refs, boxes, 0, 4)[1], AR.collapse(refs, boxes, 0, 8)[1])
    assert got == {"baseline": (22, 10, 7), "deep_lbvh": (42, 15, 7)}


# ------------------------------------------------------------------ the chain case
def test_chain_case_keeps_one_wide_level_per_chain_level():
    case = TC.case_chain()
    cell, level = TC.chain_levels()
    pad = TC.hit_pad(case.prims, case.eye)
    assert TC.quantisable(case.prims, case.eye)
    lo, hi, unb = AR.prim_bounds(case.prims, pad)
    assert not unb.any() and AR.grid(lo, hi) is not None
    # the Morton cells are the designed ones (the filler in the last cell pins the box of the centres)
    code = AR.morton_keys(lo, hi) >> np.uint64(32)
    want = (AR._expand10(cell[:, 0].astype(np.uint64)) << np.uint64(2)) | (AR._expand10(cell[:, 1].astype(np.uint64)) << np.uint64(1)) | AR._expand10(cell[:, 2].astype(np.uint64))
    assert np.array_equal(code, want)
    order, refs, t, boxes = AR.lbvh(case.prims, pad)
    lv4, depth4 = AR.collapse(refs, boxes, 0, 4)
    assert (t.depth, depth4) == (31 + TC.CHAIN_J, 30 + TC.CHAIN_J) and depth4 >= 38
    assert 3 * depth4 > 16 + 96, "the walk of k_wf_trace2 can need more than the default overflow area"
    assert 3 * depth4 <= 16 + 384, "... and less than the limit at which the build falls back to the SAH builder"
    # every chain level but the last is one wide node on the way down: the rest of the chain and the level's three triangles
    node = lv4[0][0]
    for d in range(depth4 - 1):
        b2, rs, bx = node
        inner = [r for r in rs if r >= 0]
        tri = sorted(int(order[AR.leaf_range(r)[0]]) for r in rs if r < 0)
        if d == 0:                                              # the top sibling also holds the filler
            assert len(rs) == 4 and len(inner) >= 2
            nxt = [r for r in inner if t.range_of(r)[0] == 0]
        else:
            assert len(inner) == 1 and tri == np.flatnonzero(level == d).tolist(), (d, rs)
            nxt = inner
            rest = inner[0]
            a_rest = AR.surface(*[bx[rs.index(rest)][k] for k in (0, 1)])
            assert all(AR.surface(bx[i][0], bx[i][1]) > a_rest for i, r in enumerate(rs) if r < 0), d
        node = next(x for x in lv4[d + 1] if x[0] == nxt[0])
    assert sorted(int(order[AR.leaf_range(r)[0]]) for r in node[1]) == [0, 1, 2, 3]
    # the 8-wide tree of the same scene stays far from the 60 levels of the SAH fallback: a wide level takes at least
    # one BVH2 level, the 30 code bits give 30 of them, and level 31 + k on the index bits needs a primitive index
    # with bit k set below the code -- 60 levels need more than 2^29 primitives (40 GB of records)
    depth8 = AR.collapse(refs, boxes, 0, 8)[1]
    assert depth8 <= t.depth < 60 and 7 * depth8 <= 32 + 384


def test_chain_case_rays_do_their_work(orc):
    """The ray classes of the chain case, judged like those of every other case (test_traversal_cases_cpu.py)."""
    import test_traversal_cases_cpu as T
    T.CASES["chain_lbvh"] = TC.case_chain()
    try:
        T.test_ray_classes_against_the_oracle(orc, "chain_lbvh")
    finally:
        del T.CASES["chain_lbvh"]
