"""The acceleration trees judged as STRUCTURES (run with -m gpu on an MI355X): what crt_build_accel, crt_refit_accel and
crt_set_camera leave on the device is read back (crt_debug_read_accel) and held, exactly, to accel_ref.py -- a numpy
restatement of the building rules that test_accel_ref_cpu.py anchors to the reference loop and to hand-worked
examples.  The ray and image tests judge a tree by the rays that walk it and can only notice a box that is too small;
these notice a box that is too large, a copy of a rule that drifted, a recorded depth that is not the tree's.

For every case of traversal_cases.py x builder (bvh2, lbvh) x form (test_traversal_rays_gpu.FORMS), freshly built, stale
(primitives updated, not refitted), refitted, and edited back:

  1 topology   references in range, every inner node reached once, every slot in one leaf, leaf sizes; slot_of_index and
               the records are the packing rule's; non-empty slots of a wide node are a prefix, empty ones carry the
               documented encoding; the wide trees are cuts of the BVH2 with the BVH2's boxes
  2 boxes      every BVH2 child box == the union of accel_ref.prim_bounds of the leaves below it, bit for bit, whichever
               copy of the bound rule made it (host SAH build, host-route LBVH, device-route LBVH, refit kernels)
  3 LBVH       leaf order, hierarchy (with its numbering) and collapse == the restatement; so are the recorded depths
  4 routes     the all-device LBVH route and the host route give the same BVH2 and the same quantised 4-wide tree
  5 refit      a stale tree still holds the old boxes; the refit gives the boxes, grid and planes of the edited
               primitives on the unchanged topology; editing back restores every bit; a camera with a larger pad
               re-makes the boxes at that pad, a smaller pad leaves them
  6 quantiser  base + q scale encloses the float box and exceeds it by less than two grid units (unless clamped)
  7 stacks     the depth recorded for the wavefront walks is the depth of the tree read back, and the stack entries
               allocated cover (width - 1) x depth -- checked before any ray walks
  8 overflow   the chain case needs more than the default 96 overflow levels: checked structurally first, then walked

Everything is exact: min / max unions, float32 where the product uses float32, float64 where it uses double."""
import numpy as np
import pytest

import accel_ref as AR
import test_traversal_rays_gpu as T
import traversal_cases as TC
from test_traversal_rays_gpu import brutes  # noqa: F401  (the fixture: two contexts for the reference loop)

pytestmark = pytest.mark.gpu

CASES = T.CASES
FORMS = T.FORMS
NO_RAYS = np.zeros((0, 3), np.float32)
_REF = {}                                                     # restated trees, made once per (case, state)


def restated(name, state, prims, pad, lbvh=False):
    """prim_bounds and (lbvh) the LBVH of a case's primitives at `pad`, cached: the forms and builders share them."""
    key = (name, state, float(pad) if np.isfinite(pad) else str(pad))
    if key not in _REF:
        lo, hi, unb = AR.prim_bounds(prims, pad)
        if len(_REF) > 12:
            _REF.clear()
        _REF[key] = dict(lo=lo, hi=hi, unb=unb, grid=AR.grid(lo, hi))
    ref = _REF[key]
    if lbvh and "refs" not in ref:
        order, refs, t, boxes = AR.lbvh(prims, pad)
        ref.update(order=order, refs=refs, tree=t, boxes=boxes)
    return ref


def same(a, b):
    """Bit for bit (float arrays as their bits: -0 is not +0, and a NaN equals the same NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def first_diff(a, b):
    d = np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))
    return f"{len(d)} values differ, first at {d[0].tolist()}: {a[tuple(d[0])]!r} != {b[tuple(d[0])]!r}"


# ------------------------------------------------------------------ one read-back structure against the rules
def check_wide(A, t2, boxes2, width, quantised, rule, what):
    """A read-back wide tree against the BVH2 it was collapsed from; rule: AR.collapse of that BVH2 where the tree must
    be the collapse rule's own (a refit keeps the topology of the boxes it was built with).  Returns (depth, refs)."""
    name = "nodes8q" if width == 8 else ("nodes4q" if quantised else "nodes4")
    lo, hi, refs = AR.wide_split(A[name], width, quantised)
    nw, root = len(refs), A["root8" if width == 8 else "root4"]
    assert nw == A["n8" if width == 8 else "n4"], what
    if t2.root < 0:                                             # the BVH2 is one leaf: no wide node
        assert nw == 0 and root == t2.root, (what, nw, root)
        return 0, refs
    assert root == 0 and nw >= 1, (what, root, nw)
    R = refs.tolist()
    # levels from the root: every node once, references in range, non-empty slots a prefix
    levels, seen, cur = [], np.zeros(nw, bool), [0]
    kids = [0] * nw
    while cur:
        nxt = []
        for w in cur:
            assert 0 <= w < nw and not seen[w], f"{what}: wide node {w} is out of range or reached twice"
            seen[w] = True
            k = sum(1 for r in R[w] if r != 0)
            assert k >= 2 and all(r != 0 for r in R[w][:k]) and all(r == 0 for r in R[w][k:]), f"{what}: node {w}: the non-empty slots of {R[w]} are no prefix"
            kids[w] = k
            nxt += [r for r in R[w][:k] if r > 0]
        levels.append(cur)
        cur = nxt
        assert len(levels) <= 64, what
    assert seen.all(), f"{what}: {int((~seen).sum())} wide nodes are not reached from the root"
    kid = np.array(kids)
    empty = np.arange(width)[None, :] >= kid[:, None]
    if quantised:
        assert (lo[empty] == AR.Q_EMPTY[0]).all() and (hi[empty] == AR.Q_EMPTY[1]).all(), f"{what}: an empty slot is a real box"
    else:
        assert (lo[empty] == AR.F_EMPTY).all() and (hi[empty] == AR.F_EMPTY).all(), f"{what}: an empty slot is a real box"
    # the range of slots below every wide node, bottom-up; its children tile it
    first, count = [0] * nw, [0] * nw
    for level in reversed(levels):
        for w in level:
            rg = []
            for r in R[w][:kids[w]]:
                rg.append((first[r], count[r]) if r > 0 else ((~r) >> 3, ((~r) & 7) + 1))
            s = sorted(rg)
            assert all(s[i][0] + s[i][1] == s[i + 1][0] for i in range(len(s) - 1)), f"{what}: the children of wide node {w} do not tile a range: {s}"
            first[w], count[w] = s[0][0], sum(c for _, c in s)
    # every wide child is a node or leaf of the BVH2 (found by its range), and a wide node stands for a BVH2 node
    by_range = {(int(t2.first[b]), int(t2.count[b])): b for b in range(t2.n2)}
    leaf_set = set(t2.leaves.tolist())
    assert (first[0], count[0]) == (int(t2.first[t2.root]), int(t2.count[t2.root])), what
    ref2 = np.zeros((nw, width), np.int64)                      # the BVH2 reference each slot stands for
    b2_of = [by_range.get((first[w], count[w]), -1) for w in range(nw)]
    assert min(b2_of) >= 0, f"{what}: wide node {b2_of.index(-1)} covers slots {first[b2_of.index(-1)]}+{count[b2_of.index(-1)]}, which is no BVH2 node"
    for w in range(nw):
        for i, r in enumerate(R[w][:kids[w]]):
            if r < 0:
                assert r in leaf_set, f"{what}: wide node {w} slot {i}: {r} is no leaf of the BVH2"
            ref2[w, i] = r if r < 0 else b2_of[r]
    # the boxes: the BVH2's own child boxes, bit for bit (float) or through the quantiser
    inner_box = np.zeros((max(t2.n2, 1), 2, 3), np.float32)
    leaf_box = np.zeros((t2.nslot, 2, 3), np.float32)
    r2 = t2.refs.astype(np.int64)
    for c in range(2):
        m = r2[:, c] >= 0
        inner_box[r2[m, c]] = boxes2[m, c]
        leaf_box[AR.leaf_range(r2[~m, c])[0]] = boxes2[~m, c]
    lf = AR.leaf_range(np.minimum(ref2, -1))[0]
    box = np.where((ref2 < 0)[..., None, None], leaf_box[np.where(ref2 < 0, lf, 0)], inner_box[np.maximum(ref2, 0)])   # (nw, width, 2, 3)
    full = ~empty
    if quantised:
        base, scale = A["qbase"], A["qscale"]
        ql, qh = AR.quantize(box[:, :, 0], box[:, :, 1], base, scale)
        assert same(lo[full], ql[full]) and same(hi[full], qh[full]), f"{what}: {name} is not the quantiser's rule applied to the BVH2's boxes"
        # 6: conservative and tight, from the grid alone (float64)
        b, s = base.astype(np.float64), scale.astype(np.float64)
        plo, phi = b + lo.astype(np.float64) * s, b + hi.astype(np.float64) * s
        flo, fhi = box[:, :, 0].astype(np.float64), box[:, :, 1].astype(np.float64)
        assert (plo[full] <= flo[full]).all() and (phi[full] >= fhi[full]).all(), f"{what}: a quantised box does not enclose its float box"
        loose_lo = ((flo - plo >= 2 * s) & (lo != 0))[full]
        loose_hi = ((phi - fhi >= 2 * s) & (hi != 65535))[full]
        assert not loose_lo.any() and not loose_hi.any(), f"{what}: {int(loose_lo.sum() + loose_hi.sum())} planes are two grid units or more outside their float box"
    else:
        assert same(lo[full], box[:, :, 0][full]) and same(hi[full], box[:, :, 1][full]), f"{what}: a float 4-wide box is not its BVH2 child's box"
    if rule is not None:
        lv, depth = rule
        want = {b: rs for level in lv for b, rs, _ in level}
        assert depth == len(levels) and len(want) == nw, (what, depth, len(levels))
        for w in range(nw):
            assert b2_of[w] in want and ref2[w, :kids[w]].tolist() == want[b2_of[w]], (
                f"{what}: wide node {w} (BVH2 node {b2_of[w]}) holds {ref2[w, :kids[w]].tolist()}, the collapse rule gives {want.get(b2_of[w])}")
    return len(levels), refs


def check(A, case, name, state, prims, builder, form, what, collapse_rule=True):
    """Parts 1, 2, 3, 6, 7 on one read-back structure.  collapse_rule: the tree was BUILT from these primitives (fresh,
    or rebuilt), so its order, hierarchy and collapse are the rules' own; a refitted tree keeps its topology and is held
    to everything else.  Returns (Tree2, BVH2 child boxes)."""
    n = len(prims)
    assert (A["accel_mode"], A["nprim"]) == (1, n), what
    by_lbvh = builder == "lbvh" and n >= 2
    assert A["builder"] == int(by_lbvh), (what, A["builder"])
    pad = A["tree_pad"]
    ref = restated(name, state, prims, pad, by_lbvh and collapse_rule)
    # 1: the records and the permutation
    order = A["prim"].view(np.uint32)[:, 7].astype(np.int64)
    assert sorted(order.tolist()) == list(range(n)), f"{what}: the B.w indices of the records are no permutation"
    assert np.array_equal(A["slot_of_index"][order], np.arange(n)), f"{what}: slot_of_index is not the inverse of the leaf order"
    want_prim, want_d = AR.pack_records(prims[order])
    nan_ok = np.isnan(want_d) & np.isnan(A["primD"])            # (a NaN normal has no agreed payload)
    assert same(A["prim"], want_prim), f"{what}: prim: {first_diff(A['prim'], want_prim)}"
    assert same(np.where(nan_ok, 0, A["primD"]), np.where(nan_ok, 0, want_d)), f"{what}: primD: {first_diff(A['primD'], want_d)}"
    # 1: the BVH2's topology (Tree2 asserts it), 2: its boxes
    boxes2, refs2 = AR.nodes2_split(A["nodes2"])
    assert len(refs2) == A["n2"], what
    t2 = AR.Tree2(refs2, A["root"], n, max_leaf=1 if by_lbvh else AR.MAX_LEAF)
    assert t2.n2 == (n - 1 if by_lbvh else t2.n2) and A["depth2"] == t2.depth, (what, A["depth2"], t2.depth)
    want_boxes = t2.boxes(ref["lo"][order], ref["hi"][order])
    assert same(boxes2, want_boxes), f"{what}: BVH2 boxes are not the union of the primitives' bounds at pad {pad!r}: {first_diff(boxes2, want_boxes)}"
    # 3: the LBVH is the restated one (a refitted tree keeps the order and hierarchy of the primitives it was built from)
    if by_lbvh and collapse_rule:
        assert np.array_equal(order, ref["order"]), f"{what}: the leaf order is not the order of the restated Morton keys"
        assert np.array_equal(refs2, ref["refs"]), f"{what}: the hierarchy is not the restated one: {first_diff(refs2, ref['refs'])}"
        assert t2.depth == ref["tree"].depth
    # which wide trees there are
    _, width, bpb, _, q = T.expected_tree(case, prims, builder, form, t2.n2 == 0)
    device_route = by_lbvh and q and width == 4
    assert A["device_route"] == int(device_route), (what, A["device_route"])
    assert (A["live4"], A["live4q"], A["live8q"]) == (int(t2.n2 > 0 and not device_route), int(q), int(q and width == 8)), what
    if q:
        assert ref["grid"] is not None and same(A["qbase"], ref["grid"][0]) and same(A["qscale"], ref["grid"][1]), (what, A["qbase"], A["qscale"], ref["grid"])
    depth = 0
    rule = {w: AR.collapse(t2.refs, boxes2, t2.root, w) if collapse_rule and (A["live8q"] if w == 8 else A["n4"]) else None for w in (4, 8)}
    if A["live4"]:
        depth, refs4 = check_wide(A, t2, boxes2, 4, False, rule[4], what + " / float 4-wide")
    if A["live4q"]:
        depth, refs4q = check_wide(A, t2, boxes2, 4, True, rule[4], what + " / quantised 4-wide")
        if A["live4"]:
            assert np.array_equal(refs4, refs4q), f"{what}: the quantised and the float 4-wide tree differ in their references"
    if t2.n2:
        assert A["depth4"] == depth, (what, A["depth4"], depth)
    if A["live8q"]:
        depth, _ = check_wide(A, t2, boxes2, 8, True, rule[8], what + " / quantised 8-wide")
        assert A["depth8"] == depth, (what, A["depth8"], depth)
    # 7: the depth the stacks are sized by is the depth of the tree the wavefront kernels walk
    w = 8 if A["live8q"] else 4
    assert A["wf_depth"] == depth, f"{what}: recorded depth {A['wf_depth']}, the {w}-wide tree read back has {depth} levels"
    assert A["wf_stack_need"] == (w - 1) * depth, (what, A["wf_stack_need"], w, depth)
    assert A["wf_stack_lds"] == (16 if q and w == 4 and form != "wf_trace_form=1" else 32), (what, A["wf_stack_lds"])
    assert A["wf_overflow_levels"] >= 96 and A["overflow_allocated"] >= A["wf_overflow_levels"], (what, A["wf_overflow_levels"], A["overflow_allocated"])
    assert A["overflow_allocated"] + A["wf_stack_lds"] >= A["wf_stack_need"], f"{what}: {A['overflow_allocated']} + {A['wf_stack_lds']} stack entries for a walk that can need {A['wf_stack_need']}"
    return t2, boxes2


NODE_ARRAYS = ("nodes2", "nodes4", "nodes4q", "nodes8q")


def read(renderer):
    """The structure, with the overflow area allocated as the next trace call would (a call without rays: no walk)."""
    if not renderer.debug_read_accel()["stale"]:
        renderer.debug_trace_rays(NO_RAYS, NO_RAYS)
    return renderer.debug_read_accel()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("builder", ["bvh2", "lbvh"])
@pytest.mark.parametrize("name", list(CASES))
def test_trees_are_what_the_rules_say(renderer, name, builder, form):
    case = CASES[name]
    runs, ed = TC.edited(case, np.random.default_rng(77))
    try:
        T.set_form(renderer, form)
        renderer.upload(TC.packed(case)).build_accel(builder)
        what = f"{name} / {builder} / {form}"
        A0 = read(renderer)
        assert A0["tree_pad"] == A0["hit_pad"] == TC.hit_pad(case.prims, case.eye) or np.isnan(A0["hit_pad"]), what
        t0, boxes0 = check(A0, case, name, "fresh", case.prims, builder, form, what + " / fresh")
        # 5: stale -- the records are the edited ones, every box is still the old one
        for first, rec in runs:
            renderer.update_primitives(first, rec)
        A1 = read(renderer)
        order = A0["prim"].view(np.uint32)[:, 7].astype(np.int64)
        assert A1["stale"] == 1 and same(A1["slot_of_index"], A0["slot_of_index"]), what
        assert same(A1["prim"], AR.pack_records(ed[order])[0]), f"{what}: the stale tree's records are not the edited primitives'"
        assert A1["tree_pad"] == A0["tree_pad"] and A1["hit_pad"] == TC.hit_pad(ed, case.eye), (what, A1["tree_pad"], A1["hit_pad"])
        for k in NODE_ARRAYS:
            assert same(A1[k], A0[k]), f"{what}: {k} changed before the refit"
        rebuilt = renderer.refit_accel()
        assert rebuilt is bool(A0["live8q"]), what                 # an 8-wide tree is rebuilt: the documented route
        A2 = read(renderer)
        assert not A2["stale"] and A2["tree_pad"] == A2["hit_pad"] == A1["hit_pad"], what
        t2, boxes2 = check(A2, case, name, "edited", ed, builder, form, what + (" / rebuilt" if rebuilt else " / refitted"), collapse_rule=rebuilt)
        if not rebuilt:                                          # the topology is kept slot for slot, the boxes follow the primitives
            assert np.array_equal(t2.refs, t0.refs) and same(A2["slot_of_index"], A0["slot_of_index"]), what
            for k, w, qd in (("nodes4", 4, False), ("nodes4q", 4, True)):
                assert np.array_equal(AR.wide_split(A2[k], w, qd)[2], AR.wide_split(A0[k], w, qd)[2]), f"{what}: the refit changed the references of {k}"
            moved = np.zeros(len(ed), bool)
            for first, rec in runs:
                moved[first:first + len(rec)] = True
            # leaf children whose primitives all shrank: so did their boxes.  Triangles and patches wider than the
            # padding only (extents over 12 hit_pad beyond the 12 hit_pad of padding: a quarter of that is lost to
            # the contraction, rounding is far below); a sphere's radial term grows as its radius shrinks
            flat_ok = moved & (ed["category"] != 1)
            f, c = AR.leaf_range(np.minimum(t0.refs, -1).astype(np.int64))
            shrunk = np.zeros(t0.refs.shape, bool)
            for i, j in zip(*np.nonzero(t0.refs < 0)):
                shrunk[i, j] = flat_ok[order[f[i, j]:f[i, j] + c[i, j]]].all()
            with np.errstate(invalid="ignore", over="ignore"):
                ext0 = (boxes0[:, :, 1] - boxes0[:, :, 0]).astype(np.float64).sum(2)
                ext2 = (boxes2[:, :, 1] - boxes2[:, :, 0]).astype(np.float64).sum(2)
                shrunk &= np.isfinite(ext0) & (ext0 < 1e30) & (ext0 > 24 * float(A0["tree_pad"]))
            assert (ext2[shrunk] < ext0[shrunk]).all(), f"{what}: {int((ext2[shrunk] >= ext0[shrunk]).sum())} leaf boxes of shrunk primitives did not shrink"
        # edited back: every bit of the first build returns
        renderer.update_primitives(0, case.prims)
        rebuilt2 = renderer.refit_accel()
        A3 = read(renderer)
        assert rebuilt2 is rebuilt, what
        if A3["device_route"] and (rebuilt or rebuilt2):          # (a device collapse numbers the nodes of a level as they come)
            check(A3, case, name, "fresh", case.prims, builder, form, what + " / edited back")
        else:
            for k in NODE_ARRAYS + ("prim", "primD", "slot_of_index", "qbase", "qscale"):
                assert same(A3[k], A0[k]), f"{what}: {k} after editing back and refitting is not the first build's: {first_diff(A3[k], A0[k])}"
        for k in ("tree_pad", "hit_pad", "root", "root4", "root8", "n2", "n4", "n8", "depth2", "depth4", "depth8", "wf_depth", "wf_stack_need"):
            assert A3[k] == A0[k] or (np.isnan(A3[k]) and np.isnan(A0[k])), (what, k, A3[k], A0[k])
    finally:
        T.set_form(renderer, "defaults")


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if len(c.prims) >= 2 and TC.quantisable(c.prims, c.eye)])
def test_lbvh_routes_agree(renderer, name):
    """4: under the defaults the LBVH is built, collapsed and quantised on the device; wf_width = 8 takes the host
    route (BVH2 from the device, collapse and quantisation on the host), which still uploads nodes4q."""
    case = CASES[name]
    try:
        got = {}
        for form in ("defaults", "wf_width=8"):
            T.set_form(renderer, form)
            renderer.upload(TC.packed(case)).build_accel("lbvh")
            got[form] = renderer.debug_read_accel()
        D, Hh = got["defaults"], got["wf_width=8"]
        assert D["device_route"] and not Hh["device_route"] and D["builder"] == Hh["builder"] == 1 and Hh["live4q"] and Hh["live8q"]
        for k in ("nodes2", "prim", "primD", "slot_of_index", "qbase", "qscale"):
            assert same(D[k], Hh[k]), f"{name}: {k}: {first_diff(D[k], Hh[k])}"
        assert (D["n4"], D["depth2"], D["depth4"]) == (Hh["n4"], Hh["depth2"], Hh["depth4"])
        # the same quantised 4-wide tree up to the numbering of the nodes: walk both from the root, slot by slot
        dl, dh, dr = AR.wide_split(D["nodes4q"], 4, True)
        hl, hh, hr = AR.wide_split(Hh["nodes4q"], 4, True)
        pairs, seen = [(0, 0)], 0
        while pairs:
            a, b = (np.array(x) for x in zip(*pairs))
            seen += len(a)
            assert same(dl[a], hl[b]) and same(dh[a], hh[b]), f"{name}: the routes quantise a box differently"
            ra, rb = dr[a], hr[b]
            assert np.array_equal(np.where(ra > 0, 1, ra), np.where(rb > 0, 1, rb)), f"{name}: the routes collapse a node differently"
            pairs = list(zip(ra[ra > 0].tolist(), rb[rb > 0].tolist()))
        assert seen == D["n4"]
    finally:
        T.set_form(renderer, "defaults")


@pytest.mark.parametrize("form", ["defaults", "wf_trace_form=1", "quantize=0"])
@pytest.mark.parametrize("builder", ["bvh2", "lbvh"])
def test_camera_pad_and_the_boxes(renderer, builder, form):
    """5: a farther eye gives a larger hit_pad and crt_set_camera refits: the boxes are the unions at the new pad.  A
    nearer eye gives a smaller pad; the boxes stay as they are, conservative, at the pad the header names."""
    case = CASES["grid"]
    ps = TC.packed(case)
    far = ps.camera.copy()
    far[0:3] = case.eye * np.float32(6)
    try:
        T.set_form(renderer, form)
        renderer.upload(ps).build_accel(builder)
        A0 = read(renderer)
        renderer.set_camera(far)
        A1 = read(renderer)
        assert A1["tree_pad"] == A1["hit_pad"] == TC.hit_pad(case.prims, far[0:3]) > A0["tree_pad"]
        check(A1, case, "grid", "far", case.prims, builder, form, f"grid / {builder} / {form} / far eye", collapse_rule=False)
        assert not same(A1["nodes2"], A0["nodes2"])
        renderer.set_camera(ps.camera)
        A2 = read(renderer)
        assert A2["hit_pad"] == TC.hit_pad(case.prims, case.eye) < A2["tree_pad"] == A1["tree_pad"]
        check(A2, case, "grid", "far", case.prims, builder, form, f"grid / {builder} / {form} / near eye again", collapse_rule=False)
        for k in NODE_ARRAYS:
            assert same(A2[k], A1[k])
    finally:
        T.set_form(renderer, "defaults")


def test_chain_case_reaches_the_larger_overflow_area(renderer, brutes, orc):  # noqa: F811
    """8: the chain case's 4-wide LBVH keeps one wide level per BVH2 level, 3 x depth passes the 16 + 96 entries of the
    default area.  The structure is checked first -- the depth recorded is the depth read back and restated, and the
    area allocated covers it -- and only then do rays walk it, once, through the counting kernel."""
    case = TC.case_chain()
    name = case.name
    renderer.upload(TC.packed(case)).build_accel("lbvh")
    A = read(renderer)
    check(A, case, name, "fresh", case.prims, "lbvh", "defaults", name)
    ref = restated(name, "fresh", case.prims, A["tree_pad"], True)
    depth = AR.collapse(ref["refs"], ref["boxes"], 0, 4)[1]
    assert A["device_route"] and depth >= 38 and A["wf_depth"] == depth, (A["wf_depth"], depth)
    assert A["wf_stack_need"] == 3 * depth > 16 + 96
    assert A["wf_overflow_levels"] == 3 * depth - 16 > 96
    assert A["overflow_allocated"] + A["wf_stack_lds"] >= 3 * depth, "the walk below would leave the area: not run"
    st = T.State(case, None, brutes, orc, 40, n=600)
    try:
        renderer.enable_counters(True)
        rep = st.check(renderer, name + " / lbvh / defaults / counting")
    finally:
        renderer.enable_counters(False)
    print(f"chain: depth {depth}, overflow levels {rep['overflow_levels']}, deepest stack {rep['deepest']} of {rep['capacity']}")
    assert rep["kernel"] == "k_wf_trace2" and rep["counting"] and rep["overflow_levels"] == A["wf_overflow_levels"] and rep["depth"] == depth
    assert 0 < rep["deepest"] <= 3 * depth <= rep["capacity"], rep
