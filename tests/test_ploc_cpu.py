"""CPU-only: the clustered GPU build (CRT_ACCEL_PLOC) as its definition says it -- ploc_ref.py, the numpy restatement
test_ploc_gpu.py holds the device to, bit for bit.

  interface   the mode is declared and bound in every host (header, ctypes, Renderer, the Node maps); the ABI stays 2
  by hand     four boxes whose merges can be written down: references, node numbers, order, slots; the tie-break
  every case  of traversal_cases.py: a valid tree (Tree2), the boxes are the unions, depth <= 62, rounds <= 64, and
              300 coincident triangles give a balanced tree (the XOR tie-break; "lowest index wins" gives 299 levels)
  quality     sum of node surfaces / root surface against the LBVH of the same primitives: <= 0.90 on mesh10k (0.847
              measured), <= 0.80 on atrium250k (0.702 measured), at radius 8 and the scene's own hit_pad"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import accel_ref as AR
import ploc_ref as PR
import traversal_cases as TC
from conftest import ROOT

NODE = shutil.which("node")
CASES = {c.name: c for c in TC.all_cases() + [TC.case_chain()] if len(c.prims) >= 2}
_TREES = {}


def tree(name):
    if name not in _TREES:
        c = CASES[name]
        pad = TC.hit_pad(c.prims, c.eye)
        _TREES[name] = (pad,) + PR.ploc(c.prims, pad)
    return _TREES[name]


# ------------------------------------------------------------------ interface
def test_the_mode_is_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "crt.h")).read()
    assert re.search(r"\bCRT_ACCEL_PLOC\s*=\s*3\b", text)
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+2\b", text) or re.search(r"CRT_ABI_VERSION\s*=\s*2\b", text)
    from computeraytracer_amd import _lib, renderer
    assert _lib.ACCEL_PLOC == 3
    assert renderer._ACCEL["ploc"] == 3 and renderer._ACCEL[_lib.ACCEL_PLOC] == 3
    assert _lib.load().crt_abi_version() == 2
    import computeraytracer_amd.__main__ as cli
    assert '"ploc"' in open(cli.__file__).read()


@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.parametrize("host", ["main.js", "multi.js"])
def test_the_node_hosts_map_the_mode(host):
    src = open(os.path.join(ROOT, "host", host)).read()
    m = re.search(r"const ACCEL = (\{[^}]*\});", src)
    assert m, host
    out = subprocess.run([NODE, "-e", f"const A = {m.group(1)}; console.log(A.ploc, A.lbvh, A.bvh2, A.none)"], capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["3", "2", "1", "0"]
    assert "ploc" in open(os.path.join(ROOT, "host", "index.js")).read()


# ------------------------------------------------------------------ by hand
def line_boxes(xs):
    """Unit cubes [x, x + 1] x [0, 1] x [0, 1]: the union of two has the cost 2 (extent in x) + 1."""
    lo = np.array([[x, 0, 0] for x in xs], np.float32)
    return lo, (lo + np.float32(1)).astype(np.float32)


def test_four_boxes_by_hand():
    # costs: (0,2) and (1,3) 6, (1,2) 20, (0,1) and (2,3) 23, (0,3) 26.  Round 1 merges 0 with 2 (node 2: made first) and
    # 1 with 3 (node 1); round 2 makes the root.  Node 2 covers slots 0..1, node 1 slots 2..3.
    lo, hi = line_boxes([0.0, 10.0, 1.5, 11.5])
    refs0, boxes, ccount, rounds, height = PR.cluster(lo, hi, 8)
    assert refs0.tolist() == [[2, 1], [~1, ~3], [~0, ~2]] and rounds == [(1, 2), (0, 1)] and height == 2
    assert ccount.tolist() == [[2, 2], [1, 1], [1, 1]]
    assert boxes[0, 0].tolist() == [[0, 0, 0], [2.5, 1, 1]] and boxes[0, 1].tolist() == [[10, 0, 0], [12.5, 1, 1]]
    refs, slot_of_pos = PR.slots(refs0, ccount, rounds, 4)
    assert slot_of_pos.tolist() == [0, 2, 1, 3]
    assert refs.tolist() == [[2, 1], [~(2 << 3), ~(3 << 3)], [~(0 << 3), ~(1 << 3)]]
    assert (refs[refs >= 0] > np.nonzero(refs >= 0)[0]).all()                   # a child's id is greater than its parent's
    t = AR.Tree2(refs, 0, 4, max_leaf=1)
    assert t.depth == 2
    # radius 1: only (1,2) is mutual at first (20 < 23); then 0 and 3 both cost 23 with the pair, and the XOR of the
    # positions decides for (0,1); three rounds, three levels
    refs0, _, ccount, rounds, height = PR.cluster(lo, hi, 1)
    assert refs0.tolist() == [[1, ~3], [~0, 2], [~1, ~2]] and rounds == [(2, 1), (1, 1), (0, 1)] and height == 3
    refs, slot_of_pos = PR.slots(refs0, ccount, rounds, 4)
    assert slot_of_pos.tolist() == [0, 1, 2, 3] and refs.tolist() == [[1, ~(3 << 3)], [~0, 2], [~(1 << 3), ~(2 << 3)]]


def test_four_identical_boxes_give_the_balanced_tree():
    lo, hi = line_boxes([3.0, 3.0, 3.0, 3.0])
    refs0, _, ccount, rounds, height = PR.cluster(lo, hi, 8)
    assert refs0.tolist() == [[2, 1], [~2, ~3], [~0, ~1]] and rounds == [(1, 2), (0, 1)] and height == 2
    refs, slot_of_pos = PR.slots(refs0, ccount, rounds, 4)
    assert slot_of_pos.tolist() == [0, 1, 2, 3]


def test_a_cost_that_is_not_finite_counts_as_flt_max():
    lo = np.float32([[-3e38, -3e38, -3e38], [0, 0, 0], [0, 0, 0]])
    hi = np.float32([[3e38, 3e38, 3e38], [1, 1, 1], [0, 5, 5]])
    c = PR.union_surface(lo[[0, 0]], hi[[0, 0]], lo[[1, 2]], hi[[1, 2]])
    assert (c == PR.FLT_MAX).all() and c.dtype == np.float32
    assert PR.nearest(lo, hi, 8).tolist() == [1, 2, 1]           # (0's two costs tie at FLT_MAX: 0 ^ 1 < 0 ^ 2)


# ------------------------------------------------------------------ every case
@pytest.mark.parametrize("name", list(CASES))
def test_the_restated_tree_is_a_tree(name):
    c = CASES[name]
    n = len(c.prims)
    pad, order, refs, t, boxes, rounds = tree(name)
    assert t.n2 == n - 1 and t.root == 0 and len(t.leaves) == n                # (Tree2 asserted slots and ranges)
    assert sorted(order.tolist()) == list(range(n))
    inner = refs >= 0
    assert (refs[inner] > np.nonzero(inner)[0]).all(), "a child's id is not greater than its parent's"
    lo, hi, _ = AR.prim_bounds(c.prims, pad)
    want = t.boxes(lo[order], hi[order])
    assert np.array_equal(boxes.view(np.uint32), want.view(np.uint32)), "a child box is not the union of its slots' boxes"
    assert t.depth <= 62 and rounds <= 64, (t.depth, rounds)
    if name == "coincident_tri300":
        assert t.depth <= 12, t.depth


# ------------------------------------------------------------------ quality
@pytest.mark.parametrize("scene, bound", [("mesh10k", 0.90), ("atrium250k", 0.80)])
def test_surface_cost_against_the_lbvh(scene, bound):
    from computeraytracer_amd import scenes_synth
    ps = getattr(scenes_synth, scene)()
    pad = TC.hit_pad(ps.primitives, ps.camera[0:3])
    _, _, t, boxes, rounds = PR.ploc(ps.primitives, pad, 8)
    _, _, tl, bl = AR.lbvh(ps.primitives, pad)
    ratio = PR.sah_cost(t, boxes) / PR.sah_cost(tl, bl)
    print(f"{scene}: pad {pad!r}, PLOC cost {PR.sah_cost(t, boxes):.3f} depth {t.depth} rounds {rounds}, LBVH cost {PR.sah_cost(tl, bl):.3f} "
          f"depth {tl.depth}, ratio {ratio:.4f}")
    assert ratio <= bound, ratio
