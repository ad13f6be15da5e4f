"""CPU-only: the restatement of the tree cost (accel_quality_ref.py) against a second route and against trees worked by
hand, and the new call's presence in the library, the binding and the header.

  two routes   boxes2 of the restatement == 2 x ploc_ref.sah_cost on a ploc_ref tree and on an accel_ref LBVH: the same
               formula (sum of node surfaces over the root's, float64) written twice, so only the last bits may differ
  by hand      a BVH2 of two nodes, and a 4-wide tree of two nodes with an empty slot, in the float and in the quantised
               layout, with numbers small enough to do on paper (every value below is exact in float64)"""
import ctypes as C
import os
import re

import numpy as np

import accel_quality_ref as QR
import accel_ref as AR
import ploc_ref as PR
import traversal_cases as TC
from conftest import ROOT

ULP = 2.0 ** -52


def nodes2_of(refs, boxes):
    nd = np.zeros((len(refs), 16), np.float32)
    nd[:, :12] = np.asarray(boxes, np.float32).reshape(-1, 12)
    nd[:, 12:14] = np.asarray(refs, np.int32).view(np.float32)
    return nd


def test_boxes2_is_twice_the_sah_cost_of_ploc_ref():
    from computeraytracer_amd.scenes_synth import soup
    ps = soup(300, 64, 64)
    pad = TC.hit_pad(ps.primitives, ps.camera[0:3])
    for what, (refs, t, boxes) in (("ploc", PR.ploc(ps.primitives, pad, 8)[1:4]), ("lbvh", AR.lbvh(ps.primitives, pad)[1:4])):
        boxes2, prims2, n_boxes, n_prims = QR.cost2(nodes2_of(refs, boxes), t.root)
        want = 2.0 * PR.sah_cost(t, boxes)
        assert n_boxes == len(ps.primitives) - 1 and n_prims == len(ps.primitives) >= 300, what
        assert abs(boxes2 - want) <= 4 * ULP * want, (what, boxes2, want)
        # every leaf holds one primitive: prims2 = sum of the leaf boxes' surfaces over the root's
        b = np.asarray(boxes, np.float32).astype(np.float64)
        leaf = np.asarray(refs) < 0
        d = b[:, :, 1] - b[:, :, 0]
        a = d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]
        dr = np.maximum(b[t.root, 0, 1], b[t.root, 1, 1]) - np.minimum(b[t.root, 0, 0], b[t.root, 1, 0])
        want_p = a[leaf].sum() / (dr[0] * dr[1] + dr[1] * dr[2] + dr[2] * dr[0])
        assert abs(prims2 - want_p) <= 4 * ULP * want_p, (what, prims2, want_p)


def test_bvh2_by_hand():
    """Root (node 1, not node 0: the host builder's root may be any node): child 0 = node 0, child 1 = a leaf of 3.
    Node 0: two leaves of 1 and 4 primitives.
      node 0: c0 [0,1]^3 (A = 3), c1 [1,3]x[0,1]x[0,1] (A = 2 + 1 + 2 = 5); box [0,3]x[0,1]x[0,1]: A = 3 + 1 + 3 = 7
      node 1: c0 = node 0's box (A 7), c1 [0,3]x[1,2]x[0,2] (A = 3 + 2 + 6 = 11); box [0,3]x[0,2]x[0,2]: A = 6 + 4 + 6 = 16
      boxes2 = 2 (7 + 16) / 16, prims2 = (1 x 3 + 4 x 5 + 3 x 11) / 16"""
    nd = np.zeros((2, 16), np.float32)
    nd[0, :12] = [0, 0, 0, 1, 1, 1, 1, 0, 0, 3, 1, 1]
    nd[1, :12] = [0, 0, 0, 3, 1, 1, 0, 1, 0, 3, 2, 2]
    nd[0, 12:14] = np.array([AR.leaf_ref(0, 1), AR.leaf_ref(1, 4)], np.int32).view(np.float32)
    nd[1, 12:14] = np.array([0, AR.leaf_ref(5, 3)], np.int32).view(np.float32)
    assert QR.cost2(nd, 1) == (2 * 23 / 16, 56 / 16, 2, 3)


def wide_by_hand():
    """Node 0 (root): an inner child (node 1), a leaf of 2, a leaf of 1, one empty slot.  Node 1: leaves of 4 and 1.
      node 1: [0,2]x[0,2]x[0,2] (A 12) and [2,4]x[0,2]x[0,1] (A = 4 + 2 + 2 = 8); box [0,4]x[0,2]x[0,2]: A = 8 + 4 + 8 = 20
      node 0: node 1's box (A 20), [0,4]x[2,4]x[0,2] (A = 8 + 4 + 8 = 20), [4,8]x[0,4]x[0,2] (A = 16 + 8 + 8 = 32);
              box [0,8]x[0,4]x[0,2]: A = 32 + 8 + 16 = 56
      boxes4 = (3 x 56 + 2 x 20) / 56, prims4 = (2 x 20 + 1 x 32 + 4 x 12 + 1 x 8) / 56"""
    lo = np.zeros((2, 4, 3)); hi = np.zeros((2, 4, 3))
    lo[0, :3], hi[0, :3] = [[0, 0, 0], [0, 2, 0], [4, 0, 0]], [[4, 2, 2], [4, 4, 2], [8, 4, 2]]
    lo[1, :2], hi[1, :2] = [[0, 0, 0], [2, 0, 0]], [[2, 2, 2], [4, 2, 1]]
    refs = np.array([[1, AR.leaf_ref(5, 2), AR.leaf_ref(7, 1), 0], [AR.leaf_ref(0, 4), AR.leaf_ref(4, 1), 0, 0]], np.int32)
    return lo, hi, refs, ((3 * 56 + 2 * 20) / 56, (40 + 32 + 48 + 8) / 56, 2, 4)


def test_float_4wide_by_hand():
    lo, hi, refs, want = wide_by_hand()
    nd = np.zeros((2, 32), np.float32)
    empty = refs == 0
    lo[empty], hi[empty] = AR.F_EMPTY, AR.F_EMPTY                # (what the builders leave there: skipped, not summed)
    nd[:, 0:12] = lo.transpose(0, 2, 1).reshape(2, 12)
    nd[:, 12:24] = hi.transpose(0, 2, 1).reshape(2, 12)
    nd[:, 24:28] = refs.view(np.float32)
    assert QR.cost4(nd, False) == want


def test_quantised_4wide_by_hand():
    """The same tree on the grid base (-1, 0, 0.5), scale (0.5, 0.25, 0.125): q = (plane - base) / scale, all exact."""
    lo, hi, refs, want = wide_by_hand()
    base, scale = np.float32([0.0, 0.0, 0.0]), np.float32([0.5, 0.25, 0.125])
    shift = np.float64([-1.0, 0.0, 0.5])                         # moving every box moves no surface
    ql, qh = (lo / scale).astype(np.uint16), (hi / scale).astype(np.uint16)
    empty = refs == 0
    ql[empty], qh[empty] = AR.Q_EMPTY
    planes = np.concatenate([ql.transpose(0, 2, 1).reshape(2, 12), qh.transpose(0, 2, 1).reshape(2, 12)], axis=1).astype(np.uint16)
    nd = np.zeros((2, 16), np.uint32)
    nd[:, :12] = np.ascontiguousarray(planes).view(np.uint32)
    nd[:, 12:16] = refs.view(np.uint32)
    assert QR.cost4(nd, True, (base + shift).astype(np.float32), scale) == want
    lo_r, hi_r, refs_r = AR.wide_split(nd, 4, True)              # the layout as accel_ref reads it
    assert np.array_equal(refs_r, refs) and np.array_equal(lo_r, ql) and np.array_equal(hi_r, qh)


def test_quality_of_a_read_back_structure():
    """quality() picks the trees by the header: zeros without an inner node, NaN for the 4-wide pair under the 8-wide
    tree, the quantised tree before the float one."""
    lo, hi, refs, want = wide_by_hand()
    v, terms, has4 = QR.quality(dict(accel_mode=1, n2=0, root=-1))
    assert v.tolist() == [0, 0, 0, 0] and terms == [0, 0, 0, 0] and has4
    v, terms, has4 = QR.quality(dict(accel_mode=0, n2=0, root=-1))
    assert v.tolist() == [0, 0, 0, 0] and has4
    nd2 = np.zeros((1, 16), np.float32)
    nd2[0, :12] = [0, 0, 0, 1, 1, 1, 1, 0, 0, 3, 1, 1]
    nd2[0, 12:14] = np.array([AR.leaf_ref(0, 1), AR.leaf_ref(1, 4)], np.int32).view(np.float32)
    v, terms, has4 = QR.quality(dict(accel_mode=1, n2=1, root=0, nodes2=nd2, live8q=1))
    assert v[0] == 2.0 and v[1] == 23 / 7 and np.isnan(v[2:]).all() and not has4 and terms == [1, 2, 0, 0]


def test_the_call_is_declared_exported_and_bound():
    from computeraytracer_amd import Renderer, _lib
    text = open(os.path.join(ROOT, "include", "crt.h")).read()
    assert re.search(r"int\s+crt_accel_quality\s*\(\s*crt_ctx\s*\*\s*ctx\s*,\s*double\s+out\[12\]\s*\)\s*;", text)
    assert '"refit_rebuild_pct"' in text
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+2\b", text) or re.search(r"CRT_ABI_VERSION\s*=\s*2\b", text)
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "crt_accel_quality")
    assert _lib.SIGNATURES["crt_accel_quality"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert callable(getattr(Renderer, "accel_quality"))
    assert _lib.load().crt_accel_quality(None, None) == -1       # CRT_EINVAL: no context, no GPU needed
    addon = open(os.path.join(ROOT, "addon", "crt_napi.c")).read()
    assert "accelQuality" in addon and "crt_accel_quality" in addon


def test_cli_refuses_rebuild_pct_without_animate_device():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-m", "computeraytracer_amd", "--rebuild-pct", "150"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 2 and "--rebuild-pct goes with --animate-device" in out.stderr
