"""A numpy binary64 restatement of the tree cost crt_accel_quality reports (include/crt.h pins the definition), written
from that definition and working from the parts crt_debug_read_accel returns (Renderer.debug_read_accel): the header,
NODES2 and NODES4 / NODES4Q.

  A(box) = dx dy + dy dz + dz dx,  d = hi - lo, in float64 on the box values converted from what the device holds
  BVH2    box_i = the union of node i's two child boxes;  boxes2 = sum_i 2 A(box_i) / A(box_root),
          prims2 = sum over leaf children of count A(child box) / A(box_root)
  4-wide  an empty slot (ref == 0) is skipped; a quantised plane is float64(base) + float64(q) float64(scale);
          box_i = the union of node i's live child boxes;  boxes4 = sum_i nch_i A(box_i) / A(box_root),
          prims4 = sum over leaf children of count A(child box) / A(box_root)
  a leaf is ref < 0, ~ref = first << 3 | count - 1

Every function also returns how many terms its sums have: the tests' tolerance is stated in terms."""
from __future__ import annotations

import numpy as np


def area(lo, hi):
    d = hi - lo
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def _cost(lo, hi, refs, live, weight, root):
    """lo, hi (n, w, 3) float64, refs (n, w) int, live (n, w) bool, weight (n,): (boxes, prims, terms of each)."""
    with np.errstate(invalid="ignore", over="ignore"):
        blo = np.fmin.reduce(np.where(live[..., None], lo, np.inf), axis=1)
        bhi = np.fmax.reduce(np.where(live[..., None], hi, -np.inf), axis=1)
        a_node = area(blo, bhi)
        leaf = live & (refs < 0)
        count = ((~refs.astype(np.int64)) & 7) + 1
        a_child = area(lo, hi)
        boxes = float((weight * a_node).sum() / a_node[root])
        prims = float((count * a_child)[leaf].sum() / a_node[root])
    return boxes, prims, len(a_node), int(leaf.sum())


def cost2(nodes2, root):
    """(boxes2, prims2, terms, terms) of a read-back BVH2 node array (n2, 16) float32."""
    nd = np.ascontiguousarray(nodes2, np.float32).reshape(-1, 16)
    box = nd[:, :12].astype(np.float64).reshape(-1, 2, 2, 3)      # [child][lo | hi][axis]
    refs = nd[:, 12:14].copy().view(np.int32)
    return _cost(box[:, :, 0], box[:, :, 1], refs, np.ones(refs.shape, bool), np.full(len(nd), 2.0), int(root))


def cost4(nodes, quantised, base=None, scale=None, root=0):
    """(boxes4, prims4, terms, terms) of a read-back 4-wide node array: (n4, 32) float32, or (n4, 16) uint32 on the
    grid base / scale (float32)."""
    if quantised:
        nd = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
        q = nd[:, :12].copy().view(np.uint16).reshape(-1, 6, 4).astype(np.float64)      # [plane lo.x .. hi.z][child]
        b, s = np.asarray(base, np.float32).astype(np.float64), np.asarray(scale, np.float32).astype(np.float64)
        planes = np.concatenate([b[None, :, None] + q[:, 0:3] * s[None, :, None], b[None, :, None] + q[:, 3:6] * s[None, :, None]], axis=1)
        refs = nd[:, 12:16].copy().view(np.int32)
    else:
        nd = np.ascontiguousarray(nodes, np.float32).reshape(-1, 32)
        planes = nd[:, :24].astype(np.float64).reshape(-1, 6, 4)
        refs = nd[:, 24:28].copy().view(np.int32)
    lo, hi = planes[:, 0:3].transpose(0, 2, 1), planes[:, 3:6].transpose(0, 2, 1)      # (n, child, axis)
    live = refs != 0
    return _cost(lo, hi, refs, live, live.sum(1).astype(np.float64), int(root))


def quality(A):
    """From Renderer.debug_read_accel(): (values [boxes2, prims2, boxes4, prims4] float64, terms [4] -- the number of
    terms of each sum --, has4).  Zeros without an inner node; NaN for the 4-wide pair where the 8-wide tree is walked."""
    v, terms = np.zeros(4), [0, 0, 0, 0]
    if A["accel_mode"] != 1 or A["n2"] == 0 or A["root"] < 0:
        return v, terms, True
    v[0], v[1], terms[0], terms[1] = cost2(A["nodes2"], A["root"])
    if A["live8q"]:
        v[2] = v[3] = np.nan
        return v, terms, False
    if A["live4q"]:
        v[2], v[3], terms[2], terms[3] = cost4(A["nodes4q"], True, A["qbase"], A["qscale"], A["root4"])
    elif A["live4"]:
        v[2], v[3], terms[2], terms[3] = cost4(A["nodes4"], False, root=A["root4"])
    return v, terms, True
