"""A numpy restatement of the rules the acceleration trees are built by, written from DESIGN.md 3 and the comments of
crt_bvh.h -- not a translation of the builders.  float32 where the product computes in float32, float64 where it
computes in double; unions are min / max and therefore exact, so every box a test derives from here is expected bit
for bit.

  prim_bounds      the conservative box of a primitive: corner box, the region a patch's test accepts, the radial term
                   of a sphere, non-finite -> +-3e38, then -+ g
  lbvh             Morton keys, their order, and the hierarchy (a recursive split at the highest differing key bit)
                   with the node numbering of Karras' construction
  Tree2            a BVH2 as an array of child references: levels, reachability, leaf ranges, boxes bottom-up
  collapse         BVH2 -> 4- or 8-wide: open the inner child with the largest surface until the node is full
  grid / quantize  the 16-bit grid over the scene box and the outward rounding with one unit of slack

Child references are crt_bvh.h's: >= 0 an inner node, < 0 a leaf ~((first_slot << 3) | (count - 1))."""
from __future__ import annotations

import numpy as np

import traversal_cases as TC

F = np.float32
BIG = F(3.0e38)
MAX_LEAF = 4                      # crt_bvh.h kMaxLeaf (the SAH builder; an LBVH leaf holds one primitive)


# ------------------------------------------------------------------ primitive bounds
def prim_bounds(records, pad):
    """(lo (n, 3) float32, hi (n, 3) float32, unbounded (n,) bool) of the 80-byte records at hit_pad `pad`."""
    pad = F(pad)
    n = len(records)
    cat = records["category"]
    c = TC.corners(records)                                       # (n, 4, 3) float32
    nc = np.where(cat == 0, 4, np.where(cat == 1, 2, 3))
    lo, hi = c[:, 0].copy(), c[:, 0].copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(1, 4):                                     # a NaN in a later corner is dropped, one in the first stays
            use = (k < nc)[:, None]
            lo = np.where(use & (c[:, k] < lo), c[:, k], lo)
            hi = np.where(use & (c[:, k] > hi), c[:, k], hi)
        unb = np.zeros(n, bool)
        # patches: the region {P0 + m : 0 <= m.e1 <= e1.e1, 0 <= m.e2 <= e2.e2}, its four points in float64
        for i in np.flatnonzero(cat == 0):
            e1, e2, p0 = (records[k][i].astype(np.float64) for k in ("data2", "data3", "data1"))
            # (sums in index order, as a dot product is written)
            g11 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]
            g22 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]
            g12 = (e1[0] * e2[0] + e1[1] * e2[1]) + e1[2] * e2[2]
            det = g11 * g22 - g12 * g12
            if not det > 1e-9 * g11 * g22:
                lo[i], hi[i], unb[i] = -BIG, BIG, True
                continue
            for a, b in ((0.0, 0.0), (g11, 0.0), (0.0, g22), (g11, g22)):
                al, be = (a * g22 - b * g12) / det, (b * g11 - a * g12) / det
                v = ((p0 + al * e1) + be * e2).astype(np.float32)
                dn, up = np.nextafter(v, F(-np.inf)), np.nextafter(v, F(np.inf))
                lo[i] = np.where(dn < lo[i], dn, lo[i])
                hi[i] = np.where(up > hi[i], up, hi[i])
        g = np.full(n, F(2) * pad, np.float32)
        S = F(pad * F(131072.0))
        r = np.abs(records["data2"][:, 0]).astype(np.float32)
        rad = np.where(r > 0, np.minimum(F(F(S * S) * F(9.5367431640625e-07)) / r, S), S).astype(np.float32)
        g = np.where(cat == 1, g + rad, g).astype(np.float32)
        bad = ~np.isfinite(lo) | ~np.isfinite(hi)                 # per axis
        lo = np.where(bad, -BIG, lo)
        hi = np.where(bad, BIG, hi)
        unb |= bad.any(1)
        lo = (lo - g[:, None]).astype(np.float32)
        hi = (hi + g[:, None]).astype(np.float32)
    return lo, hi, unb


# ------------------------------------------------------------------ leaf-ordered records
def fma32(a, b, c):
    """fma(a, b, c) of float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd
    there (TwoSum gives the residual), and the final rounding to float32 is then the only one that counts."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def dot32(a, b):
    """The numeric contract's dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return fma32(a[:, 2], b[:, 2], fma32(a[:, 1], b[:, 1], (a[:, 0] * b[:, 0]).astype(np.float32)))


def cross32(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([fma32(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1]).astype(np.float32)),
                         fma32(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2]).astype(np.float32)),
                         fma32(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]).astype(np.float32))], 1)


def pack_records(records):
    """The 48-byte leaf-ordered records (n, 12) float32 -- A = (data1, meta), B = (data2, index), C = (data3, 0) -- and
    D (n, 4).  meta = category | material << 2 | emission << 4 | reflectance << 18.  A patch carries its unit normal
    and |e1|^2 in D and |e2|^2 in C.w; a sphere carries (r, r^2, 0) in B."""
    n = len(records)
    cat, d1, d2, d3, d4 = (records[k] for k in ("category", "data1", "data2", "data3", "data4"))
    prim, D = np.zeros((n, 12), np.float32), np.zeros((n, 4), np.float32)
    meta = (cat & 3) | ((d4[:, 2] & 3) << 2) | ((d4[:, 0] & 0x3FFF) << 4) | ((d4[:, 1] & 0x3FFF) << 18)
    prim[:, 0:3], prim[:, 4:7], prim[:, 8:11] = d1, d2, d3
    prim.view(np.uint32)[:, 3] = meta
    prim.view(np.uint32)[:, 7] = d4[:, 3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pt = cat == 0
        if pt.any():
            c = cross32(d2[pt], d3[pt])
            D[pt, 0:3] = c / np.sqrt(dot32(c, c))[:, None]
            D[pt, 3] = dot32(d2[pt], d2[pt])
            prim[pt, 11] = dot32(d3[pt], d3[pt])
        sp = cat == 1
        r = d2[sp, 0]
        prim[sp, 4], prim[sp, 5], prim[sp, 6] = r, (r * r).astype(np.float32), 0
    return prim, D


# ------------------------------------------------------------------ references and trees
def leaf_ref(first, count=1):
    return ~((int(first) << 3) | (int(count) - 1))


def leaf_range(ref):
    """(first slot, count) of leaf references (arrays or scalars)."""
    u = ~np.asarray(ref, np.int64)
    return u >> 3, (u & 7) + 1


class Tree2:
    """A BVH2 given by its child references (n2, 2) int32 and the root reference.  Construction checks the topology:
    every reference in range, every inner node reached exactly once, every slot in exactly one leaf, every node a
    contiguous range of slots."""

    def __init__(self, refs, root, nslot, max_leaf=MAX_LEAF):
        self.refs = refs = np.asarray(refs, np.int32).reshape(-1, 2)
        self.root, self.n2, self.nslot = int(root), len(refs), int(nslot)
        self.levels = []
        seen = np.zeros(self.n2, np.int64)
        cur = np.array([self.root] if self.root >= 0 else [], np.int64)
        leaves = [np.array([self.root], np.int64)] if self.root < 0 else []
        while len(cur):
            assert (cur < self.n2).all(), "a child reference past the node array"
            np.add.at(seen, cur, 1)
            assert (seen[cur] == 1).all(), "an inner node is reached twice"
            self.levels.append(cur)
            ch = refs[cur].reshape(-1).astype(np.int64)
            leaves.append(ch[ch < 0])
            cur = ch[ch >= 0]
            assert len(self.levels) <= 64, "deeper than any tree the builders make"
        assert (seen == 1).all(), f"{int((seen == 0).sum())} inner nodes are not reached from the root"
        self.leaves = np.concatenate(leaves) if leaves else np.zeros(0, np.int64)
        first, count = leaf_range(self.leaves)
        assert ((count >= 1) & (count <= max_leaf)).all(), f"leaf counts {np.unique(count)} outside 1..{max_leaf}"
        assert (first >= 0).all() and (first + count <= self.nslot).all(), "a leaf past the primitive array"
        cover = np.zeros(self.nslot + 1, np.int64)
        np.add.at(cover, first, 1)
        np.add.at(cover, first + count, -1)
        assert (np.cumsum(cover)[: self.nslot] == 1).all(), "a slot is in no leaf or in two"
        # the range of slots below every node, bottom-up
        self.first, self.count = np.zeros(max(self.n2, 1), np.int64), np.zeros(max(self.n2, 1), np.int64)
        for ids in reversed(self.levels):
            f, c = self.child_range(refs[ids])
            assert (np.minimum(f[:, 0], f[:, 1]) + c.sum(1) == np.maximum(f[:, 0] + c[:, 0], f[:, 1] + c[:, 1])).all(), "not a contiguous range"
            self.first[ids], self.count[ids] = f.min(1), c.sum(1)
        self.depth = len(self.levels)                             # inner levels (= the deepest leaf, the root at 0)

    def child_range(self, ref):
        ref = np.asarray(ref, np.int64)
        lf, lc = leaf_range(np.minimum(ref, -1))
        inner = np.maximum(ref, 0)
        return np.where(ref < 0, lf, self.first[inner]), np.where(ref < 0, lc, self.count[inner])

    def range_of(self, ref):
        f, c = self.child_range(np.asarray([ref]))
        return int(f[0]), int(c[0])

    def boxes(self, slot_lo, slot_hi):
        """The child boxes (n2, 2, 2, 3) float32 [child][lo | hi][axis]: the union of the slots' boxes below each child."""
        out = np.zeros((self.n2, 2, 2, 3), np.float32)
        for ids in reversed(self.levels):
            for c in range(2):
                ref = self.refs[ids, c].astype(np.int64)
                first, count = leaf_range(np.minimum(ref, -1))
                first = np.where(ref < 0, first, 0)
                lo, hi = slot_lo[first].copy(), slot_hi[first].copy()
                for k in range(1, 8):
                    m = (ref < 0) & (k < count)
                    if not m.any():
                        break
                    s = np.where(m, first + k, first)
                    lo, hi = np.minimum(lo, slot_lo[s]), np.maximum(hi, slot_hi[s])
                inner = np.maximum(ref, 0)
                nlo, nhi = np.minimum(out[inner, 0, 0], out[inner, 1, 0]), np.maximum(out[inner, 0, 1], out[inner, 1, 1])
                out[ids, c, 0] = np.where((ref < 0)[:, None], lo, nlo)
                out[ids, c, 1] = np.where((ref < 0)[:, None], hi, nhi)
        return out


def nodes2_split(nodes2):
    """A read-back BVH2 node array (n2, 16) float32 -> (boxes (n2, 2, 2, 3) float32, refs (n2, 2) int32)."""
    nodes2 = np.ascontiguousarray(nodes2, np.float32).reshape(-1, 16)
    return nodes2[:, :12].reshape(-1, 2, 2, 3).copy(), nodes2[:, 12:14].copy().view(np.int32)


# ------------------------------------------------------------------ LBVH
def _expand10(v):
    v = v.astype(np.uint64) & 0x3FF
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_keys(lo, hi):
    """The 62-bit keys of primitive boxes: the 30-bit Morton code of the box centre in the box of the finite centres
    (10 bits per axis, x highest), the primitive's index below it."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = (F(0.5) * lo + F(0.5) * hi).astype(np.float32)
        ok = ((c > F(-1.0e30)) & (c < F(1.0e30))).all(1)
        q = []
        for a in range(3):
            l, h = (c[ok, a].min(), c[ok, a].max()) if ok.any() else (F(0), F(1))
            sc = F(F(1024.0) / np.maximum(F(h - l), F(1.0e-20)))
            f = ((c[:, a] - l) * sc).astype(np.float32)
            q.append(np.floor(np.where(f > 0, np.where(f < F(1023.0), f, F(1023.0)), F(0))).astype(np.uint64))   # (a NaN lands in cell 0)
    m = (_expand10(q[0]) << np.uint64(2)) | (_expand10(q[1]) << np.uint64(1)) | _expand10(q[2])
    return (m << np.uint64(32)) | np.arange(len(lo), dtype=np.uint64)


def hierarchy(keys):
    """The binary radix tree over sorted unique keys: every range splits at its highest differing key bit.  Inner
    nodes are numbered as Karras' construction numbers them -- the node of a range sits at the end of the range that
    touches its sibling: the left child of a split after position g is node g, the right child node g + 1, the root
    node 0.  Returns refs (n - 1, 2) int32."""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    assert n >= 2 and (keys[1:] > keys[:-1]).all()
    refs = np.zeros((n - 1, 2), np.int32)
    stack = [(0, 0, n - 1)]
    while stack:
        node, first, last = stack.pop()
        bit = (int(keys[first]) ^ int(keys[last])).bit_length() - 1
        border = ((int(keys[last]) >> bit) << bit)                # the smallest key of the range with that bit set
        g = int(np.searchsorted(keys[first:last + 1], np.uint64(border), "left")) + first - 1
        for c, (a, b, me) in enumerate(((first, g, g), (g + 1, last, g + 1))):
            if a == b:
                refs[node, c] = leaf_ref(a)
            else:
                refs[node, c] = me
                stack.append((me, a, b))
    return refs


def lbvh(records, pad):
    """(order: slot -> primitive index, refs of the hierarchy, Tree2, child boxes) of the LBVH of these records."""
    lo, hi, _ = prim_bounds(records, pad)
    keys = np.sort(morton_keys(lo, hi))
    order = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    refs = hierarchy(keys)
    t = Tree2(refs, 0, len(records), max_leaf=1)
    return order, refs, t, t.boxes(lo[order], hi[order])


# ------------------------------------------------------------------ collapse
def surface(lo, hi):
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)).astype(np.float32)
        return F(F(F(d[0] * d[1]) + F(d[1] * d[2])) + F(d[2] * d[0]))


def collapse(refs2, boxes2, root, width):
    """The wide tree of a BVH2, level by level from the root.  A wide node starts as the two children of the BVH2 node
    it stands for; while it has room, the inner child with the largest surface (float32, the first maximum on a tie) is
    replaced by its first child and its second child is appended.  Returns (nodes, depth): nodes[l] lists the wide
    nodes of level l as (BVH2 node, [BVH2 child reference per slot], [box (2, 3) per slot]); depth = inner levels."""
    if root < 0:
        return [], 0
    with np.errstate(invalid="ignore", over="ignore"):           # the surfaces of all child boxes at once, in float32
        d = (boxes2[:, :, 1] - boxes2[:, :, 0]).astype(np.float32)
        area = ((d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]).astype(np.float32) + d[..., 2] * d[..., 0]).astype(np.float32).tolist()
    refs = np.asarray(refs2).tolist()
    levels, cur = [], [int(root)]
    while cur:
        level, nxt = [], []
        for b in cur:
            ch = [(b, 0), (b, 1)]                                 # a child is (BVH2 node, which of its two children)
            while len(ch) < width:
                best, ba = -1, -1.0
                for i, (p, c) in enumerate(ch):
                    if refs[p][c] >= 0 and area[p][c] > ba:      # (a NaN surface is never the largest)
                        best, ba = i, area[p][c]
                if best < 0:
                    break
                o = refs[ch[best][0]][ch[best][1]]
                ch[best] = (o, 0)
                ch.append((o, 1))
            level.append((b, [refs[p][c] for p, c in ch], [boxes2[p, c] for p, c in ch]))
            nxt += [refs[p][c] for p, c in ch if refs[p][c] >= 0]
        levels.append(level)
        cur = nxt
    return levels, len(levels)


# ------------------------------------------------------------------ grid and quantisation
def grid(lo, hi):
    """(base (3,) float32, scale (3,) float32) of the 16-bit grid over boxes lo / hi (k, 3), or None where the rule
    refuses: a plane not inside +-1e30, or bounds farther from the origin than 16 extents."""
    glo, ghi = np.asarray(lo, np.float32).reshape(-1, 3).min(0), np.asarray(hi, np.float32).reshape(-1, 3).max(0)
    with np.errstate(invalid="ignore", over="ignore"):
        if not ((glo > F(-1.0e30)).all() and (ghi < F(1.0e30)).all()):
            return None
        ext = np.maximum((ghi - glo).astype(np.float32), F(1.0e-3))
        mag = np.maximum(np.abs(glo), np.abs(ghi))
        if (mag > F(16.0) * ext).any():
            return None
        return glo, (ext / F(65533.0)).astype(np.float32)


def quantize(lo, hi, base, scale):
    """(qlo, qhi) uint16 of box planes (..., 3): floor - 1 / ceil + 1 of (plane - base) / scale in float64, clamped."""
    b, s = np.asarray(base, np.float32).astype(np.float64), np.asarray(scale, np.float32).astype(np.float64)
    ql = np.floor((np.asarray(lo, np.float32).astype(np.float64) - b) / s) - 1
    qh = np.ceil((np.asarray(hi, np.float32).astype(np.float64) - b) / s) + 1
    return np.clip(ql, 0, 65535).astype(np.uint16), np.clip(qh, 0, 65535).astype(np.uint16)


Q_EMPTY = (65535, 0)              # lo, hi of an empty slot of a quantised node; its reference is 0
F_EMPTY = BIG                     # lo = hi of an empty slot of a float 4-wide node


def wide_split(nodes, width, quantised):
    """A read-back wide node array -> (lo, hi (n, width, 3): float32 or uint16 grid coordinates; refs (n, width) int32).
    Layouts of crt_bvh.h: planes lo.x lo.y lo.z hi.x hi.y hi.z, `width` children each, then the references."""
    if quantised:
        nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 4 * width)
        planes = nodes[:, :3 * width].copy().view(np.uint16).reshape(-1, 6, width)
        refs = nodes[:, 3 * width:4 * width].copy().view(np.int32)
    else:
        nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 32)
        planes = nodes[:, :24].reshape(-1, 6, 4)
        refs = nodes[:, 24:28].copy().view(np.int32)
    return planes[:, 0:3].transpose(0, 2, 1).copy(), planes[:, 3:6].transpose(0, 2, 1).copy(), refs
