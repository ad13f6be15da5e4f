"""A numpy restatement of the clustered GPU build (CRT_ACCEL_PLOC, DESIGN.md 3 "GPU build, clustered"), written from the
definition -- not a translation of crt_ploc.hip.  Parallel locally-ordered clustering (Meister & Bittner, TVCG 2018) over
the Morton-sorted primitives of accel_ref: bounds, keys and their order are accel_ref's, everything from there on is here.

  start   cluster p = the leaf of sorted position p
  round   nn[i] = the j within `radius` places of i (j != i) that minimises (surface of the union box, i XOR j); the
          surface in float32, (dx dy + dy dz) + dz dx, a non-finite one counts as FLT_MAX.  i leads a merge iff
          nn[nn[i]] == i and i < nn[i]: cluster i becomes the new node (child 0 = old i, child 1 = old nn[i]), cluster
          nn[i] disappears, the others keep their order.  The k-th node made (over rounds, by ascending i within one) is
          node n - 2 - k: the root is node 0 and a child's id is greater than its parent's.
  slots   top-down: first[root] = 0, first[child 0] = first[node], first[child 1] = first[node] + count[child 0]; a leaf's
          slot is its first, order[slot] its primitive.

Everything is float32 where the product computes in float32; unions are min / max and exact."""
from __future__ import annotations

import numpy as np

import accel_ref as AR

F = np.float32
FLT_MAX = np.finfo(np.float32).max


def union_surface(lo_a, hi_a, lo_b, hi_b):
    """The cost of merging boxes a and b (arrays (k, 3) float32): the union's surface in float32, FLT_MAX if not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.maximum(hi_a, hi_b) - np.minimum(lo_a, lo_b)).astype(np.float32)
        a = ((d[:, 0] * d[:, 1]).astype(np.float32) + (d[:, 1] * d[:, 2]).astype(np.float32)).astype(np.float32)
        a = (a + (d[:, 2] * d[:, 0]).astype(np.float32)).astype(np.float32)
    return np.where(np.isfinite(a), a, FLT_MAX).astype(np.float32)


def nearest(lo, hi, radius):
    """nn (m,) of clusters with boxes lo / hi (m, 3): the minimum of (cost, i XOR j) over 0 < |i - j| <= radius."""
    m = len(lo)
    idx = np.arange(m, dtype=np.int64)
    best_c = np.full(m, np.inf, np.float64)
    best_x = np.full(m, np.iinfo(np.int64).max, np.int64)
    nn = np.full(m, -1, np.int64)
    for d in range(1, min(radius, m - 1) + 1):
        c = union_surface(lo[:-d], hi[:-d], lo[d:], hi[d:]).astype(np.float64)      # pairs (i, i + d)
        x = idx[:-d] ^ idx[d:]
        for me, other in ((slice(0, m - d), idx[d:]), (slice(d, m), idx[:-d])):
            better = (c < best_c[me]) | ((c == best_c[me]) & (x < best_x[me]))
            best_c[me] = np.where(better, c, best_c[me])
            best_x[me] = np.where(better, x, best_x[me])
            nn[me] = np.where(better, other, nn[me])
    return nn


def cluster(lo, hi, radius=8, max_rounds=1 << 30):
    """The hierarchy over boxes in sorted order: (refs (n - 1, 2) with leaves as ~position, boxes (n - 1, 2, 2, 3),
    count of each child (n - 1, 2), node id ranges per round [(first id, number)], height of the root)."""
    n = len(lo)
    assert n >= 2 and 1 <= radius
    clo, chi = np.asarray(lo, np.float32).copy(), np.asarray(hi, np.float32).copy()
    ref = ~np.arange(n, dtype=np.int64)
    cnt, height = np.ones(n, np.int64), np.zeros(n, np.int64)
    refs = np.zeros((n - 1, 2), np.int64)
    boxes = np.zeros((n - 1, 2, 2, 3), np.float32)
    ccount = np.zeros((n - 1, 2), np.int64)
    made, rounds = 0, []
    while len(ref) > 1:
        assert len(rounds) < max_rounds, "not finished within the rounds limit"
        m = len(ref)
        nn = nearest(clo, chi, radius)
        i = np.arange(m)
        mutual = nn[nn] == i
        lead = np.flatnonzero(mutual & (i < nn))
        assert len(lead) >= 1, "the smallest pair is always mutual"
        j = nn[lead]
        ids = n - 2 - (made + np.arange(len(lead)))
        refs[ids, 0], refs[ids, 1] = ref[lead], ref[j]
        boxes[ids, 0, 0], boxes[ids, 0, 1], boxes[ids, 1, 0], boxes[ids, 1, 1] = clo[lead], chi[lead], clo[j], chi[j]
        ccount[ids, 0], ccount[ids, 1] = cnt[lead], cnt[j]
        clo[lead], chi[lead] = np.minimum(clo[lead], clo[j]), np.maximum(chi[lead], chi[j])
        ref[lead], cnt[lead], height[lead] = ids, cnt[lead] + cnt[j], np.maximum(height[lead], height[j]) + 1
        rounds.append((int(ids[-1]), len(lead)))
        made += len(lead)
        keep = ~(mutual & (i > nn))
        clo, chi, ref, cnt, height = clo[keep], chi[keep], ref[keep], cnt[keep], height[keep]
    assert made == n - 1 and ref[0] == 0
    return refs, boxes, ccount, rounds, int(height[0])


def slots(refs, ccount, rounds, n):
    """The top-down slot pass: (final refs (n - 1, 2) int32 with leaves ~(slot << 3), slot of each sorted position)."""
    first = np.zeros(n - 1, np.int64)
    out = np.zeros((n - 1, 2), np.int32)
    slot_of_pos = np.full(n, -1, np.int64)
    for base, k in reversed(rounds):                              # parents are made in later rounds than their children
        ids = np.arange(base, base + k)
        for c in range(2):
            r = refs[ids, c]
            f = first[ids] + (ccount[ids, 0] if c else 0)
            inner = r >= 0
            first[r[inner]] = f[inner]
            slot_of_pos[~r[~inner]] = f[~inner]
            out[ids, c] = np.where(inner, r, ~(f << 3)).astype(np.int32)
    assert sorted(slot_of_pos.tolist()) == list(range(n))
    return out, slot_of_pos


def ploc(records, pad, radius=8):
    """(order: slot -> primitive index, refs, Tree2, child boxes, rounds) of the PLOC tree of these records."""
    lo, hi, _ = AR.prim_bounds(records, pad)
    keys = np.sort(AR.morton_keys(lo, hi))
    prim = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    n = len(records)
    refs0, boxes, ccount, rounds, height = cluster(lo[prim], hi[prim], radius)
    refs, slot_of_pos = slots(refs0, ccount, rounds, n)
    order = np.zeros(n, np.int64)
    order[slot_of_pos] = prim
    t = AR.Tree2(refs, 0, n, max_leaf=1)
    assert t.depth == height, (t.depth, height)
    return order, refs, t, boxes, len(rounds)


def sah_cost(tree, boxes):
    """Sum over inner nodes of surface(node) / surface(root), in float64 (node box = the union of its child boxes)."""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    d = np.maximum(b[:, 0, 1], b[:, 1, 1]) - np.minimum(b[:, 0, 0], b[:, 1, 0])
    a = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    return float(a.sum() / a[tree.root])
