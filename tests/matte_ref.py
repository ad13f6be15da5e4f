"""The restatement of crt_render_mattes (include/crt.h "ID mattes"): the per-sample hit indices come from
the CPU oracle (aov_ref.camera_hits); the table, the overflow rule and the ranking are applied in plain Python, pixel by
pixel, sample by sample.  A helper module, not collected by pytest."""
import numpy as np

MISS = 0xFFFFFFFF                # camera_hits' "no hit", and the id of a rank without an entry
PLANES = ("ids", "counts", "hits", "overflow")
PRIMITIVE, OBJECT, MATERIAL = 0, 1, 2


def hit_ids(ps, index, source, table=None):
    """The id of every hit of index (th, tw, n) uint32 (MISS stays MISS): the array position, the id table's entry (None:
    the identity), or material << 24 | reflectance index of the hit primitive."""
    index = np.asarray(index, np.uint32)
    if source == PRIMITIVE:
        return index.copy()
    prims = np.asarray(ps.primitives)
    if source == OBJECT:
        lut = np.arange(len(prims), dtype=np.uint32) if table is None else np.asarray(table, np.uint32)
    elif source == MATERIAL:
        d4 = prims["data4"]
        lut = (d4[:, 2].astype(np.uint32) << np.uint32(24)) | d4[:, 1].astype(np.uint32)
    else:
        raise ValueError(source)
    hit = index != MISS
    out = np.full(index.shape, MISS, np.uint32)
    out[hit] = lut[index[hit]]
    return out


def pixel(ids, slots):
    """One pixel: ids = its samples' ids in sample order (MISS: the ray hit nothing).  Returns (entries in insertion
    order [(id, count)], entries ranked, hits, overflow)."""
    table, h, over = [], 0, 0
    for v in ids:
        v = int(v)
        if v == MISS:
            continue
        h += 1
        for e in table:
            if e[0] == v:
                e[1] += 1
                break
        else:
            if len(table) < slots:
                table.append([v, 1])
            else:
                over += 1
    inserted = [tuple(e) for e in table]
    ranked = sorted(inserted, key=lambda e: (-e[1], e[0]))       # count descending, equal counts by id ascending
    return inserted, ranked, h, over


def mattes(ids, slots, n=None):
    """The four planes from per-sample ids (th, tw, n_max): ids and counts (slots, th, tw), hits and overflow (th, tw), all
    uint32.  n (th, tw), if given, is how many of each pixel's samples count (the adaptive state)."""
    ids = np.asarray(ids, np.uint32)
    th, tw, _ = ids.shape
    out = dict(ids=np.full((slots, th, tw), MISS, np.uint32), counts=np.zeros((slots, th, tw), np.uint32),
               hits=np.zeros((th, tw), np.uint32), overflow=np.zeros((th, tw), np.uint32))
    for y in range(th):
        for x in range(tw):
            row = ids[y, x] if n is None else ids[y, x, :int(n[y, x])]
            _, ranked, h, over = pixel(row, slots)
            for r, (v, k) in enumerate(ranked):
                out["ids"][r, y, x], out["counts"][r, y, x] = v, k
            out["hits"][y, x], out["overflow"][y, x] = h, over
    return out


def distinct(ids):
    """Per pixel: how many different ids its samples hit."""
    ids = np.asarray(ids, np.uint32)
    out = np.zeros(ids.shape[:2], np.int64)
    for y in range(ids.shape[0]):
        for x in range(ids.shape[1]):
            v = ids[y, x]
            out[y, x] = len(np.unique(v[v != MISS]))
    return out


def tie_pixels(planes):
    """Pixels where two ranked entries hold the same count (the id decides their order)."""
    c = np.asarray(planes["counts"])
    return ((c[:-1] == c[1:]) & (c[1:] > 0)).any(axis=0) if len(c) > 1 else np.zeros(c.shape[1:], bool)


def reordered_pixels(ids, slots):
    """Pixels whose ranked order differs from their insertion order."""
    ids = np.asarray(ids, np.uint32)
    out = np.zeros(ids.shape[:2], bool)
    for y in range(ids.shape[0]):
        for x in range(ids.shape[1]):
            inserted, ranked, _, _ = pixel(ids[y, x], slots)
            out[y, x] = inserted != ranked
    return out


def check_invariant(planes):
    """Sum of counts + overflow = hits, and a rank has an id exactly where it has a count."""
    c = np.asarray(planes["counts"]).astype(np.uint64)
    assert np.array_equal(c.sum(axis=0) + planes["overflow"], np.asarray(planes["hits"]).astype(np.uint64))
    assert np.array_equal(np.asarray(planes["ids"]) == MISS, np.asarray(planes["counts"]) == 0)
    assert (c[:-1] >= c[1:]).all()


def assert_planes(got, want, what=""):
    """Exactly, plane by plane."""
    for p in PLANES:
        if p not in got:
            continue
        g, w = np.asarray(got[p]), np.asarray(want[p])
        assert g.shape == w.shape and g.dtype == w.dtype == np.uint32, (what, p, g.shape, w.shape, g.dtype)
        bad = g != w
        assert not bad.any(), f"{what} {p}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0].tolist()}"
