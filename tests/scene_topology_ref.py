"""numpy restatement of crt_remove_primitives / crt_append_primitives (include/crt.h "Scene edits"), written
record by record and without the package's own helpers: what the device array, the light list and a fresh upload's
buffers must be after an edit.  Records are 80-byte rows handled as bytes; data4.w is the little-endian uint32 at 76."""
import numpy as np

REC = 80
INDEX_AT = 76


def _rows(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, REC).copy()


def _index(rows):
    return rows[:, INDEX_AT:INDEX_AT + 4].copy().view("<u4").reshape(-1)


def _set_index(rows, values):
    rows[:, INDEX_AT:INDEX_AT + 4] = np.asarray(values, "<u4").reshape(-1, 1).view(np.uint8)


def concat(*parts):
    """80-byte records one after another, byte for byte (np.concatenate would repack the fields and drop the padding)."""
    return np.concatenate([_rows(p) for p in parts]).reshape(-1).view(np.asarray(parts[0]).dtype)


def valid(ranges, n, light_index=()):
    """What crt_remove_primitives accepts with lights == NULL: every range inside [0, n) (first + count taken exactly), no
    primitive named twice, a primitive left, and no light of `light_index` on a removed primitive."""
    hit = np.zeros(n, np.int64)
    for first, count in ranges:
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > n:
            return False
        hit[first:first + count] += 1
    if (hit > 1).any() or (n > 0 and hit.all() and hit.sum() > 0):
        return False
    return not any(int(i) < n and hit[int(i)] for i in light_index)


def remove(prims, ranges, lights=None):
    """(records, lights) after the ranges are removed: the survivors in their order, data4.w = new position, every
    other byte kept; a light's data4.w below the old count lowered by the primitives removed before it."""
    rows = _rows(prims)
    n = len(rows)
    gone = set()
    for first, count in ranges:
        gone.update(range(int(first), int(first) + int(count)))
    survivors = [i for i in range(n) if i not in gone]
    out = rows[survivors] if survivors else rows[:0]
    _set_index(out, np.arange(len(out)))
    res_l = None
    if lights is not None:
        res_l = _rows(lights)
        idx = _index(res_l).astype(np.int64)
        for k, i in enumerate(idx):
            if i < n:
                assert i not in gone, f"light {k} lies on removed primitive {i}"
                idx[k] = i - sum(1 for g in gone if g < i)
        _set_index(res_l, idx)
        res_l = res_l.reshape(-1).view(np.asarray(lights).dtype)
    return out.reshape(-1).view(np.asarray(prims).dtype), res_l


def append(prims, records):
    """The records with `records` after them, byte for byte (their data4.w must already be their positions)."""
    rows, new = _rows(prims), _rows(records)
    assert np.array_equal(_index(new), np.arange(len(rows), len(rows) + len(new))), "appended records are numbered by position"
    return np.concatenate([rows, new]).reshape(-1).view(np.asarray(prims).dtype)
