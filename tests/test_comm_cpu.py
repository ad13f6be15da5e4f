"""CPU-only: crt_layout_rows -- the one definition of the multi-GPU row partition, which crt_comm_partition sizes its strips
by and k_assemble inverts -- against the restatement of tests/comm_ref.py, at every height 1..40 for every world size 1..9
and the bands where the arithmetic has edges (1, a band beyond H, bands that leave parts without rows)."""
import ctypes as C

import numpy as np
import pytest

import comm_ref

BANDS = (0, 1, 2, 3, 5, 8, 64)


def layout_rows(lib, H, band, world, part):
    n = C.c_uint32()
    assert lib.crt_layout_rows(H, band, world, part, C.byref(n), None) == 0
    rows = np.full(n.value + 1, 0xFFFFFFFF, np.uint32)          # (one past the end: a canary)
    m = C.c_uint32()
    assert lib.crt_layout_rows(H, band, world, part, C.byref(m), rows.ctypes.data) == 0
    assert m.value == n.value and rows[n.value] == 0xFFFFFFFF
    return rows[: n.value].astype(np.int64)


@pytest.mark.parametrize("band", BANDS)
def test_layout_rows_is_the_restatement(band):
    from computeraytracer_amd import _lib
    lib = _lib.load()
    for H in range(1, 41):
        for world in range(1, 10):
            own = comm_ref.owners(H, world, band)
            parts = [layout_rows(lib, H, band, world, p) for p in range(world)]
            for p, rows in enumerate(parts):
                # the owner and the local row of every y: local row k of part p is global row rows[k]
                assert [own[y] for y in rows] == [(p, k) for k in range(len(rows))], (H, world, band, p)
                assert np.array_equal(rows, comm_ref.rows_of(H, world, band, p)), (H, world, band, p)
            assert comm_ref.rows_max(H, world, band) == max(len(r) for r in parts), (H, world, band)
            # the parts tile 0 .. H-1 exactly once
            assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(H)), (H, world, band)


def test_assemble_puts_every_row_back():
    """The restatement's own frame: strips cut from a known frame by the library's row lists assemble to that frame, and
    the padding is never read."""
    from computeraytracer_amd import _lib
    lib = _lib.load()
    W = 3
    for H, world, band in [(1, 3, 0), (2, 4, 0), (5, 2, 64), (17, 3, 1), (13, 4, 5), (40, 9, 8), (37, 5, 0)]:
        frame = np.arange(H * W, dtype=np.uint32).reshape(H, W)
        rmax = comm_ref.rows_max(H, world, band)
        strips = []
        for p in range(world):
            rows = layout_rows(lib, H, band, world, p)
            s = np.full((max(rmax, 1), W), 0xDEADBEEF, np.uint32)
            s[: len(rows)] = frame[rows]
            strips.append(s)
        assert np.array_equal(comm_ref.assemble(W, H, world, band, strips), frame), (H, world, band)
