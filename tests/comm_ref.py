"""The multi-GPU frame assembly restated in numpy (include/crt.h "Multi-GPU", crt_layout_rows): which part owns a row of the
frame, where the row lies in that part's strip, and the [H][W] frame the padded strips of all parts assemble to.  Written
from the rule alone -- one row at a time, no shared code with crt_comm.cpp or k_assemble:

    band > 0   row y belongs to part (y // band) % world and is that part's local row (y // band // world) * band + y % band;
    band = 0   the parts are contiguous strips of ceil(H / world) rows.
"""
import numpy as np


def owner(y, H, world, band):
    """(part, local row) of row y of an H-row frame."""
    assert 0 <= y < H and world >= 1 and band >= 0
    if band == 0:
        per = -(-H // world)
        return y // per, y % per
    b = y // band
    return b % world, (b // world) * band + y % band


def owners(H, world, band):
    """[(part, local row)] for y = 0 .. H-1."""
    return [owner(y, H, world, band) for y in range(H)]


def rows_of(H, world, band, part):
    """The rows of the frame that `part` owns, in its local order."""
    own = owners(H, world, band)
    ys = [y for y in range(H) if own[y][0] == part]
    return np.asarray(sorted(ys, key=lambda y: own[y][1]), np.int64)


def rows_max(H, world, band):
    """The height every strip is padded to: the most rows any part owns."""
    return max(len(rows_of(H, world, band, p)) for p in range(world))


def assemble(W, H, world, band, strips):
    """strips: one array per part, [rows >= its row count][W][...]; rows past the part's own are padding and never read.
    Returns the [H][W][...] frame."""
    assert len(strips) == world
    frame = np.zeros((H, W) + tuple(np.shape(strips[0])[2:]), np.asarray(strips[0]).dtype)
    for y, (part, local) in enumerate(owners(H, world, band)):
        frame[y] = np.asarray(strips[part])[local]
    return frame
