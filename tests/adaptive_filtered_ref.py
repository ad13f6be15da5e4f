"""numpy restatement of crt_trace_adaptive_filtered's tile error (include/crt.h "Adaptive sampling judged by the filtered
preview") in float32, operation for operation as k_as_select_var computes it, and the protocol by which
the rule is compared with crt_trace_adaptive's.  A helper module, not collected by pytest."""
import numpy as np

import adaptive_ref as aref

F = np.float32
INF = F(np.inf)

# The comparison of DESIGN.md 6k: 16 samples everywhere, then rounds of 16 for the active tiles, 128 at most; today's
# rule at threshold 0.15 against the new one at 0.02; truth = 4096 samples drawn from sample index 100 001 on.
FIRST, STEP, CAP = 16, 16, 128
TAU_RAW, TAU_FILTERED = 0.15, 0.02
TRUTH_SPP, TRUTH_FIRST = 4096, 100001
# MSE(new) / MSE(old) of the filtered image in display space, measured with the float64 restatements on oracle renders of
# the Cornell box 96 x 96 (tests/test_adaptive_filtered_cpu.py); the oracle is deterministic, so the margin of 0.05
# covers libm differences alone, as in DESIGN.md 6g and 6i.
RATIO_MEASURED = 0.748
RATIO_MARGIN = 0.05


def tile_errors_filtered(v_out, counts):
    """E' per 8x8 tile: sqrt of the maximum of v' over the tile's in-frame pixels (NaN -> +inf before the maximum, one
    float32 square root after it); +inf for a count below 2.  v_out: (th, tw), what crt_denoise_adaptive returns as
    var_out; counts: (tiles_y, tiles_x)."""
    v = np.asarray(v_out, F)
    counts = np.asarray(counts, np.uint32)
    th, tw = v.shape
    ty, tx = counts.shape
    assert ty == (th + 7) // 8 and tx == (tw + 7) // 8
    v = np.where(np.isnan(v), INF, v)
    pad = np.zeros((ty * 8, tx * 8), F)                      # (v' >= +0: 0 is neutral, as for the lanes outside the frame)
    pad[:th, :tw] = v
    m = pad.reshape(ty, 8, tx, 8).max(axis=(1, 3)).astype(F)
    with np.errstate(invalid="ignore"):
        E = np.sqrt(m).astype(F)
    return np.where(counts < 2, INF, E).astype(F)


def rounds(tile_error, shape, tau):
    """The protocol's rounds for one rule: tile_error(counts) -> E or E' per tile.  Returns the final counts."""
    counts = np.full(shape, FIRST, np.uint32)
    while True:
        act = aref.active(counts, tile_error(counts), FIRST, CAP, tau)
        if not act.any():
            return counts
        counts = counts + np.uint32(STEP) * act.astype(np.uint32)
