"""numpy float32 restatement of adaptive sampling's noise estimate and tile rule (include/crt.h "Adaptive sampling",
DESIGN.md 6c), operation for operation as crt_adaptive.hip / k_wf_resolve_as / k_trace<ADAPT> compute them.

exp_ is the device's exp (crt_math.h), taken from the oracle's math_eval, which is pinned bit for bit to the device."""
import numpy as np

F = np.float32
INF = F(np.inf)


def max_(a, b):
    """crt_math.h max_: (a < b) ? b : a  (a NaN `a` stays NaN)."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    return np.where(a < b, b, a).astype(F)


def accumulate(ys, S=None, Q=None):
    """Sample-ordered sums over ys (k, ...) of the per-sample Y: S += y and Q = Q + y*y, each one f32 operation."""
    ys = np.asarray(ys, F)
    S = np.zeros(ys.shape[1:], F) if S is None else np.array(S, F)
    Q = np.zeros(ys.shape[1:], F) if Q is None else np.array(Q, F)
    with np.errstate(over="ignore", invalid="ignore"):
        for y in ys:
            S = (S + y).astype(F)
            Q = (Q + (y * y).astype(F)).astype(F)
    return S, Q


def pixel_error(S, Q, n, exp_):
    """e per pixel for a count n >= 2 (broadcast): m = S/n, v = max_(Q/n - m*m, 0), se = sqrt(v/(n-1)),
    e = (2.2 * exp_(-2.2 * max_(m, 0))) * se.  exp_: elementwise float32 -> float32."""
    S = np.asarray(S, F)
    Q = np.asarray(Q, F)
    n = np.asarray(n, np.uint32)
    nf = n.astype(F)
    with np.errstate(all="ignore"):
        m = (S / nf).astype(F)
        v = ((Q / nf).astype(F) - (m * m).astype(F)).astype(F)
        v = max_(v, F(0))
        se = np.sqrt((v / (n - 1).astype(F)).astype(F)).astype(F)
        arg = (F(-2.2) * max_(m, F(0))).astype(F)
        slope = (F(2.2) * np.asarray(exp_(arg.ravel()), F).reshape(arg.shape)).astype(F)
        return (slope * se).astype(F)


def tile_errors(S, Q, counts, exp_):
    """E per 8x8 tile: max of e over the tile's in-frame pixels, NaN -> +inf; +inf for a count below 2.
    S, Q: (th, tw); counts: (tiles_y, tiles_x)."""
    S = np.asarray(S, F)
    Q = np.asarray(Q, F)
    counts = np.asarray(counts, np.uint32)
    th, tw = S.shape
    ty, tx = counts.shape
    assert ty == (th + 7) // 8 and tx == (tw + 7) // 8
    n_pix = np.repeat(np.repeat(counts, 8, 0), 8, 1)[:th, :tw]
    e = pixel_error(S, Q, np.maximum(n_pix, 2), exp_)
    e = np.where(np.isnan(e), INF, e)
    pad = np.full((ty * 8, tx * 8), -INF, F)
    pad[:th, :tw] = e
    E = pad.reshape(ty, 8, tx, 8).max(axis=(1, 3)).astype(F)
    return np.where(counts < 2, INF, E).astype(F)


def active(counts, E, min_samples, max_samples, threshold):
    """The rule: (max == 0 || n < max) && (n < min || !(E <= threshold))."""
    counts = np.asarray(counts, np.uint32)
    E = np.asarray(E, F)
    below_max = np.ones(counts.shape, bool) if max_samples == 0 else counts < max_samples
    with np.errstate(invalid="ignore"):
        return below_max & ((counts < min_samples) | ~(E <= F(threshold)))


def pixel_counts(counts, th, tw):
    """The tile counts spread over the tile's pixels: (th, tw)."""
    return np.repeat(np.repeat(np.asarray(counts, np.uint32), 8, 0), 8, 1)[:th, :tw]
