"""Every walk of the project against float64 geometry (run with -m gpu on an MI355X): the rays of
test_geometry_truth_cpu.py -- six scenes x 13-15 classes x 2000 -- compared with geometry_truth.py directly, not with the
oracle, through

  crt_debug_intersect    under "none" (the loop over every primitive) and on the BVH2 of "bvh2", "lbvh" and "ploc"
  crt_debug_trace_rays   the wavefront traversal kernels: defaults (k_wf_trace2), wf_trace_form = 1, quantize = 0, wf_width = 8
  crt_debug_walk_rays    walk 0 ("finish": the quantised 4-wide walk of k_wf_finish)

Every clear ray must come back with the expected primitive (or as a miss) and |t - t*| <= mu_t; no tolerance on the
decision.  The clear shares are asserted first (the floors of the CPU file), and each run asserts which tree and which
kernel it took (accel_stats, crt_debug_read_accel's header and the hook's report), as the ray-parity tests do.  For the
closed meshes M1-M3 every run also counts the rays from inside that come back as a miss and asserts that each of them is
UNCLEAR by the reference.

Measured on one MI355X: see DESIGN.md 3 (test list) for this file's time next to the whole -m gpu suite's."""
import numpy as np
import pytest

import geometry_truth as G
import test_geometry_truth_cpu as CPU
import test_traversal_rays_gpu as T
from geometry_truth import MAXU

pytestmark = pytest.mark.gpu

SCENES = CPU.SCENES
BUILDER = {"bvh2": "sah-host", "lbvh": "lbvh-gpu", "ploc": "ploc-gpu"}
ROUTES = ([("intersect", b) for b in ("none", "bvh2", "lbvh", "ploc")] + [("trace", f) for f in T.FORMS] + [("walk", "finish")])


def run(r, b, hook, arg):
    """The batch's rays through one route: (t, index, what ran)."""
    sc = b.sc
    case = sc.case()
    r.upload(sc.packed())
    if hook == "intersect":
        r.build_accel(arg)
        A = r.debug_read_accel()
        if arg == "none":
            assert A["accel_mode"] == 0 and A["n2"] == 0, A["accel_mode"]
        else:
            st = r.accel_stats()
            assert A["accel_mode"] == 1 and st["builder"] == BUILDER[arg] and st["nodes"] == A["n2"] > 0 and A["stale"] == 0, (sc.name, arg, st)
        out = r.debug_intersect(b.o, b.d, b.ex)
        return out[:, 0].copy(), out[:, 7].view(np.uint32).copy(), f"crt_debug_intersect / {arg}"
    T.set_form(r, arg if hook == "trace" else "defaults")
    r.build_accel("bvh2")
    if hook == "trace":
        _, _, _, rep0 = r.debug_trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))
        T.assert_tree(r, rep0, case, sc.prims, "bvh2", arg, f"{sc.name} / {arg}")
        t, i, _, rep = r.debug_trace_rays(b.o, b.d, b.ex)
        assert rep == rep0
        return t, i, f"crt_debug_trace_rays / {arg} / {rep['kernel']}"
    A = r.debug_read_accel()
    wide = A["live4q"] == 1 and A["live8q"] == 0
    assert wide is bool(T.expected_tree(case, sc.prims, "bvh2", "defaults", r.accel_stats()["nodes"] == 0)[4]), (sc.name, A["live4q"], A["live8q"])
    t, i, _, flags, _, rep = r.debug_walk_rays(b.o, b.d, b.ex, walk=arg)
    walked, fell = (flags & 1) != 0, (flags & 2) != 0
    assert rep["wide"] is wide and (rep["walked_wide"], rep["fell_back"]) == (int(walked.sum()), int(fell.sum())), rep
    assert walked.all() if wide else not walked.any(), (sc.name, rep)
    assert 3 * A["depth4"] <= rep["stack_entries"] and not fell.any(), (sc.name, rep)
    return t, i, f"crt_debug_walk_rays / {arg} / {'traverse4q' if wide else 'traverse'}"


@pytest.mark.parametrize("route", ROUTES, ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("name", list(SCENES))
def test_every_walk_decides_every_clear_ray_as_geometry_does(renderer, name, route):
    b = G.batch(SCENES[name])
    CPU.assert_floors(b)                                        # before anything is compared
    try:
        t, i, what = run(renderer, b, *route)
    finally:
        T.set_form(renderer, "defaults")
    msg, rel, leaks = G.report(b, t, i, f"{name} / {what}")
    print(f"{name} / {what}: largest |t - t*| / (2^-24 s_t) {rel:.3f}" + (f"; leaks from inside: {CPU.fmt_leaks(leaks)}" if leaks else ""))
    assert msg is None, msg
    assert rel <= G.K
    assert bool(leaks) is b.sc.closed
    for c, (n, unclear, of) in leaks.items():
        assert n == unclear, f"{name} / {what} / {c}: {n} of {of} rays from inside leak, {n - unclear} of them CLEAR by the reference"
    # (a miss is a miss on every route: the index, not t, says so)
    assert ((i == MAXU) | (i < len(b.sc.prims))).all()
