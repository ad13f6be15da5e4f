"""Ray-level parity of the SINGLE-RAY walks (run with -m gpu on an MI355X): caller-chosen rays go through the walks as
the product kernels call them (crt_debug_walk_rays) --

  walk "finish"   as k_wf_finish walks its stragglers' rays: traverse4q on the quantised 4-wide tree where that tree is
                  live and no 8-wide tree is, repeated with traverse() on the BVH2 when its stack would overflow; shadow
                  rays any-hit, primed with the light's own t and index
  walk "bvh2"     as the pipeline = 0 kernel walks: traverse() on the BVH2; a shadow ray tests the light's own primitive
                  itself, then walks any-hit

-- and must come back exactly as the reference's loop over every primitive gives them: (bits(t), index) per extension
ray, the visibility bit per shadow ray, and under "bvh2" the bits of the t_light the kernel computed.  No tolerance
anywhere.  The reference is test_traversal_rays_gpu.State (crt_debug_intersect under build_accel("none"), spot-checked
against the oracle), shared with that module; every fourth ray of its 2000 per class is walked here.

For every case of traversal_cases.py x builder (bvh2, lbvh, ploc) x form (defaults, quantize=0, wf_width=8) x state
(freshly built; after update_primitives + refit_accel) x walk.  Which walk ran is asserted from the hook's flags and
crt_debug_read_accel's header, so a silent BVH2 run cannot pass for coverage of traverse4q; where 3 x (4-wide levels)
fits the stack no ray may fall back, and on the chain case under the LBVH most must (floors: half of near_tmin, inside
and deep_centre, a quarter of the plain shadow rays -- half of what the restated first descent gives on the CPU,
test_traversal_cases_cpu.py).

Measured on one MI355X: see DESIGN.md 3 (test list) for this file's time next to the whole -m gpu suite's."""
import numpy as np
import pytest

import test_traversal_rays_gpu as T
import traversal_cases as TC
from conftest import bits
from test_traversal_rays_gpu import brutes  # noqa: F401  (the fixture: two contexts for the reference loop)

pytestmark = pytest.mark.gpu

CASES = T.CASES
FORMS = ("defaults", "quantize=0", "wf_width=8")
BUILDERS = ("bvh2", "lbvh", "ploc")
WALKS = ("finish", "bvh2")
K_STACK = 64                                                  # crt_device.h kStackDepth


def quarter(st):
    """Every fourth ray of a State, both parities of the position (the plain shadow class excludes a primitive on every
    second ray): 500 of each class of 2000, 250 of a tie class."""
    k = np.arange(len(st.o)) % 8
    return np.flatnonzero((k == 0) | (k == 5))


def check(st, r, walk, what, sel=None):
    """The rays `sel` of State `st` through the hook: parity with the reference loop, t_light, which walk ran.  Returns
    (flags, the selection, report)."""
    sel = np.arange(len(st.o)) if sel is None else sel
    sh = st.shadow[sel]
    t, i, vis, flags, t_l, rep = r.debug_walk_rays(st.o[sel], st.d[sel], st.ex[sel], sh, st.t_light[sel], st.light[sel], walk=walk)
    ext = sel[~sh]
    assert (ext < st.n_ext).all()
    bad = np.zeros(len(sel), bool)
    bad[~sh] = (i[~sh] != st.want_i[ext]) | (bits(t[~sh]) != bits(st.want_t[ext]))      # (a miss carries the loop's initial t_max on both sides)
    bad[sh] = vis[sh] != st.want_vis[sel][sh]
    lab = st.lab[sel]
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        g = int(sel[k])
        per = {st.names[c]: int(bad[lab == c].sum()) for c in np.unique(lab[bad])}
        got = f"visible {int(vis[k])}" if sh[k] else f"t {t[k]!r} ({T.hexbits(t[k])}) index {int(i[k])}"
        exp = (f"visible {int(st.want_vis[g])} (light {int(st.light[g])}, t_light {st.t_light[g]!r})" if sh[k] else
               f"t {st.want_t[g]!r} ({T.hexbits(st.want_t[g])}) index {int(st.want_i[g])}")
        pytest.fail(f"{what}: {int(bad.sum())} of {len(bad)} rays differ from the reference loop, by class {per}; first: ray {g} of class "
                    f"{st.names[lab[k]]}: o {st.o[g].tolist()} d {st.d[g].tolist()} exclude {int(st.ex[g])} flags {int(flags[k])}: "
                    f"kernel {got}, loop {exp}; {rep}")
    if walk == "bvh2":                                          # the kernel's own test of the light's primitive
        off = bits(t_l[sh]) != bits(st.t_light[sel][sh])
        assert not off.any(), (f"{what}: {int(off.sum())} shadow rays: the kernel's t_light differs from the reference loop's; first: "
                               f"{T.hexbits(t_l[sh][off][0])} for {T.hexbits(st.t_light[sel][sh][off][0])}")
        assert (t_l[~sh].view(np.uint32) == 0).all(), what
    else:
        assert (t_l.view(np.uint32) == 0).all(), what
    # which walk ran
    A = r.debug_read_accel()
    wide = A["live4q"] == 1 and A["live8q"] == 0
    assert rep["wide"] is wide and rep["stack_entries"] == K_STACK and (rep["depth4"], rep["depth2"]) == (A["depth4"], A["depth2"]), (what, rep)
    assert (flags <= 3).all(), what
    walked, fell = (flags & 1) != 0, (flags & 2) != 0
    assert (rep["walked_wide"], rep["fell_back"]) == (int(walked.sum()), int(fell.sum())), (what, rep)
    if walk == "finish" and wide:
        assert walked.all(), f"{what}: {int((~walked).sum())} rays did not walk the quantised 4-wide tree"
    else:
        assert not walked.any() and not fell.any(), f"{what}: {int(walked.sum())} rays report the 4-wide walk, {int(fell.sum())} the fallback"
    if 3 * A["depth4"] <= K_STACK:                              # a walk holds at most (width - 1) x levels entries
        assert not fell.any(), f"{what}: {int(fell.sum())} rays fell back on a tree of {A['depth4']} levels"
    return flags, sel, rep


def expect_wide(case, prims, builder, form, r):
    """The tree must be the one the combination stands for (test_traversal_rays_gpu.expected_tree): quantised and
    4-wide <=> k_wf_finish walks it."""
    _, width, _, _, q = T.expected_tree(case, prims, "lbvh" if builder == "ploc" else builder, form, r.accel_stats()["nodes"] == 0)
    A = r.debug_read_accel()
    assert (A["live4q"] == 1 and A["live8q"] == 0) is bool(q and width == 4), (case.name, builder, form, A["live4q"], A["live8q"])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(CASES))
def test_single_ray_walks_equal_the_reference_loop(renderer, brutes, orc, name, builder, form):  # noqa: F811
    case = CASES[name]
    fresh, runs, edit, ed = T.states(name, brutes, orc)
    try:
        T.set_form(renderer, form)
        renderer.upload(fresh.ps).build_accel(builder)
        expect_wide(case, case.prims, builder, form, renderer)
        for walk in WALKS:
            check(fresh, renderer, walk, f"{name} / {builder} / {form} / fresh / {walk}", quarter(fresh))
        for first, rec in runs:                                 # the refit sub-case: a third of the primitives moved and shrunk
            renderer.update_primitives(first, rec)
        renderer.refit_accel()
        expect_wide(case, ed, builder, form, renderer)
        for walk in WALKS:
            check(edit, renderer, walk, f"{name} / {builder} / {form} / refitted / {walk}", quarter(edit))
    finally:
        T.set_form(renderer, "defaults")


_CHAIN = {}


def chain_state(brutes, orc):  # noqa: F811
    if not _CHAIN:
        case = TC.case_chain()
        st = T.State(case, None, brutes, orc, TC.WALK_SEED, n=TC.WALK_N)
        rays = TC.state_rays(case, TC.WALK_N, TC.WALK_SEED)      # what the CPU side of the floors walks
        assert [c for c, _, _, _ in rays] == st.names
        assert np.array_equal(bits(np.concatenate([o for _, o, _, _ in rays])), bits(st.o))
        assert np.array_equal(bits(np.concatenate([d for _, _, d, _ in rays])), bits(st.d))
        _CHAIN["st"] = (case, st)
    return _CHAIN["st"]


@pytest.mark.parametrize("builder", BUILDERS)
def test_the_chain_case_takes_the_fallback(renderer, brutes, orc, builder):  # noqa: F811
    """38 four-wide levels under the LBVH: a walk of traverse4q can need 114 entries against 64, and the first descent of
    most rays from inside the boxes does (test_traversal_cases_cpu.py shows it on the restated tree).  Every ray still
    comes back as the reference loop's, and the rays that fell back are counted: half of the classes from inside the
    boxes and a quarter of the plain shadow rays at the least."""
    case, st = chain_state(brutes, orc)
    renderer.upload(st.ps).build_accel(builder)
    expect_wide(case, case.prims, builder, "defaults", renderer)
    what = f"chain_lbvh / {builder} / defaults"
    flags, sel, rep = check(st, renderer, "finish", what + " / finish")
    check(st, renderer, "bvh2", what + " / bvh2")
    fell = (flags & 2) != 0
    per = {c: (int((st.lab == k).sum()), int(fell[st.lab == k].sum())) for k, c in enumerate(st.names)}
    print(f"fallback {what}: 4-wide levels {rep['depth4']}, BVH2 depth {rep['depth2']}, rays that fell back per class (of): "
          + ", ".join(f"{c} {f} ({n})" for c, (n, f) in per.items()))
    if builder == "lbvh":
        assert renderer.accel_stats()["builder"] == "lbvh-gpu" and rep["depth4"] == 30 + TC.CHAIN_J and 3 * rep["depth4"] > K_STACK, rep
        for c in ("near_tmin", "inside", "deep_centre"):
            assert per[c][0] == TC.WALK_N and 2 * per[c][1] >= per[c][0], (c, per[c])
        sh = per[f"shadow[light {case.lights[0]}]"]
        assert sh[0] == TC.WALK_N and 4 * sh[1] >= sh[0], sh


@pytest.mark.parametrize("builder", BUILDERS)
def test_a_larger_pad_through_set_camera_requantises_the_tree(renderer, brutes, orc, builder):  # noqa: F811
    """crt_set_camera with a farther eye grows hit_pad: the 4-wide tree is refitted and re-quantised inline, and
    k_wf_finish's walk reads the new grid."""
    case = CASES["grid"]
    ps = TC.packed(case)
    cam = ps.camera.copy()
    cam[0:3] = case.eye * np.float32(6)
    far = TC.Case("grid", case.prims, lights=case.lights, tie_lights=case.tie_lights, eye=cam[0:3].copy())
    st = T.State(far, None, brutes, orc, 30, n=TC.WALK_N)        # the reference: uploaded with the far camera
    try:
        for form in ("defaults", "quantize=0"):
            T.set_form(renderer, form)
            renderer.upload(ps).build_accel(builder)
            pad0 = renderer.debug_hit_pad
            q0 = renderer.debug_read_accel()["qscale"].copy()
            renderer.set_camera(cam)
            assert renderer.debug_hit_pad == TC.hit_pad(case.prims, cam[0:3]) > pad0
            expect_wide(far, case.prims, builder, form, renderer)
            if form == "defaults":
                assert (renderer.debug_read_accel()["qscale"] > q0).all(), "the grid did not grow with the pad"
            check(st, renderer, "finish", f"grid / {builder} / {form} / set_camera / finish")
    finally:
        T.set_form(renderer, "defaults")


def test_hook_refusals(renderer):
    from computeraytracer_amd._lib import CrtError
    case = CASES["tiny5"]
    o, d = np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32)
    renderer.upload(TC.packed(case)).build_accel("none")
    with pytest.raises(CrtError, match="CRT_ACCEL_NONE") as e:
        renderer.debug_walk_rays(o, d)
    assert e.value.code == -3
    renderer.build_accel("bvh2")
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 2):
            for arr in (0, 1):
                oo, dd = o.copy(), d.copy()
                (oo, dd)[arr][1, col] = bad
                with pytest.raises(CrtError, match="not finite") as e:
                    renderer.debug_walk_rays(oo, dd)
                assert e.value.code == -1
    with pytest.raises(CrtError, match="light index") as e:      # a shadow ray towards a primitive that does not exist
        renderer.debug_walk_rays(o, d, None, np.ones(3, bool), np.ones(3, np.float32), np.full(3, 5, np.uint32))
    assert e.value.code == -1
    with pytest.raises(CrtError, match="t_light") as e:
        renderer.debug_walk_rays(o, d, None, np.ones(3, bool), np.full(3, np.inf, np.float32), np.zeros(3, np.uint32))
    assert e.value.code == -1
    rays, out = np.zeros((1, 12), np.float32), np.zeros((1, 4), np.uint32)
    rays[0, 3:6] = 1.0
    rays.view(np.uint32)[0, 7] = 2                              # a bad kind
    assert renderer._lib.crt_debug_walk_rays(renderer._h, 0, rays.ctypes.data, 1, out.ctypes.data, None) == -1
    assert b"kind" in renderer._lib.crt_last_error(renderer._h)
    rays.view(np.uint32)[0, 7] = 0
    assert renderer._lib.crt_debug_walk_rays(renderer._h, 2, rays.ctypes.data, 1, out.ctypes.data, None) == -1      # a bad walk
    assert b"walk" in renderer._lib.crt_last_error(renderer._h)
    renderer.update_primitives(0, case.prims[:1])
    with pytest.raises(CrtError, match="crt_refit_accel") as e:
        renderer.debug_walk_rays(o, d)
    assert e.value.code == -3
    renderer.refit_accel()
    from computeraytracer_amd import Renderer
    with Renderer(0) as r:                                       # no scene; a scene without a tree
        for _ in range(2):
            with pytest.raises(CrtError, match="scene \\+ accel required") as e:
                r.debug_walk_rays(o, d)
            assert e.value.code == -3
            r.upload(TC.packed(case))
    # it works under either pipeline (the trees are the same), and an empty call reports the tree
    want = renderer.debug_walk_rays(o, d)
    assert len(want[0]) == 3 and want[5]["wide"] and want[5]["walked_wide"] == 3 and want[5]["fell_back"] == 0
    empty = renderer.debug_walk_rays(np.zeros((0, 3)), np.zeros((0, 3)))[5]
    assert empty == {**want[5], "walked_wide": 0}
    try:
        renderer.set_option("pipeline", 0)
        got = renderer.debug_walk_rays(o, d)
        assert all(np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(got[:5], want[:5])) and got[5] == want[5]
    finally:
        renderer.set_option("pipeline", 1)
