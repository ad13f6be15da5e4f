"""The clustered GPU build, crt_build_accel(CRT_ACCEL_PLOC) (run with -m gpu on an MI355X), held to what the other
builders are held to and to its own definition:

  1 rays       every case of traversal_cases.py x tree form: the wavefront kernels on the PLOC tree return the reference
               loop's (bits(t), index) / visibility for every ray, freshly built and after update_primitives + refit
  2 structure  the BVH2 on the device (references, node numbers, child boxes, leaf order, depth) == ploc_ref.ploc bit
               for bit; the 4-wide tree is the collapse rule's; the host route builds the same BVH2 as the device route
  3 image      Cornell under "ploc" == under "bvh2" bit for bit, a crop == the oracle
  4 quality    fewer boxes per ray than the LBVH on atrium250k
  5 rebuilds   refit of an 8-wide tree rebuilds with PLOC; the depth and rounds limits hand the build to the LBVH with a
               note; "ploc_radius" is checked and acts
  6 memory     a failed allocation anywhere in the build is CRT_ENOMEM and leaves no tree; the next build renders
  7 node       the same frame through host/main.js"""
import shutil
import subprocess

import numpy as np
import pytest

import accel_ref as AR
import ploc_ref as PR
import test_traversal_rays_gpu as T
import traversal_cases as TC
from conftest import ROOT, bits
from test_accel_structure_gpu import check_wide, same
from test_traversal_rays_gpu import brutes  # noqa: F401  (the fixture: two contexts for the reference loop)

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")

CASES = T.CASES
FORMS = T.FORMS
NO_RAYS = np.zeros((0, 3), np.float32)
_REF = {}


def restated(name, prims, pad, radius=8):
    """ploc_ref.ploc of a case's primitives at `pad`, made once."""
    key = (name, float(pad) if np.isfinite(pad) else str(pad), radius)
    if key not in _REF:
        if len(_REF) > 8:
            _REF.clear()
        order, refs, t, boxes, rounds = PR.ploc(prims, pad, radius)
        _REF[key] = dict(order=order, refs=refs, tree=t, boxes=boxes, rounds=rounds)
    return _REF[key]


def last_error(r):
    return (r._lib.crt_last_error(r._h) or b"").decode()


def expected_tree(case, prims, form, root_leaf):
    kernel, width, bpb, by, q = T.expected_tree(case, prims, "lbvh", form, root_leaf)
    return kernel, width, bpb, ("ploc-gpu" if by == "lbvh-gpu" else by), q


def assert_tree(r, rep, case, prims, form, what):
    st = r.accel_stats()
    kernel, width, bpb, by, _ = expected_tree(case, prims, form, st["nodes"] == 0)
    assert (st["width"], st["bytes_per_box"], st["builder"]) == (width, bpb, by), (what, st, last_error(r))
    assert rep["kernel"] == kernel and rep["width"] == (8 if width == 8 else 4), (what, rep)
    assert rep["lds_entries"] == (16 if kernel == "k_wf_trace2" else 32) and rep["capacity"] == rep["lds_entries"] + rep["overflow_levels"]
    assert (rep["width"] - 1) * rep["depth"] <= rep["capacity"], (what, rep)
    assert (rep["depth"] == 0) == (st["nodes"] == 0), (what, rep)


# ------------------------------------------------------------------ 1 rays
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_wavefront_kernels_on_the_ploc_tree_equal_the_reference_loop(renderer, brutes, orc, name, form):  # noqa: F811
    case = CASES[name]
    fresh, runs, edit, ed = T.states(name, brutes, orc)
    try:
        T.set_form(renderer, form)
        renderer.upload(fresh.ps).build_accel("ploc")
        what = f"{name} / ploc / {form} / fresh"
        _, _, _, rep0 = renderer.debug_trace_rays(NO_RAYS, NO_RAYS)
        assert_tree(renderer, rep0, case, case.prims, form, what)
        assert fresh.check(renderer, what) == rep0
        exp = expected_tree(case, case.prims, form, renderer.accel_stats()["nodes"] == 0)
        was8, wasq = exp[1] == 8, exp[4]
        for first, rec in runs:
            renderer.update_primitives(first, rec)
        rebuilt = renderer.refit_accel()
        what = f"{name} / ploc / {form} / refitted"
        assert rebuilt is (was8 or (wasq and not TC.quantisable(ed, case.eye))), what
        _, _, _, rep0 = renderer.debug_trace_rays(NO_RAYS, NO_RAYS)
        assert_tree(renderer, rep0, case, ed, form, what)
        edit.check(renderer, what)
    finally:
        T.set_form(renderer, "defaults")


# ------------------------------------------------------------------ 2 structure
def check_bvh2(A, name, prims, what, radius=8):
    """The read-back BVH2 of a fresh PLOC build against the restatement: returns (Tree2, child boxes)."""
    n = len(prims)
    assert (A["accel_mode"], A["nprim"], A["builder"], A["root"], A["n2"]) == (1, n, 2, 0, n - 1), what
    ref = restated(name, prims, A["tree_pad"], radius)
    boxes2, refs2 = AR.nodes2_split(A["nodes2"])
    order = A["prim"].view(np.uint32)[:, 7].astype(np.int64)
    assert np.array_equal(A["slot_of_index"][order], np.arange(n)), f"{what}: slot_of_index is not the inverse of the leaf order"
    assert np.array_equal(order, ref["order"]), f"{what}: the leaf order is not the slot pass's"
    assert np.array_equal(refs2, ref["refs"]), f"{what}: the hierarchy is not the restated one: first at {np.argwhere(refs2 != ref['refs'])[:1].tolist()}"
    assert same(boxes2, ref["boxes"]), f"{what}: a child box differs from the restated one"
    assert same(A["nodes2"][:, 14:16], np.zeros((n - 1, 2), np.float32)), f"{what}: the unused floats of a node record are not 0"
    assert A["depth2"] == ref["tree"].depth, (what, A["depth2"], ref["tree"].depth)
    want_prim, want_d = AR.pack_records(prims[order])
    nan_ok = np.isnan(want_d) & np.isnan(A["primD"])
    assert same(A["prim"], want_prim) and same(np.where(nan_ok, 0, A["primD"]), np.where(nan_ok, 0, want_d)), f"{what}: the leaf-ordered records"
    return AR.Tree2(refs2, 0, n, max_leaf=1), boxes2


STRUCT_CASES = {**{n: c for n, c in CASES.items() if len(c.prims) >= 2}, "chain_lbvh": TC.case_chain()}


@pytest.mark.parametrize("name", list(STRUCT_CASES))
def test_the_tree_on_the_device_is_the_restated_one(renderer, name):
    case = STRUCT_CASES[name]
    q = TC.quantisable(case.prims, case.eye)
    try:
        got = {}
        for form in ("defaults", "quantize=0", "wf_width=8"):
            T.set_form(renderer, form)
            renderer.upload(TC.packed(case)).build_accel("ploc")
            got[form] = A = renderer.debug_read_accel()
            what = f"{name} / ploc / {form}"
            assert A["device_route"] == int(q and form == "defaults"), (what, A["device_route"], last_error(renderer))
            if form == "defaults":
                t2, boxes2 = check_bvh2(A, name, case.prims, what)
                assert (A["live4"], A["live4q"]) == (int(not q), int(q)), what
                depth, _ = check_wide(A, t2, boxes2, 4, bool(q), AR.collapse(t2.refs, boxes2, 0, 4), what + " / 4-wide")
                assert A["depth4"] == A["wf_depth"] == depth, (what, A["depth4"], A["wf_depth"], depth)
            else:                                                 # the host route: the same bits
                assert A["builder"] == 2 and A["live8q"] == int(q and form == "wf_width=8"), what
                for k in ("nodes2", "prim", "primD", "slot_of_index"):
                    assert same(A[k], got["defaults"][k]), f"{what}: {k} differs from the device route's"
                assert A["depth2"] == got["defaults"]["depth2"], what
    finally:
        T.set_form(renderer, "defaults")


def test_rays_through_the_chain_case(renderer, brutes, orc):  # noqa: F811
    """The deepest PLOC tree of the cases (40 levels restated): structure first, then rays."""
    case = TC.case_chain()
    renderer.upload(TC.packed(case)).build_accel("ploc")
    renderer.debug_trace_rays(NO_RAYS, NO_RAYS)
    A = renderer.debug_read_accel()
    assert A["builder"] == 2 and A["depth2"] >= 30, (A["builder"], A["depth2"], last_error(renderer))
    assert A["overflow_allocated"] + A["wf_stack_lds"] >= A["wf_stack_need"] == 3 * A["wf_depth"], "the walk below would leave the area: not run"
    st = T.State(case, None, brutes, orc, 40, n=600)
    rep = st.check(renderer, case.name + " / ploc")
    assert rep["kernel"] == "k_wf_trace2" and rep["depth"] == A["wf_depth"]


# ------------------------------------------------------------------ 3 image
def test_cornell_is_the_same_image_and_the_oracles(renderer, orc):
    from computeraytracer_amd import cornell
    ps = cornell(64, 48)
    out = {}
    for mode in ("bvh2", "ploc"):
        renderer.upload(ps).build_accel(mode).frame(4).sync()
        out[mode] = (renderer.read_accum().copy(), renderer.read_rgba8().copy())
    assert renderer.accel_stats()["builder"] == "ploc-gpu"
    assert np.array_equal(bits(out["ploc"][0]), bits(out["bvh2"][0])) and np.array_equal(out["ploc"][1], out["bvh2"][1])
    x0, y0, x1, y1 = rect = (24, 16, 40, 32)
    acc_o, rgba_o, _ = orc.Scene.from_packed(ps).render(4, rect=rect)
    acc, rgba = out["ploc"]                                   # (the oracle returns the frame with the crop filled in)
    assert np.array_equal(bits(acc[y0:y1, x0:x1])[..., :3], bits(acc_o[y0:y1, x0:x1])[..., :3]) and np.array_equal(rgba[y0:y1, x0:x1], rgba_o[y0:y1, x0:x1])
    assert np.any(acc_o[y0:y1, x0:x1, :3] != 0)


# ------------------------------------------------------------------ 4 quality
def test_fewer_boxes_per_ray_than_the_lbvh(renderer):
    from computeraytracer_amd import scenes_synth
    renderer.upload(scenes_synth.atrium250k(160, 90))
    per_ray = {}
    try:
        for mode in ("bvh2", "lbvh", "ploc"):
            renderer.build_accel(mode)
            renderer.enable_counters(True).reset_counters()
            renderer.frame(1).sync()
            c = renderer.counters()
            per_ray[mode] = c["nodes"] / c["rays"]
            print(f"atrium250k 160 x 90, 1 spp, {mode}: {renderer.accel_stats()['builder']} depth {renderer.accel_stats()['max_depth']}, "
                  f"{per_ray[mode]:.2f} boxes per ray, {c['prims'] / c['rays']:.2f} primitives per ray")
            renderer.enable_counters(False)
        assert renderer.accel_stats()["builder"] == "ploc-gpu"
        assert per_ray["ploc"] < per_ray["lbvh"], per_ray
    finally:
        renderer.enable_counters(False)


# ------------------------------------------------------------------ 5 rebuilds and fallbacks
def test_rebuilds_limits_and_the_radius(renderer, brutes, orc):  # noqa: F811
    from computeraytracer_amd._lib import CrtError
    case = CASES["grid"]
    fresh, runs, edit, ed = T.states("grid", brutes, orc)
    ps = TC.packed(case)
    try:
        # an 8-wide tree is rebuilt by crt_refit_accel, with the builder that made it
        T.set_form(renderer, "wf_width=8")
        renderer.upload(ps).build_accel("ploc")
        first, rec = runs[0]
        renderer.update_primitives(first, rec)
        assert renderer.refit_accel() is True and renderer.accel_stats()["builder"] == "ploc-gpu"
        T.set_form(renderer, "defaults")
        # the limits: the same call builds the LBVH, says so, and the rays are right; the next build tries PLOC again
        depth = restated("grid", case.prims, TC.hit_pad(case.prims, case.eye))
        assert depth["tree"].depth > 4 and depth["rounds"] > 2
        for hook, value, default, word in (("debug_ploc_max_depth", 4, 62, "levels deep"), ("debug_ploc_max_rounds", 2, 256, "rounds")):
            renderer.set_option(hook, value)
            renderer.upload(ps).build_accel("ploc")
            note = last_error(renderer)
            assert renderer.accel_stats()["builder"] == "lbvh-gpu", hook
            assert "PLOC" in note and word in note and "LBVH" in note, note
            A = renderer.debug_read_accel()
            assert A["builder"] == 1 and A["device_route"] == 1 and np.array_equal(AR.nodes2_split(A["nodes2"])[1], AR.lbvh(case.prims, A["tree_pad"])[1])
            fresh.check(renderer, f"grid / {hook} = {value}")
            renderer.set_option(hook, default)
            renderer.build_accel("ploc")
            assert renderer.accel_stats()["builder"] == "ploc-gpu", hook
        for hook, bad in (("ploc_radius", 0), ("ploc_radius", 33), ("debug_ploc_max_depth", 0), ("debug_ploc_max_depth", 63), ("debug_ploc_max_rounds", 0)):
            with pytest.raises(CrtError) as e:
                renderer.set_option(hook, bad)
            assert e.value.code == -1, (hook, bad)
        for radius in (1, 32):
            renderer.set_option("ploc_radius", radius)
            for name in ("grid", "tiny9"):
                c = CASES[name]
                renderer.upload(TC.packed(c)).build_accel("ploc")
                check_bvh2(renderer.debug_read_accel(), name, c.prims, f"{name} / ploc_radius = {radius}", radius)
    finally:
        for hook, default in (("debug_ploc_max_depth", 62), ("debug_ploc_max_rounds", 256), ("ploc_radius", 8)):
            renderer.set_option(hook, default)
        T.set_form(renderer, "defaults")


# ------------------------------------------------------------------ 6 out of memory
@pytest.mark.parametrize("form", ["defaults", "wf_width=8"])
def test_a_failed_allocation_leaves_no_tree(form):
    """Every allocation of a PLOC build of `grid`, device route and host route, failed in turn."""
    from computeraytracer_amd import Renderer
    from computeraytracer_amd._lib import CrtError
    ps = TC.packed(CASES["grid"])
    r = Renderer(0)
    try:
        T.set_form(r, form)
        r.upload(ps).build_accel("ploc").frame(2).sync()
        want = (r.read_accum().copy(), r.read_rgba8().copy())
        failed = 0
        for k in range(1, 200):
            r.set_option("debug_fail_alloc", k)
            try:
                r.build_accel("ploc")
            except CrtError as e:
                assert e.code == -4, (k, str(e))
                r.set_option("debug_fail_alloc", 0)
                with pytest.raises(CrtError, match="crt_build_accel first") as e2:
                    r.frame(1)
                assert e2.value.code == -3
                failed += 1
                continue
            break
        r.set_option("debug_fail_alloc", 0)
        assert failed == k - 1 >= 20, (failed, k)                 # (the clusters, the scan, the keys ...: more than the context's own arrays)
        assert r.accel_stats()["builder"] == "ploc-gpu"
        r.build_accel("ploc").frame(2).sync()
        assert np.array_equal(bits(r.read_accum()), bits(want[0])) and np.array_equal(r.read_rgba8(), want[1])
    finally:
        r.set_option("debug_fail_alloc", 0)
        r.close()


# ------------------------------------------------------------------ 7 node
SCRIPT = r"""
const fs = require('fs');
const { Main } = require(process.argv[1] + '/host/main.js');
const r = Main({ width: 64, height: 48, accel: 'ploc' });
r.run(3);
fs.writeFileSync(process.argv[2] + '/accum.bin', Buffer.from(r.readAccum().buffer));
fs.writeFileSync(process.argv[2] + '/rgba8.bin', Buffer.from(r.readRgba8().buffer));
r.destroy();
"""


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_renders_the_same_frame(tmp_path, renderer):
    from computeraytracer_amd import cornell
    subprocess.run([NODE, "-e", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, check=True, cwd=ROOT)
    acc = np.frombuffer((tmp_path / "accum.bin").read_bytes(), np.float32).reshape(48, 64, 4)
    rgba = np.frombuffer((tmp_path / "rgba8.bin").read_bytes(), np.uint8).reshape(48, 64, 4)
    renderer.upload(cornell(64, 48)).build_accel("ploc").frame(3).sync()
    assert renderer.accel_stats()["builder"] == "ploc-gpu"
    assert np.array_equal(bits(acc), bits(renderer.read_accum())) and np.array_equal(rgba, renderer.read_rgba8())
