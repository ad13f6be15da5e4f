"""Ray-level parity of the WAVEFRONT traversal kernels (run with -m gpu on an MI355X): caller-chosen rays go through
the kernel frame() launches (crt_debug_trace_rays: k_wf_trace2, k_wf_trace<,0|1|2>, with their chunking, shard scan,
refill, any-hit shadow walk and stack overflow area) and must come back exactly as the reference's loop over every
primitive gives them -- (bits(t), index) per extension ray, the visibility bit per shadow ray, no tolerance anywhere.

  hook  ==  crt_debug_intersect under build_accel("none") (the loop on the GPU)   every ray
  that  ==  the oracle's loop                                                      a spot sample per case and state

for every case of traversal_cases.py x builder (bvh2, lbvh) x tree form (defaults, wf_trace_form=1, quantize=0,
wf_width=8) x state (freshly built; after update_primitives + refit_accel of a third of the primitives).  Each
combination asserts which tree and kernel it ran on (accel_stats and the hook's report), so a silent fallback cannot
pass for coverage.  What makes the rays worth tracing is asserted on the reference side, in test_traversal_cases_cpu.py.

Measured on one MI355X: see DESIGN.md 3 (test list) for this file's time next to the whole -m gpu suite's."""
import numpy as np
import pytest

import traversal_cases as TC
from conftest import bits
from traversal_cases import MAXU

pytestmark = pytest.mark.gpu

N = 2000                                                      # rays per class
FORMS = {"defaults": {}, "wf_trace_form=1": {"wf_trace_form": 1}, "quantize=0": {"quantize": 0}, "wf_width=8": {"wf_width": 8}}
DEFAULTS = {"wf_trace_form": 2, "quantize": 1, "wf_width": 4}
CASES = {c.name: c for c in TC.all_cases()}


def hexbits(x):
    return f"0x{int(np.float32(x).view(np.uint32)):08x}"


@pytest.fixture(scope="module")
def brutes():
    """Two more contexts for the reference loop: one holds the case, one a shadow ray's light alone."""
    from computeraytracer_amd import Renderer
    a, b = Renderer(0), Renderer(0)
    yield a, b
    a.close()
    b.close()


def gpu_reference(r, ps):
    r.upload(ps).build_accel("none")

    def ref(o, d, ex):
        out = r.debug_intersect(o, d, ex)
        return out[:, 0].copy(), out[:, 7].view(np.uint32).copy()
    return ref


class State:
    """The rays of one case in one state (fresh / edited) and what the reference loop gives them."""

    def __init__(self, case, prims, brutes, orc, seed, n=N):
        a, b = brutes
        self.ps = TC.packed(case, prims)
        self.prims = self.ps.primitives
        ref = gpu_reference(a, self.ps)
        R = TC.Rays(case, prims, seed=seed)
        rng = np.random.default_rng(seed + 1)
        o, d, ex, lab, self.names = [], [], [], [], []
        for cname, co, cd, mode in R.classes(n):
            assert np.isfinite(co).all() and np.isfinite(cd).all() and (np.abs(co) <= R.M).all()
            o.append(co); d.append(cd); ex.append(TC.resolve_exclude(ref, rng, len(self.prims), co, cd, mode))
            lab.append(np.full(len(co), len(self.names))); self.names.append(cname)
        self.n_ext = sum(len(x) for x in o)
        sh_t, sh_l, sh_vis = [], [], []
        groups = [(L, "shadow", None) for L in case.lights] + [(L, f"shadow_tie_{k}", k) for L, k in case.tie_lights]
        for L, cname, kind in groups:
            od = R.shadow_tie(L, n // 2) if kind else R.shadow(L, n)
            co, cd = od if od is not None else R.shadow(L, n // 2)
            cex = np.full(len(co), MAXU, np.uint32) if kind else TC.shadow_excludes(case, L, len(co), len(self.prims), rng)
            t_l, own, vis, tie_hi, tie_lo = TC.shadow_expect(ref, gpu_reference(b, TC.single(case, L, prims)), L, co, cd, cex)
            assert own.all(), f"{case.name}: {int((~own).sum())} shadow rays towards primitive {L} miss it in the reference loop"
            if kind and prims is None:
                assert (tie_hi if kind == "higher" else tie_lo).sum() >= 100, (case.name, L, kind)
            o.append(co); d.append(cd); ex.append(cex)
            lab.append(np.full(len(co), len(self.names))); self.names.append(f"{cname}[light {L}]")
            sh_t.append(t_l); sh_l.append(np.full(len(co), L, np.uint32)); sh_vis.append(vis)
        self.o, self.d, self.ex, self.lab = (np.concatenate(x) for x in (o, d, ex, lab))
        n_all = len(self.o)
        self.shadow = np.arange(n_all) >= self.n_ext
        self.t_light = np.zeros(n_all, np.float32)
        self.light = np.zeros(n_all, np.uint32)
        self.want_vis = np.zeros(n_all, np.uint32)
        if n_all > self.n_ext:
            self.t_light[self.n_ext:] = np.concatenate(sh_t)
            self.light[self.n_ext:] = np.concatenate(sh_l)
            self.want_vis[self.n_ext:] = np.concatenate(sh_vis)
        self.want_t, self.want_i = ref(self.o[:self.n_ext], self.d[:self.n_ext], self.ex[:self.n_ext])
        assert not np.isnan(self.want_t[self.want_i != MAXU]).any()
        # the loop on the GPU is the oracle's (spot sample, as the existing ray tests do)
        sc = orc.Scene.from_packed(self.ps)
        for k in np.linspace(0, self.n_ext - 1, 150).astype(int):
            of, ou = sc.intersect(self.o[k], self.d[k], int(self.ex[k]))
            assert int(self.want_i[k]) == (int(ou[1]) if ou[0] else MAXU), (case.name, self.names[self.lab[k]], k)
            if ou[0]:
                assert hexbits(self.want_t[k]) == hexbits(of[0]), (case.name, self.names[self.lab[k]], k)

    def check(self, r, what):
        t, i, vis, rep = r.debug_trace_rays(self.o, self.d, self.ex, self.shadow, self.t_light, self.light)
        e = self.n_ext
        bad = np.zeros(len(self.o), bool)
        bad[:e] = (i[:e] != self.want_i) | (bits(t[:e]) != bits(self.want_t))     # (a miss carries the loop's initial t_max on both sides)
        bad[e:] = vis[e:] != self.want_vis[e:]
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            per = {self.names[c]: int(bad[self.lab == c].sum()) for c in np.unique(self.lab[bad])}
            got = f"visible {int(vis[k])}" if k >= e else f"t {t[k]!r} ({hexbits(t[k])}) index {int(i[k])}"
            exp = (f"visible {int(self.want_vis[k])} (light {int(self.light[k])}, t_light {self.t_light[k]!r})" if k >= e else
                   f"t {self.want_t[k]!r} ({hexbits(self.want_t[k])}) index {int(self.want_i[k])}")
            pytest.fail(f"{what}: {int(bad.sum())} of {len(bad)} rays differ from the reference loop, by class {per}; first: ray {k} of class "
                        f"{self.names[self.lab[k]]}: o {self.o[k].tolist()} d {self.d[k].tolist()} exclude {int(self.ex[k])}: "
                        f"kernel {got}, loop {exp}; {rep}")
        return rep


_STATES = {}


def states(name, brutes, orc):
    """(fresh state, update runs, edited state) of a case, made once."""
    if name not in _STATES:
        case = CASES[name]
        runs, ed = TC.edited(case, np.random.default_rng(77))
        _STATES.clear()                                         # (one case at a time: the parametrisation goes case by case)
        _STATES[name] = (State(case, None, brutes, orc, 10), runs, State(case, ed, brutes, orc, 20), ed)
    return _STATES[name]


def expected_tree(case, prims, builder, form, root_leaf):
    """What crt_build_accel makes of these primitives: (kernel, accel_stats width, bytes per box, builder, quantised).
    root_leaf: the BVH2 has no inner node (accel_stats) -- the SAH builder's choice for up to four primitives, and
    every builder's for one."""
    n = len(prims)
    q = TC.quantisable(prims, case.eye) and form != "quantize=0" and n >= 2
    by = "lbvh-gpu" if builder == "lbvh" and n >= 2 else "sah-host"          # (both LBVH routes hand n < 2 to the host builder)
    if root_leaf:
        assert n == 1 or (n <= 4 and by == "sah-host"), (case.name, n, by)
        return "k_wf_trace<,0>", 2, 32, by, False                            # the root is a leaf: no wide node at all
    if not q:
        return "k_wf_trace<,0>", 4, 32, by, False
    if form == "wf_width=8":
        return "k_wf_trace<,2>", 8, 16, by, True
    return ("k_wf_trace<,1>" if form == "wf_trace_form=1" else "k_wf_trace2"), 4, 16, by, True


def assert_tree(r, rep, case, prims, builder, form, what):
    st = r.accel_stats()
    kernel, width, bpb, by, _ = expected_tree(case, prims, builder, form, st["nodes"] == 0)
    assert (st["width"], st["bytes_per_box"], st["builder"]) == (width, bpb, by), (what, st)
    assert rep["kernel"] == kernel and rep["width"] == (8 if width == 8 else 4), (what, rep)
    assert rep["lds_entries"] == (16 if kernel == "k_wf_trace2" else 32) and rep["capacity"] == rep["lds_entries"] + rep["overflow_levels"]
    assert (rep["width"] - 1) * rep["depth"] <= rep["capacity"], (what, rep)
    assert (rep["depth"] == 0) == (st["nodes"] == 0), (what, rep)


def set_form(r, form):
    for k, v in {**DEFAULTS, **FORMS[form]}.items():
        r.set_option(k, v)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("builder", ["bvh2", "lbvh"])
@pytest.mark.parametrize("name", list(CASES))
def test_wavefront_kernels_equal_the_reference_loop(renderer, brutes, orc, name, builder, form):
    case = CASES[name]
    fresh, runs, edit, ed = states(name, brutes, orc)
    try:
        set_form(renderer, form)
        renderer.upload(fresh.ps).build_accel(builder)
        what = f"{name} / {builder} / {form} / fresh"
        # (the hook reports the tree before any ray is traced: assert_tree's capacity check comes from a call without rays)
        _, _, _, rep0 = renderer.debug_trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))
        assert_tree(renderer, rep0, case, case.prims, builder, form, what)
        rep = fresh.check(renderer, what)
        assert rep == rep0
        # the refit sub-case: a third of the primitives moved and shrunk, the tree refitted in place
        exp = expected_tree(case, case.prims, builder, form, renderer.accel_stats()["nodes"] == 0)
        was8, wasq = exp[1] == 8, exp[4]
        for first, rec in runs:
            renderer.update_primitives(first, rec)
        rebuilt = renderer.refit_accel()
        what = f"{name} / {builder} / {form} / refitted"
        assert rebuilt is (was8 or (wasq and not TC.quantisable(ed, case.eye))), what     # 8-wide: the documented rebuild
        _, _, _, rep0 = renderer.debug_trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))
        assert_tree(renderer, rep0, case, ed, builder, form, what)
        edit.check(renderer, what)
    finally:
        set_form(renderer, "defaults")


@pytest.mark.parametrize("builder", ["bvh2", "lbvh"])
def test_a_larger_pad_through_set_camera_requantises_the_tree(renderer, brutes, orc, builder):
    """crt_set_camera with a farther eye grows hit_pad: the 4-wide tree is refitted and re-quantised inline."""
    case = CASES["grid"]
    ps = TC.packed(case)
    cam = ps.camera.copy()
    cam[0:3] = case.eye * np.float32(6)
    far = TC.Case("grid", case.prims, lights=case.lights, tie_lights=case.tie_lights, eye=cam[0:3].copy())
    st = State(far, None, brutes, orc, 30)                      # the reference: uploaded with the far camera
    try:
        for form in ("defaults", "wf_trace_form=1", "quantize=0"):
            set_form(renderer, form)
            renderer.upload(ps).build_accel(builder)
            pad0 = renderer.debug_hit_pad
            renderer.set_camera(cam)
            assert renderer.debug_hit_pad == TC.hit_pad(case.prims, cam[0:3]) > pad0
            rep = st.check(renderer, f"grid / {builder} / {form} / set_camera")
            assert_tree(renderer, rep, far, case.prims, builder, form, form)
    finally:
        set_form(renderer, "defaults")


STACKS = {}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("builder", ["bvh2", "lbvh"])
@pytest.mark.parametrize("name", ["baseline", "deep_lbvh"])
def test_counting_variant_and_stack_depths(renderer, brutes, orc, name, builder, form):
    """The counting kernels give the same rays the same answers and report the deepest stack a lane reached.  The deep
    LBVH must take the walk past the LDS entries of the kernel under test, into the overflow area, and stay inside it."""
    case = CASES[name]
    fresh = states(name, brutes, orc)[0]
    try:
        set_form(renderer, form)
        renderer.upload(fresh.ps).build_accel(builder)
        _, _, _, rep0 = renderer.debug_trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))
        assert_tree(renderer, rep0, case, case.prims, builder, form, name)      # (width - 1) x depth <= capacity, BEFORE tracing
        renderer.enable_counters(True)
        rep = fresh.check(renderer, f"{name} / {builder} / {form} / counting")
        st = renderer.accel_stats()
        STACKS[(name, builder, form)] = rep
        print(f"stack {name} {builder} {form}: builder {st['builder']} bvh2 depth {st['max_depth']} | {rep}")
        assert rep["counting"] and 0 < rep["deepest"] <= min(rep["capacity"], (rep["width"] - 1) * rep["depth"]), rep
        if name == "deep_lbvh" and builder == "lbvh":
            assert st["builder"] == "lbvh-gpu", st
            assert rep["deepest"] > rep["lds_entries"], f"the overflow area was not reached: {rep}"
    finally:
        renderer.enable_counters(False)
        set_form(renderer, "defaults")


def test_hook_refusals(renderer):
    from computeraytracer_amd._lib import CrtError
    case = CASES["tiny5"]
    o, d = np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32)
    renderer.upload(TC.packed(case)).build_accel("none")
    with pytest.raises(CrtError, match="no wavefront tree") as e:
        renderer.debug_trace_rays(o, d)
    assert e.value.code == -3
    renderer.build_accel("bvh2")
    try:
        renderer.set_option("pipeline", 0)
        with pytest.raises(CrtError, match="no wavefront tree") as e:
            renderer.debug_trace_rays(o, d)
        assert e.value.code == -3
    finally:
        renderer.set_option("pipeline", 1)
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 2):
            for arr in (0, 1):
                oo, dd = o.copy(), d.copy()
                (oo, dd)[arr][1, col] = bad
                with pytest.raises(CrtError, match="not finite") as e:
                    renderer.debug_trace_rays(oo, dd)
                assert e.value.code == -1
    with pytest.raises(CrtError, match="light index") as e:      # a shadow ray towards a primitive that does not exist
        renderer.debug_trace_rays(o, d, None, np.ones(3, bool), np.ones(3, np.float32), np.full(3, 5, np.uint32))
    assert e.value.code == -1
    renderer.update_primitives(0, case.prims[:1])
    with pytest.raises(CrtError, match="crt_refit_accel") as e:
        renderer.debug_trace_rays(o, d)
    assert e.value.code == -3
    renderer.refit_accel()
    t, i, vis, rep = renderer.debug_trace_rays(o, d)
    assert len(t) == 3 and rep["kernel"] == "k_wf_trace2" and not rep["counting"] and rep["deepest"] == 0


def test_read_accel_refusals():
    """crt_debug_read_accel: CRT_ESTATE without a scene or tree, CRT_EINVAL for an unknown part or a buffer that is too
    small; a size query writes nothing; under CRT_ACCEL_NONE only the records and slot_of_index come back."""
    import ctypes as C
    from computeraytracer_amd import Renderer
    from computeraytracer_amd._lib import CrtError
    case = CASES["tiny5"]
    with Renderer(0) as r:
        for _ in range(2):                                      # no scene; a scene without a tree
            with pytest.raises(CrtError, match="scene \\+ accel required") as e:
                r.debug_read_accel()
            assert e.value.code == -3
            r.upload(TC.packed(case))
        r.build_accel("none")
        a = r.debug_read_accel()
        assert (a["accel_mode"], a["nprim"], a["root"], a["root4"], a["root8"], a["n2"], a["n4"], a["n8"]) == (0, 5, -1, -1, -1, 0, 0, 0)
        assert a["prim"].shape == (5, 12) and a["slot_of_index"].tolist() == [0, 1, 2, 3, 4]
        assert all(len(a[k]) == 0 for k in ("nodes2", "nodes4", "nodes4q", "nodes8q", "primD"))
        r.build_accel("bvh2")
        lib, h = r._lib, r._h
        nbytes = C.c_size_t(77)
        assert lib.crt_debug_read_accel(h, 1, None, 0, C.byref(nbytes)) == 0 and nbytes.value == r.accel_stats()["nodes"] * 64 > 0
        buf = np.full(nbytes.value // 4 + 1, 7.0, np.float32)
        assert lib.crt_debug_read_accel(h, 1, buf.ctypes.data, nbytes.value - 1, None) == -1          # too small: nothing is written
        assert b"the buffer" in lib.crt_last_error(h) and (buf == 7.0).all()
        assert lib.crt_debug_read_accel(h, 1, buf.ctypes.data, nbytes.value, None) == 0 and buf[-1] == 7.0 and not (buf[:-1] == 7.0).all()
        for part in (-1, 8, 99):
            assert lib.crt_debug_read_accel(h, part, None, 0, C.byref(nbytes)) == -1 and nbytes.value == 0
        assert lib.crt_debug_read_accel(h, 0, buf.ctypes.data, 8, None) == -1                         # the header too
        assert lib.crt_debug_read_accel(None, 0, None, 0, None) == -1


def test_read_accel_only_reads(renderer):
    """Counters, accumulator, sample count and the tree itself are the same before and after crt_debug_read_accel, and
    the render goes on from there bit for bit as it does without the call."""
    from computeraytracer_amd import cornell
    ps = cornell(32, 32)

    def run(hook):
        renderer.upload(ps).build_accel("lbvh")
        renderer.enable_counters(True)
        renderer.reset_counters()
        renderer.frame(3).sync()
        before = (renderer.counters(), renderer.sample, renderer.read_accum().copy(), renderer.accel_stats())
        a = renderer.debug_read_accel() if hook else None
        after = (renderer.counters(), renderer.sample, renderer.read_accum().copy(), renderer.accel_stats())
        assert before[0] == after[0] and before[1] == after[1] == 3 and before[3] == after[3]
        assert np.array_equal(bits(before[2]), bits(after[2]))
        if hook:
            b = renderer.debug_read_accel()
            for k, v in a.items():
                assert np.array_equal(np.atleast_1d(v).view(np.uint8), np.atleast_1d(b[k]).view(np.uint8)), k
            assert a["n2"] == after[3]["nodes"] and a["n4"] == after[3]["wide_nodes"] and a["depth2"] == after[3]["max_depth"]
        renderer.frame(2).sync()
        assert renderer.sample == 5
        return renderer.read_accum().copy()
    try:
        assert np.array_equal(bits(run(True)), bits(run(False)))
    finally:
        renderer.enable_counters(False)
