"""k_wf_trace2's pass variants (run with -m gpu on an MI355X): whatever the build's CRT_WF_T2_* switches
are, the production instantiation behind crt_debug_trace_rays gives every ray what the references give it, bit for bit:

  extension rays   (bits(t), index)  ==  crt_debug_intersect under build_accel("none"), the reference loop on the GPU
  shadow rays      visibility        ==  the same hook with wf_trace_form=1 (k_wf_trace<,1>) on the same tree
  counting variant (enable_counters) ==  the plain one, output for output

for ray counts around the ring of 32 ready rays, a wave of 64 and the 128-entry chunks, both kinds of ray in all four
list classes (the hook lays ray i out by i % 16 and (i / 16) & 1), on two scenes:

  mixed   6 patches, 3 spheres, 304 triangles: leaves that mix kinds; coplanar duplicate triangles (equal t: the later
          index wins), triangles in the floor patch's plane (a patch and a triangle at equal t), excluded primitives,
          and shadow rays towards a light patch that lies in the ceiling patch's plane, occluded and not.
  deep    traversal_cases.case_deep under the LBVH builder: the walk leaves the 16 LDS stack entries, whole waves at once
          (the rays start inside every box of the chain), so a second node step pushes and pops in the overflow area.

What the mixed scene is for is asserted on the reference side (test_mixed_scene_holds_what_it_is_for).  One 64 x 64 render
of mesh10k at 4 spp is byte-equal between the two forms."""
import numpy as np
import pytest

import traversal_cases as TC
from conftest import bits
from traversal_cases import MAXU

pytestmark = pytest.mark.gpu

COUNTS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4097]
NMAX = max(COUNTS)
LIGHT = 5                                                     # mixed scene: the light patch, in the plane of patch 3 (the ceiling)
N_GRID = 288                                                  # ... its 12 x 12 x 2 grid triangles, indices 9 ..
DUP0, FLOOR0 = 9 + N_GRID, 9 + N_GRID + 8                     # ... the copies of the grid's first eight, the eight floor triangles


def mixed_case():
    F = np.float32
    box = TC.box_patches([0, 0, 0], [32, 16, 32])[:5]        # back, left, floor (2), ceiling (3), right; the front is open
    light = TC.patches([[12, 16, 12]], [[8, 0, 0]], [[0, 0, 8]])
    sph = TC.spheres([[8, 6, 8], [22, 5, 20], [16, 11, 16]], [3.0, 2.5, 2.0])        # the third hangs under the light
    grid = TC.grid_quad(12, 2.0, (4.0, 4.0, 4.0))            # the plane y = 4
    dup = grid[:8].copy()                                     # cells (0, 0..3) once more: x in [4, 6], z in [4, 12]
    floor = TC.grid_quad(2, 4.0, (8.0, 0.0, 8.0))            # in the floor patch's plane: x, z in [8, 16]
    prims = TC.join(box, light, sph, grid, dup, floor)
    assert len(prims) == FLOOR0 + 8 == 313 and (prims["category"][:6] == 0).all() and (prims["category"][6:9] == 1).all()
    assert F(prims["data1"][LIGHT][1]) == F(16)
    return TC._finish(TC.Case("mixed", prims, lights=[LIGHT], shadow_close=0.4))


def down_rays(rng, n, xs, zs, ys):
    """Straight down from exact coordinates: every primitive of one horizontal plane sits at exactly the same t."""
    o = np.stack([rng.choice(np.float32(xs), n), rng.choice(np.float32(ys), n), rng.choice(np.float32(zs), n)], 1).astype(np.float32)
    return o, np.tile(np.float32([0, -1, 0]), (n, 1))


class Bundle:
    """NMAX rays of a case -- ray i is a shadow ray where i % 3 == 1 -- and what the references give them."""

    def __init__(self, case, builder, brutes, renderer):
        a, b = brutes
        self.case, self.builder, self.ps = case, builder, TC.packed(case)
        L = case.lights[0]
        a.upload(self.ps).build_accel("none")
        b.upload(TC.single(case, L)).build_accel("none")

        def ref_of(r):
            def ref(o, d, ex):
                out = r.debug_intersect(o, d, ex)
                return out[:, 0].copy(), out[:, 7].view(np.uint32).copy()
            return ref
        self.ref = ref = ref_of(a)
        nprim = len(case.prims)
        R = TC.Rays(case, seed=41)
        rng = np.random.default_rng(42)
        eo, ed, ee, self.names, lab = [], [], [], [], []
        for cname, co, cd, mode in R.classes(230):
            eo.append(co); ed.append(cd); ee.append(TC.resolve_exclude(ref, rng, nprim, co, cd, mode))
            lab.append(np.full(len(co), len(self.names))); self.names.append(cname)
        if case.name == "mixed":
            q = np.arange(1, 4) * 0.25
            for cname, (co, cd) in (("dup_tie", down_rays(rng, 150, 4 + q, 4 + np.arange(1, 32) * 0.25, [5, 6, 8])),
                                    ("floor_tie", down_rays(rng, 150, 8 + np.arange(1, 32) * 0.25, 8 + np.arange(1, 32) * 0.25, [1, 2, 3]))):
                eo.append(co); ed.append(cd); ee.append(np.full(len(co), MAXU, np.uint32))
                lab.append(np.full(len(co), len(self.names))); self.names.append(cname)
        eo, ed, ee, lab = (np.concatenate(x) for x in (eo, ed, ee, lab))
        so, sd = R.shadow(L, 1400)
        tie = R.shadow_tie(L, 300)
        if tie is not None:
            so, sd = np.concatenate([so, tie[0]]), np.concatenate([sd, tie[1]])
        se = TC.shadow_excludes(case, L, len(so), nprim, rng)
        t_l, own, self.loop_vis, _, _ = TC.shadow_expect(ref, ref_of(b), L, so, sd, se)
        assert own.all(), f"{case.name}: {int((~own).sum())} shadow rays miss their light in the reference loop"
        pe, psh = rng.permutation(len(eo)), rng.permutation(len(so))
        self.shadow = np.arange(NMAX) % 3 == 1
        ns, ne = int(self.shadow.sum()), int((~self.shadow).sum())
        assert ne <= len(pe) and ns <= len(psh), (ne, len(pe), ns, len(psh))
        pe, psh = pe[:ne], psh[:ns]
        self.o, self.d = np.zeros((NMAX, 3), np.float32), np.zeros((NMAX, 3), np.float32)
        self.ex, self.light = np.full(NMAX, MAXU, np.uint32), np.zeros(NMAX, np.uint32)
        self.t_light = np.zeros(NMAX, np.float32)
        self.lab = np.full(NMAX, -1)
        self.o[~self.shadow], self.d[~self.shadow], self.ex[~self.shadow], self.lab[~self.shadow] = eo[pe], ed[pe], ee[pe], lab[pe]
        self.o[self.shadow], self.d[self.shadow], self.ex[self.shadow] = so[psh], sd[psh], se[psh]
        self.t_light[self.shadow], self.light[self.shadow] = t_l[psh], L
        self.loop_vis = self.loop_vis[psh]
        # the references, once: the loop for the extension rays, form 1 on the same tree for the shadow rays
        self.want_t, self.want_i = np.zeros(NMAX, np.float32), np.zeros(NMAX, np.uint32)
        self.want_t[~self.shadow], self.want_i[~self.shadow] = ref(self.o[~self.shadow], self.d[~self.shadow], self.ex[~self.shadow])
        renderer.upload(self.ps).build_accel(builder)
        try:
            renderer.set_option("wf_trace_form", 1)
            _, _, vis1, rep = renderer.debug_trace_rays(self.o, self.d, self.ex, self.shadow, self.t_light, self.light)
        finally:
            renderer.set_option("wf_trace_form", 2)
        assert rep["kernel"] == "k_wf_trace<,1>", rep
        self.want_vis = np.where(self.shadow, vis1, 0).astype(np.uint32)
        for arr in (self.o, self.d, self.ex, self.t_light, self.light, self.want_t, self.want_i, self.want_vis):
            arr.setflags(write=False)

    def trace(self, renderer, n, counting):
        renderer.enable_counters(counting)
        try:
            return renderer.debug_trace_rays(self.o[:n], self.d[:n], self.ex[:n], self.shadow[:n], self.t_light[:n], self.light[:n])
        finally:
            renderer.enable_counters(False)

    def check(self, renderer, n):
        t, i, vis, rep = self.trace(renderer, n, False)
        assert rep["kernel"] == "k_wf_trace2" and not rep["counting"] and rep["lds_entries"] == 16, rep
        bad = (bits(t) != bits(self.want_t[:n])) | (i != self.want_i[:n]) | (vis != self.want_vis[:n])
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            kind = "shadow" if self.shadow[k] else self.names[self.lab[k]]
            pytest.fail(f"{self.case.name} / {n} rays: {int(bad.sum())} differ from their reference; first: ray {k} ({kind}) o {self.o[k].tolist()} "
                        f"d {self.d[k].tolist()} exclude {int(self.ex[k])}: kernel t 0x{int(bits(t)[k]):08x} index {int(i[k])} visible {int(vis[k])}, "
                        f"reference t 0x{int(bits(self.want_t)[k]):08x} index {int(self.want_i[k])} visible {int(self.want_vis[k])}; {rep}")
        tc, ic, visc, repc = self.trace(renderer, n, True)
        assert repc["counting"] and repc["kernel"] == "k_wf_trace2", repc
        assert np.array_equal(bits(tc), bits(t)) and np.array_equal(ic, i) and np.array_equal(visc, vis), f"{self.case.name} / {n} rays: counting variant differs"
        return repc


@pytest.fixture(scope="module")
def brutes():
    from computeraytracer_amd import Renderer
    a, b = Renderer(0), Renderer(0)
    yield a, b
    a.close()
    b.close()


_BUNDLE = {}
SCENES = {"mixed": (mixed_case, "bvh2"), "deep": (TC.case_deep, "lbvh")}


def bundle(name, brutes, renderer):
    """The scene's rays and references, made once; `renderer` holds that scene's tree afterwards."""
    if name not in _BUNDLE:
        make, builder = SCENES[name]
        _BUNDLE.clear()                                         # (one scene at a time: the parametrisation goes scene by scene)
        _BUNDLE[name] = Bundle(make(), builder, brutes, renderer)
    elif renderer.scene is not _BUNDLE[name].ps:
        renderer.upload(_BUNDLE[name].ps).build_accel(_BUNDLE[name].builder)
    return _BUNDLE[name]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", list(SCENES))
def test_rays_equal_their_references(renderer, brutes, name, n):
    B = bundle(name, brutes, renderer)
    repc = B.check(renderer, n)
    if name == "deep" and n >= 64:                              # a whole wave's rays start on the root together
        assert repc["deepest"] > repc["lds_entries"] == 16, f"the overflow area was not reached: {repc}"
        assert repc["deepest"] <= repc["capacity"], repc


def test_mixed_scene_holds_what_it_is_for(renderer, brutes):
    B = bundle("mixed", brutes, renderer)
    ext = ~B.shadow
    lab = np.where(ext, B.lab, -1)

    def tie_count(cls, later, earlier):
        """Rays of the class whose closest hit is in `later` and that hit a primitive of `earlier` at the same t without it."""
        m = (lab == B.names.index(cls)) & np.isin(B.want_i, later)
        assert m.sum() >= 40, (cls, int(m.sum()))
        t2, i2 = B.ref(B.o[m], B.d[m], B.want_i[m])             # the winner excluded: the runner-up
        return int((np.isin(i2, earlier) & (bits(t2) == bits(B.want_t[m]))).sum())
    assert tie_count("dup_tie", np.arange(DUP0, DUP0 + 8), np.arange(9, 17)) >= 40           # coplanar copies: the later index wins
    assert tie_count("floor_tie", np.arange(FLOOR0, FLOOR0 + 8), [2]) >= 40                  # a patch and a triangle at equal t
    assert (ext & (B.ex != MAXU)).sum() >= 500                                              # excluded primitives
    assert (ext & (B.ex != MAXU) & (B.want_i != MAXU)).sum() >= 200
    cats = B.case.prims["category"][B.want_i[ext & (B.want_i != MAXU)]]
    assert all((cats == c).sum() >= 30 for c in (0, 1, 2)), np.bincount(cats)                # closest hits of every kind
    sh = B.shadow
    vis = B.want_vis[sh]
    assert (vis == 1).sum() >= 100 and (vis == 0).sum() >= 100, np.bincount(vis)            # occluded and not
    assert np.array_equal(vis, B.loop_vis.astype(np.uint32)), "form 1 and the reference loop disagree on the shadow rays"
    # the light lies in the ceiling's plane: without the light, unoccluded shadow rays end on the ceiling at the light's t
    k = np.flatnonzero(sh)[vis == 1]
    t3, i3 = B.ref(B.o[k], B.d[k], np.full(len(k), LIGHT, np.uint32))
    assert ((i3 == 3) & (bits(t3) == bits(B.t_light[k]))).sum() >= 50


def test_render_is_the_same_under_both_forms(renderer):
    from computeraytracer_amd.scenes_synth import mesh10k
    ps = mesh10k(64, 64)
    got = {}
    try:
        for form, kernel in ((2, "k_wf_trace2"), (1, "k_wf_trace<,1>")):
            renderer.set_option("wf_trace_form", form)
            renderer.upload(ps).build_accel("bvh2")
            assert renderer.debug_trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))[3]["kernel"] == kernel
            renderer.frame(4).sync()
            got[form] = (renderer.read_accum().copy(), renderer.read_rgba8().copy())
    finally:
        renderer.set_option("wf_trace_form", 2)
    assert np.array_equal(got[2][0].view(np.uint8), got[1][0].view(np.uint8)), "read_accum differs between the forms"
    assert np.array_equal(got[2][1].view(np.uint8), got[1][1].view(np.uint8)), "read_rgba8 differs between the forms"
    assert got[2][1].any()
