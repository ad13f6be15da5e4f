"""GPU tests of the ray queries (include/crt.h "Ray queries"; run with -m gpu on an MI355X):
crt_query_rays, crt_query_rays_device and crt_pick against the expectation tests/query_ref.py builds from the oracle
alone.  Every comparison is bit for bit.  What makes the ray sets worth querying is asserted on the CPU side,
test_query_cpu.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import query_ref as Q
import traversal_cases as TC
from conftest import bits
from traversal_cases import MAXU

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ESTATE, ENOMEM = -1, -3, -4
CASES = {c.name: c for c in TC.all_cases()}
BUILDERS = ("bvh2", "lbvh", "ploc")
COMBOS = [(n, b) for n in CASES for b in BUILDERS] + [(n, "none") for n in CASES if n == "baseline" or n.startswith("tiny")]
_RAYS = {}


def case_rays(name, orc):
    if name not in _RAYS:
        _RAYS[name] = Q.CaseRays(CASES[name], orc)
    return _RAYS[name]


def denominators(r, cr):
    """(C.w, D.w) per primitive as they lie on the device (debug_read_accel's PRIM and PRIMD parts), which must be the
    restated ones; CRT_ACCEL_NONE keeps no PRIMD part to read, so D.w is the restated one there."""
    cw, dw = Q.device_denominators(r.debug_read_accel(), len(cr.prims))
    cw0, dw0 = Q.patch_denominators(cr.prims)
    pat = cr.prims["category"] == 0
    assert np.array_equal(bits(cw[pat]), bits(cw0[pat]))
    if dw is None:
        dw = dw0
    assert np.array_equal(bits(dw[pat]), bits(dw0[pat]))
    return cw, dw


def fail_on_differences(got, want, cr, what, t_max=None):
    diff = Q.differences(got, want)
    if not diff:
        return
    plane, bad = next(iter(diff.items()))
    k = int(bad[0])
    per = {cr.names[c]: int((cr.lab[bad] == c).sum()) for c in np.unique(cr.lab[bad])} if len(cr.lab) == len(got[plane]) else {}
    kk = k % len(cr.o)
    pytest.fail(f"{what}: planes {[(p, len(b)) for p, b in diff.items()]} differ from the reference; plane {plane!r} by class {per}; first: "
                f"ray {k}: o {cr.o[kk].tolist()} d {cr.d[kk].tolist()} exclude {int(cr.ex[kk])} t_max {None if t_max is None else t_max[k]!r}: "
                f"kernel {np.asarray(got[plane][k]).tolist()} ({[hex(v) for v in np.atleast_1d(np.asarray(got[plane][k])).view(np.uint32)]}), "
                f"reference {np.asarray(want[plane][k]).tolist()} ({[hex(v) for v in np.atleast_1d(np.asarray(want[plane][k])).view(np.uint32)]}); "
                f"reference t* {cr.t[kk]!r} i* {int(cr.i[kk])}")


def batch(cr, kinds=Q.LIMITS):
    """The rays of a case once per limit class, in one batch: (o, d, t_max, exclude)."""
    L = np.concatenate([Q.limits(cr, k) for k in kinds])
    m = len(kinds)
    return np.tile(cr.o, (m, 1)), np.tile(cr.d, (m, 1)), L, np.tile(cr.ex, m)


def tiled(cr, m):
    """The case's rays m times over, as fail_on_differences reads them."""
    return SimpleNamespace(o=np.tile(cr.o, (m, 1)), d=np.tile(cr.d, (m, 1)), ex=np.tile(cr.ex, m), lab=np.tile(cr.lab, m), names=cr.names,
                           t=np.tile(cr.t, m), i=np.tile(cr.i, m))


def want_batch(cr, uv, table, kinds=Q.LIMITS):
    parts = [Q.expect(cr, Q.limits(cr, k), uv, table) for k in kinds]
    return {p: np.concatenate([e[p] for e in parts]) for p in parts[0]}


# ------------------------------------------------------------------ 1. CLOSEST against the reference, 4. ANY
@pytest.mark.parametrize("name,builder", COMBOS)
def test_closest_hit_equals_the_reference(renderer, orc, name, builder):
    cr = case_rays(name, orc)
    renderer.upload(cr.ps).build_accel(builder)
    table = renderer.primitive_ids()
    uv = cr.uv(*denominators(renderer, cr))
    o, d, L, ex = batch(cr)
    got = renderer.query_rays(o, d, L, ex)
    assert sorted(got) == sorted(Q.expect(cr, Q.limits(cr, "none"), uv)) and all(len(a) == len(o) for a in got.values())
    fail_on_differences(got, want_batch(cr, uv, table), tiled(cr, len(Q.LIMITS)), f"{name} / {builder}", L)
    # +inf means "no limit" too
    inf = renderer.query_rays(cr.o, cr.d, np.full(len(cr.o), np.inf, F), cr.ex)
    fail_on_differences(inf, Q.expect(cr, np.full(len(cr.o), np.inf, F), uv, table), cr, f"{name} / {builder} / t_max = +inf")
    # a non-identity id table, and again after it changed between two calls
    for mul, add in ((7, 100), (3, 5)):
        t2 = (np.arange(len(cr.prims), dtype=np.uint32) * np.uint32(mul) + np.uint32(add)).astype(np.uint32)
        renderer.set_primitive_ids(0, t2)
        ids = renderer.query_rays(cr.o, cr.d, None, cr.ex, planes=("prim", "id"))
        assert sorted(ids) == ["id", "prim"]
        fail_on_differences(ids, Q.expect(cr, Q.limits(cr, "none"), uv, t2), cr, f"{name} / {builder} / id table x{mul}+{add}")
    # ANY: the hit flag of CLOSEST on every ray, every limit class
    a = renderer.query_rays(o, d, L, ex, mode="any")
    assert list(a) == ["hit"]
    off = np.flatnonzero(a["hit"] != got["hit"])
    assert not len(off), f"{name} / {builder}: ANY differs from CLOSEST's hit flag on {len(off)} rays, first {int(off[0])}: t_max {L[off[0]]!r}"


# ------------------------------------------------------------------ 2. the fallback
@pytest.mark.parametrize("builder", ("lbvh",))
def test_the_chain_case_takes_the_fallback(renderer, orc, builder):
    case = TC.case_chain()
    cr = Q.CaseRays(case, orc)
    renderer.upload(cr.ps).build_accel(builder)
    *_, flags, _, rep = renderer.debug_walk_rays(cr.o, cr.d, cr.ex, walk="finish")
    fell = int(((flags & 2) != 0).sum())
    print(f"chain_lbvh / {builder}: {fell} of {len(cr.o)} rays fell back to the BVH2; {rep}")
    assert rep["wide"] and fell >= 1, f"vacuous: no ray of the batch fell back ({rep})"
    uv = cr.uv(*denominators(renderer, cr))
    o, d, L, ex = batch(cr, ("none", "at", "below"))
    got = renderer.query_rays(o, d, L, ex)
    fail_on_differences(got, want_batch(cr, uv, None, ("none", "at", "below")), tiled(cr, 3), f"chain_lbvh / {builder}", L)
    a = renderer.query_rays(o, d, L, ex, mode="any")
    assert np.array_equal(a["hit"], got["hit"])


# ------------------------------------------------------------------ 3. the BVH2 forms
@pytest.mark.parametrize("option,value,default", [("quantize", 0, 1), ("wf_width", 8, 4), ("pipeline", 0, 1)])
def test_the_grid_case_on_the_bvh2(renderer, orc, option, value, default):
    cr = case_rays("grid", orc)
    try:
        renderer.set_option(option, value)
        renderer.upload(cr.ps).build_accel("bvh2")
        A = renderer.debug_read_accel()
        if option != "pipeline":
            assert not (A["live4q"] == 1 and A["live8q"] == 0), "the stragglers' kernel would still walk the quantised 4-wide tree"
        uv = cr.uv(*denominators(renderer, cr))
        o, d, L, ex = batch(cr, ("none", "at", "below"))
        got = renderer.query_rays(o, d, L, ex)
        fail_on_differences(got, want_batch(cr, uv, None, ("none", "at", "below")), tiled(cr, 3), f"grid / {option} = {value}", L)
        assert np.array_equal(renderer.query_rays(o, d, L, ex, mode="any")["hit"], got["hit"])
    finally:
        renderer.set_option(option, default)


def test_any_refuses_other_planes(renderer, orc):
    from computeraytracer_amd import _lib
    cr = case_rays("tiny5", orc)
    renderer.upload(cr.ps).build_accel("bvh2")
    rays = _rays(cr.o[:4], cr.d[:4])
    hit, other = np.full(4, 9, np.uint32), np.full(16, -7.0, F)
    for plane in ("prim", "id", "t", "position", "normal", "uv"):
        p = _lib.QueryPlanes(hit=hit.ctypes.data, **{plane: other.ctypes.data})
        assert renderer._lib.crt_query_rays(renderer._h, rays.ctypes.data, 4, 1, C.byref(p)) == EINVAL, plane
        assert b"CRT_QUERY_ANY" in renderer._lib.crt_last_error(renderer._h)
        assert (hit == 9).all() and (other == -7.0).all()


# ------------------------------------------------------------------ 5. non-finite rays
def _rays(o, d, t_max=None, ex=None):
    from computeraytracer_amd.renderer import pack_rays
    return pack_rays(o, d, t_max, ex)


@pytest.mark.parametrize("builder", ("bvh2", "none"))
def test_non_finite_rays_miss(renderer, orc, builder):
    cr = case_rays("tiny9", orc)
    renderer.upload(cr.ps).build_accel(builder)
    k = np.flatnonzero(cr.hit & (cr.ex == MAXU))[:24]
    assert len(k) == 24
    bad = [np.inf, -np.inf, np.nan, 3.0e38, -3.0e38]
    o, d, L = [], [], []
    for j, v in enumerate(bad):
        for comp in range(3):
            for which in (0, 1):
                oo, dd = cr.o[k[(3 * j + comp) % 24]].copy(), cr.d[k[(3 * j + comp) % 24]].copy()
                (oo, dd)[which][comp] = v
                o.append(oo); d.append(dd)
                L.append([Q.NO_LIMIT, F(5.0), F(np.inf)][(j + comp + which) % 3])
    o, d, L = np.array(o, F), np.array(d, F), np.array(L, F)
    # (the same rays hit while they are finite)
    assert renderer.query_rays(cr.o[k], cr.d[k], planes=("hit",))["hit"].all()
    got = renderer.query_rays(o, d, L)
    n = len(o)
    assert not got["hit"].any() and (got["prim"] == MAXU).all() and (got["id"] == MAXU).all()
    assert np.array_equal(bits(got["t"]), bits(L))
    for p in ("position", "normal", "uv"):
        assert not got[p].view(np.uint32).any(), p
    assert not renderer.query_rays(o, d, L, mode="any")["hit"].any()
    assert n == 30


# ------------------------------------------------------------------ 6. block edges, 7. the device form
def _device(renderer, rays, mode="closest", planes=None, stream=None):
    """query_rays(rays=<torch tensor>) -> numpy planes (the uint32 planes viewed as such)."""
    import torch
    t = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to(f"cuda:{renderer.device}")
    keep = t.clone()
    if stream is None:
        out = renderer.query_rays(rays=t, mode=mode, planes=planes)
        torch.cuda.current_stream(t.device).synchronize()
    else:
        stream.wait_stream(torch.cuda.current_stream(t.device))      # (the upload above ran on the current stream)
        with torch.cuda.stream(stream):
            out = renderer.query_rays(rays=t, mode=mode, planes=planes)
        stream.synchronize()
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), "the device form wrote to its input"
    assert all(v.device == t.device for v in out.values())
    res = {}
    for p, v in out.items():
        a = v.cpu().numpy()
        res[p] = a.view(np.uint32) if p in ("hit", "prim", "id") else a
    return res


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 4097))
def test_block_edges_host_and_device_forms_agree(renderer, orc, n):
    cr = case_rays("tiny9", orc)
    renderer.upload(cr.ps).build_accel("bvh2")
    uv = cr.uv(*denominators(renderer, cr))
    idx = np.arange(n) % len(cr.o)
    L = np.where(idx % 3 == 0, Q.limits(cr, "below")[idx], Q.NO_LIMIT).astype(F)
    rays = _rays(cr.o[idx], cr.d[idx], L, cr.ex[idx])
    host = renderer.query_rays(rays=rays)
    assert all(len(a) == n for a in host.values())
    full = Q.expect(cr, Q.limits(cr, "none"), uv)
    below = Q.expect(cr, Q.limits(cr, "below"), uv)
    want = {p: np.where((idx % 3 == 0).reshape((-1,) + (1,) * (full[p].ndim - 1)), below[p][idx], full[p][idx]) for p in full}
    sub = SimpleNamespace(o=cr.o[idx], d=cr.d[idx], ex=cr.ex[idx], lab=cr.lab[idx], names=cr.names, t=cr.t[idx], i=cr.i[idx])
    if n:
        fail_on_differences(host, want, sub, f"tiny9 / n = {n} / host form", L)
    dev = _device(renderer, rays)
    assert sorted(dev) == sorted(host)
    assert not Q.differences(dev, host), f"n = {n}: the device form differs from the host form in {list(Q.differences(dev, host))}"
    a_host, a_dev = renderer.query_rays(rays=rays, mode="any"), _device(renderer, rays, mode="any")
    assert list(a_host) == list(a_dev) == ["hit"] and np.array_equal(a_host["hit"], a_dev["hit"]) and np.array_equal(a_host["hit"], host["hit"])


def test_device_form_on_torch_streams(renderer, orc):
    import torch
    cr = case_rays("grid", orc)
    renderer.upload(cr.ps).build_accel("bvh2")
    uv = cr.uv(*denominators(renderer, cr))
    t2 = (np.arange(len(cr.prims), dtype=np.uint32) * np.uint32(5) + np.uint32(9)).astype(np.uint32)
    renderer.set_primitive_ids(0, t2)                              # (the device form makes the table's copy itself)
    o, d, L, ex = batch(cr, ("none", "at", "below"))
    rays = _rays(o, d, L, ex)
    host = renderer.query_rays(rays=rays)
    fail_on_differences(host, want_batch(cr, uv, t2, ("none", "at", "below")), tiled(cr, 3), "grid / host form", L)
    renderer.set_primitive_ids(0, t2)                              # drops the copy again
    cur = _device(renderer, rays)
    side = _device(renderer, rays, stream=torch.cuda.Stream(device=renderer.device))
    for name, got in (("current stream", cur), ("second stream", side)):
        assert not Q.differences(got, host), f"device form on the {name}: {list(Q.differences(got, host))} differ from the host form"
    part = _device(renderer, rays, planes=("t", "uv"))
    assert sorted(part) == ["t", "uv"] and not Q.differences(part, host)
    # refusals of the tensor form
    with pytest.raises(ValueError, match="contiguous"):
        renderer.query_rays(rays=torch.zeros((4, 7), dtype=torch.float32, device=f"cuda:{renderer.device}"))
    with pytest.raises(ValueError, match="contiguous"):
        renderer.query_rays(rays=torch.zeros((4, 16), dtype=torch.float32, device=f"cuda:{renderer.device}")[:, ::2])
    with pytest.raises(ValueError, match="the context on"):
        renderer.query_rays(rays=torch.zeros((4, 8), dtype=torch.float32))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="the context on"):
            renderer.query_rays(rays=torch.zeros((4, 8), dtype=torch.float32, device="cuda:1"))


# ------------------------------------------------------------------ 8. no flush
W, H = 32, 32
PIPELINE_DEFAULTS = {"wf_cohort": 16, "wf_defer": 1}


@pytest.fixture(scope="module")
def cornell_oracle(orc):
    from computeraytracer_amd import cornell
    ps = cornell(W, H)
    sc = orc.Scene.from_packed(ps)
    return ps, {n: sc.render(n)[0] for n in (21, 40)}


def _some_rays(ps, n=200):
    rng = np.random.default_rng(3)
    o = np.tile(ps.camera[0:3].astype(F), (n, 1))
    d = rng.normal(size=(n, 3)).astype(F)
    return o, d


def test_queries_do_not_flush(orc, cornell_oracle):
    from computeraytracer_amd import Renderer
    ps, acc = cornell_oracle
    o, d = _some_rays(ps)
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2")
        want = r.query_rays(o, d)                                   # at sample 0
        want_pick = r.pick_pixels([(5, 7), (31, 31), (0, 0)])
        assert want["hit"].any()
        r.set_option("wf_defer", 1).set_option("wf_cohort", 16)
        r.frame(16).sync()
        for _ in range(5):
            r.frame(1)
        got, got_pick = r.query_rays(o, d), r.pick_pixels([(5, 7), (31, 31), (0, 0)])
        assert r.sample == 21 and r.latest_sample == 16, "a query published the pending samples"
        assert not Q.differences(got, want) and not Q.differences(got_pick, want_pick)
        r.sync()
        assert r.latest_sample == 21
        assert np.array_equal(r.read_accum().view(np.uint32)[..., :3], acc[21].view(np.uint32)[..., :3])
        # batches in flight: every call its own batch, a query every fourth call
        r.reset().set_option("wf_cohort", 1)
        for k in range(1, 41):
            r.frame(1)
            if k % 4 == 0:
                assert not Q.differences(r.query_rays(o, d), want)
                assert not Q.differences(r.pick_pixels([(5, 7), (31, 31), (0, 0)]), want_pick)
        assert r.sample == 40
        r.sync()
        assert np.array_equal(r.read_accum().view(np.uint32)[..., :3], acc[40].view(np.uint32)[..., :3])


# ------------------------------------------------------------------ 9. edits
def _check_against_records(r, orc, case, what, seed):
    prims = r.read_primitives()
    cr = Q.CaseRays(case, orc, prims=prims, seed=seed)
    assert cr.hit.sum() * 5 >= len(cr.o), f"{what}: the edited scene is hardly hit ({int(cr.hit.sum())} of {len(cr.o)})"
    uv = cr.uv(*denominators(r, cr))
    o, d, L, ex = batch(cr, ("none", "at", "below"))
    got = r.query_rays(o, d, L, ex)
    fail_on_differences(got, want_batch(cr, uv, r.primitive_ids(), ("none", "at", "below")), tiled(cr, 3), what, L)


@pytest.mark.parametrize("builder", ("bvh2", "lbvh"))
def test_queries_after_edits(renderer, orc, builder):
    from computeraytracer_amd._lib import CrtError
    case = CASES["tiny9"]
    ps = TC.packed(case)
    renderer.upload(ps).build_accel(builder)
    o, d = case_rays("tiny9", orc).o[:8], case_rays("tiny9", orc).d[:8]
    # a stale tree
    renderer.transform_primitives([(0, 4, [1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 1.0]), (6, 2, [0, -1, 0, 6, 1, 0, 0, 0, 0, 0, 1, 0], 0.5)])
    for call in (lambda: renderer.query_rays(o, d), lambda: renderer.query_rays(o, d, mode="any"), lambda: renderer.pick(0, 0)):
        with pytest.raises(CrtError, match="crt_refit_accel") as e:
            call()
        assert e.value.code == ESTATE
    renderer.refit_accel()
    _check_against_records(renderer, orc, case, f"tiny9 / {builder} / transform + refit", 51)
    # a topology-stale tree
    renderer.remove_primitives([(2, 2)], lights=ps.lights)
    with pytest.raises(CrtError, match="crt_refit_accel") as e:
        renderer.query_rays(o, d)
    assert e.value.code == ESTATE
    renderer.refit_accel()
    assert len(renderer.read_primitives()) == 7
    _check_against_records(renderer, orc, case, f"tiny9 / {builder} / remove + refit", 52)
    more = TC.join(TC.tris([[1, 1, -9]], [[9, 1, -9]], [[1, 9, -8]]), TC.spheres([[-3, 8, 3]], [2.0]))
    more["data4"][:, 3] += 7                                    # (a record's index is its position in the new list)
    renderer.append_primitives(more)
    with pytest.raises(CrtError, match="crt_refit_accel"):
        renderer.query_rays(o, d)
    renderer.refit_accel()
    renderer.set_primitive_ids(7, [40, 41])
    assert len(renderer.read_primitives()) == 9
    _check_against_records(renderer, orc, case, f"tiny9 / {builder} / append + refit", 53)


# ------------------------------------------------------------------ 10. pick
def _pick_all(r, x0=0, y0=0, w=W, h=H):
    xs, ys = np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + h))
    return r.pick_pixels(np.stack([xs.ravel(), ys.ravel()], 1))


def _same_as_gbuffer(r, got, what):
    if r.sample == 0:
        r.frame(1).sync()                                       # (crt_read_gbuffer wants a sample traced; crt_pick does not)
    g = r.read_gbuffer().reshape(-1, 8)
    assert len(g) == len(got["t"]), what
    assert np.array_equal(bits(got["t"]), bits(g[:, 0])), what
    assert np.array_equal(bits(got["position"][:, :3]), bits(g[:, 1:4])) and not got["position"][:, 3].view(np.uint32).any(), what
    assert np.array_equal(bits(got["normal"][:, :3]), bits(g[:, 4:7])) and not got["normal"][:, 3].view(np.uint32).any(), what
    assert np.array_equal(got["prim"], g[:, 7].view(np.uint32)), what
    assert np.array_equal(got["hit"], (g[:, 7].view(np.uint32) != MAXU).astype(np.uint32)), what
    return g


@pytest.mark.parametrize("builder", ("bvh2", "none"))
def test_pick_equals_the_gbuffer(cornell_oracle, builder):
    from computeraytracer_amd import Renderer
    from computeraytracer_amd._lib import CrtError
    from computeraytracer_amd.scene import PackedScene, orbit_cameras
    ps, _ = cornell_oracle
    with Renderer(0) as r:
        r.upload(ps).build_accel(builder)
        ids = (np.arange(len(ps.primitives), dtype=np.uint32) + np.uint32(1000)).astype(np.uint32)
        r.set_primitive_ids(0, ids)
        full = _pick_all(r)
        g = _same_as_gbuffer(r, full, f"cornell / {builder}")
        hit = full["hit"] == 1
        assert hit.sum() * 2 > W * H and (full["id"][~hit] == MAXU).all()
        assert np.array_equal(full["id"][hit], ids[full["prim"][hit]])
        # the scalar form
        k = int(np.flatnonzero(hit)[W * H // 3])
        one = r.pick(k % W, k // W)
        assert one["prim"] == int(full["prim"][k]) and one["id"] == int(ids[one["prim"]]) and F(one["t"]) == full["t"][k]
        assert np.array_equal(bits(one["position"]), bits(g[k, 1:4])) and np.array_equal(bits(one["normal"]), bits(g[k, 4:7]))
        # under a tile: global coordinates
        r.set_tile(8, 4, 24, 20)
        tile = _pick_all(r, 8, 4, 16, 16)
        _same_as_gbuffer(r, tile, f"cornell / {builder} / tile")
        sel = (np.arange(4, 20)[:, None] * W + np.arange(8, 24)[None, :]).ravel()
        assert not Q.differences(tile, {p: a[sel] for p, a in full.items()})
        assert not Q.differences(_pick_all(r), full), "crt_set_tile moved the pick's coordinates"
        r.set_tile(0, 0, W, H)
        # outside the image
        for xy in ((W, 0), (0, H), (0xFFFFFFFF, 0)):
            with pytest.raises(CrtError, match="outside") as e:
                r.pick_pixels([(1, 1), xy])
            assert e.value.code == EINVAL
        # after a camera move
        r.set_camera(orbit_cameras(ps.camera, 16)[3])
        moved = _pick_all(r)
        _same_as_gbuffer(r, moved, f"cornell / {builder} / set_camera")
        assert Q.differences(moved, full)
        # the camera at infinity: every ray is non-finite, every pixel a miss
        cam = ps.camera.copy()
        cam[0:3] = np.inf
        r.upload(PackedScene(ps.primitives, ps.lights, cam, ps.spectra, ps.cie)).build_accel(builder)
        far = _pick_all(r)
        assert not far["hit"].any() and (far["prim"] == MAXU).all() and (bits(far["t"]) == bits(Q.NO_LIMIT)).all()
        assert r.pick(3, 3) is None


# ------------------------------------------------------------------ 11. refusals
def _raw(r, rays, n, mode, planes, device=False):
    from computeraytracer_amd import _lib
    p = None if planes is None else _lib.QueryPlanes(**{k: (v if isinstance(v, int) else v.ctypes.data) for k, v in planes.items()})
    ptr = rays if rays is None or isinstance(rays, int) else rays.ctypes.data
    arg = None if p is None else C.byref(p)
    if device:
        return r._lib.crt_query_rays_device(r._h, ptr, n, mode, arg, None)
    return r._lib.crt_query_rays(r._h, ptr, n, mode, arg)


def test_refusals(orc):
    from computeraytracer_amd import Renderer
    cr = case_rays("tiny5", orc)
    rays = _rays(cr.o[:8], cr.d[:8])
    hit, pos = np.full(8, 9, np.uint32), np.full((9, 4), -7.0, F)
    xy = np.zeros(2, np.uint32)
    with Renderer(0) as r:
        from computeraytracer_amd import _lib
        planes = _lib.QueryPlanes(hit=hit.ctypes.data)
        # no scene; a scene without a tree
        for _ in range(2):
            for dev in (False, True):
                assert _raw(r, rays, 8, 0, dict(hit=hit), dev) == ESTATE and b"scene + accel required" in r._lib.crt_last_error(r._h)
            assert r._lib.crt_pick(r._h, xy.ctypes.data, 1, C.byref(planes)) == ESTATE
            r.upload(cr.ps)
        r.build_accel("bvh2")
        for dev in (False, True):
            assert _raw(r, rays, 8, 0, None, dev) == EINVAL and b"out is NULL" in r._lib.crt_last_error(r._h)
            assert _raw(r, rays, 8, 0, {}, dev) == EINVAL and b"every plane is NULL" in r._lib.crt_last_error(r._h)
            assert _raw(r, rays, 8, 2, dict(hit=hit), dev) == EINVAL and b"unknown mode" in r._lib.crt_last_error(r._h)
            assert _raw(r, rays, 8, -1, dict(hit=hit), dev) == EINVAL
            assert _raw(r, None, 8, 0, dict(hit=hit), dev) == EINVAL and b"NULL" in r._lib.crt_last_error(r._h)
            assert _raw(r, rays.ctypes.data + 4, 7, 0, dict(hit=hit), dev) == EINVAL and b"16-byte aligned" in r._lib.crt_last_error(r._h)
            assert _raw(r, rays, 8, 0, dict(position=pos.ctypes.data + 4), dev) == EINVAL and b"16-byte aligned" in r._lib.crt_last_error(r._h)
            assert _raw(r, rays, 8, 0, dict(normal=pos.ctypes.data + 8), dev) == EINVAL
            assert _raw(r, rays, 1 << 32, 0, dict(hit=hit), dev) == EINVAL and b"2^32" in r._lib.crt_last_error(r._h)
            assert _raw(r, rays, 0, 0, dict(hit=hit), dev) == 0          # n == 0 succeeds and does nothing
            assert _raw(r, None, 0, 0, dict(hit=hit), dev) == 0
        assert r._lib.crt_pick(r._h, None, 1, C.byref(planes)) == EINVAL
        assert r._lib.crt_pick(r._h, xy.ctypes.data, 1, None) == EINVAL
        assert r._lib.crt_pick(r._h, xy.ctypes.data, 0, C.byref(planes)) == 0
        assert (hit == 9).all() and (pos == -7.0).all()
        assert _raw(r, rays, 8, 0, dict(hit=hit)) == 0 and (hit <= 1).all()


def test_failed_allocations_leave_nothing_behind(orc):
    """Each device allocation of a fresh context's first crt_query_rays fails in turn: CRT_ENOMEM, the outputs untouched,
    and the next call correct."""
    from computeraytracer_amd import Renderer
    from computeraytracer_amd import renderer as R
    cr = case_rays("tiny9", orc)
    rays = _rays(cr.o, cr.d, None, cr.ex)
    n = len(rays)
    want = None
    failed = 0
    for k in range(1, 40):
        with Renderer(0) as r:
            r.upload(cr.ps).build_accel("bvh2")
            r.set_primitive_ids(0, np.arange(len(cr.prims), dtype=np.uint32) + np.uint32(3))      # (the `id` plane needs a copy of the table)
            out = {p: np.full((n,) + R._QUERY_SHAPE[p][0], 0x5A5A5A5A, np.uint32) for p in R.QUERY_PLANES}
            try:
                r.set_option("debug_fail_alloc", k)
                rc = _raw(r, rays, n, 0, out)
            finally:
                r.set_option("debug_fail_alloc", 0)
            if rc == 0:
                want = {p: (a if p in ("hit", "prim", "id") else a.view(F)) for p, a in out.items()}
                break
            assert rc == ENOMEM, (k, rc, r._lib.crt_last_error(r._h))
            failed += 1
            assert all((a == 0x5A5A5A5A).all() for a in out.values()), f"allocation {k} failed and the call wrote to its outputs"
            again = r.query_rays(rays=rays)
            uv = cr.uv(*denominators(r, cr))
            fail_on_differences(again, Q.expect(cr, Q.limits(cr, "none"), uv, r.primitive_ids()), cr, f"the call after allocation {k} failed")
    assert want is not None and failed == 9, f"{failed} allocations failed in turn; the call makes 9 (the rays, seven planes, the id table)"
    assert (want["id"][want["hit"] == 1] == want["prim"][want["hit"] == 1] + 3).all()
