"""GPU tests of the radiance queries (include/crt.h "Radiance queries"; run with -m gpu on an MI355X):
crt_radiance_rays and crt_radiance_rays_device against the expectation tests/radiance_ref.py builds from the oracle
alone.  Every comparison is bit for bit, NaNs by their bits.  What makes the ray set worth tracing is asserted on the CPU
side, test_radiance_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import radiance_ref as R
from conftest import bits

pytestmark = pytest.mark.gpu

F = np.float32
MAXU = 0xFFFFFFFF
EINVAL, ESTATE, ENOMEM = -1, -3, -4
BUILDERS = ("bvh2", "lbvh", "ploc", "none")


def both(orc, name):
    """The scene as uploaded, and its probe rays followed by the extra probe's: (ps, o, d, keys (n, 4), expected)."""
    ps, a = R.rays_of(orc, name)
    _, b = R.rays_of(orc, name, extra=True)
    ea, eb = R.expected(a), R.expected(b)
    keys = np.concatenate([a.keys, b.keys])
    keys = np.concatenate([keys, np.zeros((len(keys), 1), np.uint32)], axis=1)
    want = {p: np.concatenate([getattr(ea, p), getattr(eb, p)]) for p in ("xyz", "y2", "rgba8", "has8")}
    want["finite"] = np.concatenate([a.finite, b.finite])
    return ps, np.concatenate([a.o, b.o]), np.concatenate([a.d, b.d]), keys, want


def raw(a):
    """The bytes of each row of a plane."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1)


def check(got, want, what, sel=None):
    """got: radiance_rays' dict for one sample per ray; want: both()'s expectation (sel: the rays of it that were sent)."""
    w = want if sel is None else {p: a[sel] for p, a in want.items()}
    n = len(w["y2"])
    assert got["xyz"].shape == (n, 4) and got["y2"].shape == (n,) and got["rgba8"].shape == (n, 4), what
    bad = np.flatnonzero((bits(got["xyz"][:, :3]) != bits(w["xyz"])).any(axis=1))
    assert not len(bad), (f"{what}: xyz of {len(bad)} of {n} rays differs from the oracle's; first: ray {int(bad[0])}: kernel "
                          f"{got['xyz'][bad[0]].tolist()}, oracle {w['xyz'][bad[0]].tolist()}")
    assert not got["xyz"][:, 3].view(np.uint32).any(), f"{what}: channel 3 of xyz is not +0"
    bad = np.flatnonzero(bits(got["y2"]) != bits(w["y2"]))
    assert not len(bad), f"{what}: y2 of {len(bad)} rays is not fl(Y * Y); first: ray {int(bad[0])}: {got['y2'][bad[0]]!r}, want {w['y2'][bad[0]]!r}"
    h = w["has8"]
    bad = np.flatnonzero((got["rgba8"][h] != w["rgba8"][h]).any(axis=1))
    assert not len(bad), f"{what}: rgba8 of {len(bad)} rays with key sample 1 is not the oracle's render(1) pixel"


# ------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", R.SCENES)
def test_radiance_equals_the_oracle(renderer, orc, name, builder):
    ps, o, d, keys, want = both(orc, name)
    renderer.upload(ps).build_accel(builder)
    assert renderer.debug_hit_pad == orc.Scene.from_packed(ps).hit_pad()
    check(renderer.radiance_rays(o, d, keys), want, f"{name} / {builder}")


@pytest.mark.parametrize("option,value,default", [("quantize", 0, 1), ("wf_width", 8, 4), ("pipeline", 0, 1)])
def test_radiance_on_the_bvh2_walks(renderer, orc, option, value, default):
    ps, o, d, keys, want = both(orc, "baseline")
    try:
        renderer.set_option(option, value)
        renderer.upload(ps).build_accel("bvh2")
        A = renderer.debug_read_accel()
        if option != "pipeline":
            assert not (A["live4q"] == 1 and A["live8q"] == 0), "the quantised 4-wide tree would still be walked"
        check(renderer.radiance_rays(o, d, keys), want, f"baseline / {option} = {value}")
    finally:
        renderer.set_option(option, default)


# ------------------------------------------------------------------ 2. the product
def own_camera_rays(orc, ps, samples):
    """The camera rays of every pixel of ps's own camera for each sample: (o, d, keys (n, 4)), sample-major, row-major."""
    sc = orc.Scene.from_packed(ps)
    o, d, k = [], [], []
    for s in samples:
        for y in range(ps.height):
            for x in range(ps.width):
                log = sc.ray_log(x, y, s, cap=4)
                o.append(log[0, 0:3]); d.append(log[0, 3:6]); k.append((x, y, s, 0))
    return np.array(o, F), np.array(d, F), np.array(k, np.uint32)


@pytest.mark.parametrize("name", ("patch", "sphere_only"))
def test_own_camera_rays_sum_to_the_accumulator(renderer, orc, name):
    ps = R.scene(name)
    renderer.upload(ps).build_accel("bvh2")
    npix = ps.width * ps.height
    o, d, k = own_camera_rays(orc, ps, (1, 2, 3, 4))
    parts = []
    for j in range(4):
        sl = slice(j * npix, (j + 1) * npix)
        assert (k[sl, 2] == j + 1).all()
        g = renderer.radiance_rays(o[sl], d[sl], k[sl], planes=("xyz", "y2"))
        parts.append((g["xyz"], g["y2"]))
    total, _ = R.sequential_sums(parts)
    renderer.reset()
    renderer.frame(4).sync()
    acc = renderer.read_accum().reshape(npix, 4)
    assert renderer.sample == 4
    assert np.array_equal(bits(total[:, :3]), bits(acc[:, :3])), f"{name}: four calls of one sample do not sum to crt_read_accum after crt_trace(4)"


# ------------------------------------------------------------------ 3. several samples
def _fixed_rays(orc, n=300):
    ps, o, d, keys, want = both(orc, "tri")
    sel = np.flatnonzero(want["finite"])[:: max(1, int(want["finite"].sum()) // n)][:n]
    assert len(sel) == n
    return ps, o[sel], d[sel], keys[sel]


@pytest.mark.parametrize("s0", (3, 0xFFFFFFFE))
def test_several_samples_are_the_sequential_sum(renderer, orc, s0):
    ps, o, d, keys = _fixed_rays(orc)
    renderer.upload(ps).build_accel("bvh2")
    k = keys.copy()
    k[:, 2] = s0
    got = renderer.radiance_rays(o, d, k, n_samples=5)
    order = [(s0 + j) & MAXU for j in range(5)]
    if s0 == 0xFFFFFFFE:
        assert order == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1, 2]
    parts = []
    for s in order:
        k1 = keys.copy()
        k1[:, 2] = s
        g = renderer.radiance_rays(o, d, k1, planes=("xyz", "y2"))
        parts.append((g["xyz"], g["y2"]))
    assert any(not np.array_equal(bits(parts[0][0]), bits(p[0])) for p in parts[1:]), "vacuous: every sample gives the same paths"
    sx, sq = R.sequential_sums(parts)
    assert np.array_equal(bits(got["xyz"]), bits(sx)) and np.array_equal(bits(got["y2"]), bits(sq))
    # rgba8: the colour tail of xyz / 5, by the oracle's own tail (radiance_ref.oracle_rgba8)
    assert np.array_equal(got["rgba8"], R.oracle_rgba8(orc, got["xyz"], 5))
    assert (got["rgba8"][:, :3].max(axis=1) > 0).sum() > 100, "vacuous: the rays see nothing"


# ------------------------------------------------------------------ 4. ownership and the stride
@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_block_edges(renderer, orc, n):
    ps, o, d, keys, want = both(orc, "patch")
    renderer.upload(ps).build_accel("bvh2")
    sel = (np.arange(n) * 7 + 3) % len(o)
    pre = {"xyz": np.full((n + 1, 4), -7.0, F), "y2": np.full(n + 1, -7.0, F), "rgba8": np.full((n + 1, 4), 9, np.uint8)}
    from computeraytracer_amd import _lib
    from computeraytracer_amd.renderer import pack_keys, pack_rays
    rays, k = pack_rays(o[sel], d[sel]), pack_keys(keys[sel, 0], keys[sel, 1], keys[sel, 2])
    arg = _lib.RadiancePlanes(**{p: a.ctypes.data for p, a in pre.items()})
    assert renderer._lib.crt_radiance_rays(renderer._h, rays.ctypes.data, k.ctypes.data, n, 1, C.byref(arg)) == 0
    check({p: a[:n] for p, a in pre.items()}, want, f"n = {n}", sel)
    assert (pre["xyz"][n] == -7.0).all() and pre["y2"][n] == -7.0 and (pre["rgba8"][n] == 9).all(), "the call wrote past ray n - 1"
    assert renderer.radiance_lanes(n) == 64 * ((n + 63) // 64)


def test_more_rays_than_lanes(renderer, orc):
    ps, o, d, keys, want = both(orc, "patch")
    renderer.upload(ps).build_accel("bvh2")
    m = len(o)
    G = renderer.radiance_lanes(1 << 30)
    assert G % 64 == 0 and G >= 64 * 256, G
    copies = G // m + 2
    n = copies * m - 5                                           # (no multiple of 64 or of the set)
    assert n > G and renderer.radiance_lanes(n) == G, "the batch does not exceed the persistent grid: nothing strides"
    idx = np.arange(n) % m
    got = renderer.radiance_rays(o[idx], d[idx], keys[idx])
    check({p: a[:m] for p, a in got.items()}, want, "the first copy of each ray")
    for p, a in got.items():
        first = a[:m][idx]
        same = (first.view(np.uint32) == a.view(np.uint32)) if a.dtype != np.uint8 else (first == a)
        bad = np.flatnonzero(~same.reshape(n, -1).all(axis=1))
        assert not len(bad), f"{p}: {len(bad)} copies differ from their ray's first copy; first at {int(bad[0])} (ray {int(idx[bad[0]])}, G = {G})"
    # several samples per ray while striding, and a permuted batch
    perm = np.random.default_rng(5).permutation(n)
    a3 = renderer.radiance_rays(o[idx], d[idx], keys[idx], n_samples=3)
    b3 = renderer.radiance_rays(o[idx][perm], d[idx][perm], keys[idx][perm], n_samples=3)
    for p in a3:
        assert np.array_equal(a3[p][perm].view(np.uint8), b3[p].view(np.uint8)), f"{p}: a permuted batch does not return permuted outputs"
        assert np.array_equal(a3[p][:m][idx].view(np.uint8), a3[p].view(np.uint8)), f"{p}: copies differ at three samples per ray"


# ------------------------------------------------------------------ 5. no flush
def _pipeline_run(ps, o, d, keys, call, counters):
    """frame(16), a sync, five frame(1) left in flight, then (call) the radiance call; what the context holds after a
    sync.  counters: with crt_enable_counters."""
    from computeraytracer_amd import Renderer
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2")
        r.enable_counters(counters)
        quiet = r.radiance_rays(o, d, keys) if call else None
        before = r.counters()
        r.set_option("wf_defer", 1).set_option("wf_cohort", 16)
        r.frame(16).sync()
        for _ in range(5):
            r.frame(1)
        got = latest = None
        if call:
            got = r.radiance_rays(o, d, keys)
            latest = (r.sample, r.latest_sample)
        r.sync()
        assert r.latest_sample == 21
        return quiet, got, before, latest, r.read_accum(), r.sample, r.counters()


def test_radiance_does_not_stop_the_pipeline(orc):
    ps, o, d, keys, want = both(orc, "patch")
    quiet, got, _, latest, acc, sample, _ = _pipeline_run(ps, o, d, keys, True, False)
    check(quiet, want, "a quiet context")
    assert latest == (21, 16), f"the call published the pending samples: (sample, latest_sample) = {latest}"
    for p in quiet:
        assert np.array_equal(raw(quiet[p]), raw(got[p])), f"{p} differs while batches are in flight"
    assert sample == 21 and np.array_equal(bits(acc[..., :3]), bits(orc.Scene.from_packed(ps).render(21)[0][..., :3]))
    # the counters: nothing of the call in them
    quiet, got, before, _, acc1, sample1, counters1 = _pipeline_run(ps, o, d, keys, True, True)
    assert all(v == 0 for v in before.values()), f"crt_counters counted the call's rays: {before}"
    for p in quiet:
        assert np.array_equal(raw(quiet[p]), raw(got[p])), f"{p} differs while batches are in flight (counters on)"
    _, _, _, _, acc0, sample0, counters0 = _pipeline_run(ps, o, d, keys, False, True)
    assert sample1 == sample0 == 21 and np.array_equal(bits(acc1), bits(acc0)) and np.array_equal(bits(acc1), bits(acc))
    # (the counters that depend on the paths alone: "nodes" and "prims" also depend on which walk served a ray, a matter
    # of timing, and differ between any two runs of the same render -- test_denoise_temporal_gpu.py's PATH_COUNTERS)
    path_counters = ("rays", "paths", "bounces", "shadow", "hits", "walked")
    assert counters1["paths"] == 21 * R.W * R.H
    assert all(counters1[k] == counters0[k] for k in path_counters), f"counters with the call {counters1}, without {counters0}"


# ------------------------------------------------------------------ 6. the device form
def _device(renderer, rays, keys, n_samples=1, planes=None, stream=None):
    import torch
    dev = f"cuda:{renderer.device}"
    t = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to(dev)
    k = None if keys is None else torch.from_numpy(keys.view(np.uint32).reshape(-1, 4).view(np.int32).copy()).to(dev)
    keep = t.clone()
    if stream is None:
        out = renderer.radiance_rays(rays=t, keys=k, n_samples=n_samples, planes=planes)
        torch.cuda.current_stream(t.device).synchronize()
    else:
        stream.wait_stream(torch.cuda.current_stream(t.device))
        with torch.cuda.stream(stream):
            out = renderer.radiance_rays(rays=t, keys=k, n_samples=n_samples, planes=planes)
        stream.synchronize()
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), "the device form wrote to its input"
    assert all(v.device == t.device for v in out.values())
    return {p: v.cpu().numpy() for p, v in out.items()}


def test_device_form_equals_the_host_form(renderer, orc):
    import torch
    from computeraytracer_amd.renderer import pack_keys, pack_rays
    ps, o, d, keys, want = both(orc, "sphere")
    renderer.upload(ps).build_accel("ploc")
    rays, k = pack_rays(o, d), pack_keys(keys[:, 0], keys[:, 1], keys[:, 2])
    host = renderer.radiance_rays(rays=rays, keys=k)
    check(host, want, "host form")
    cur = _device(renderer, rays, k)
    side = _device(renderer, rays, k, stream=torch.cuda.Stream(device=renderer.device))
    for name, got in (("current stream", cur), ("second stream", side)):
        assert sorted(got) == sorted(host)
        for p in host:
            assert got[p].dtype == host[p].dtype and np.array_equal(got[p].view(np.uint8), host[p].view(np.uint8)), f"{p} on the {name}"
    part = _device(renderer, rays, k, n_samples=3, planes=("y2",))
    assert list(part) == ["y2"] and np.array_equal(bits(part["y2"]), bits(renderer.radiance_rays(rays=rays, keys=k, n_samples=3)["y2"]))
    # keys = None is (i, 0, 1), in both forms
    n = len(rays)
    default = pack_keys(np.arange(n), 0, 1)
    h_none, h_def = renderer.radiance_rays(rays=rays), renderer.radiance_rays(rays=rays, keys=default)
    d_none, d_def = _device(renderer, rays, None), _device(renderer, rays, default)
    assert not np.array_equal(bits(h_none["xyz"]), bits(host["xyz"])), "vacuous: the keys do not matter"
    for p in h_none:
        for other in (h_def, d_none, d_def):
            assert np.array_equal(h_none[p].view(np.uint8), other[p].view(np.uint8)), p
    assert {p: v.shape for p, v in _device(renderer, rays[:0], None).items()} == {"xyz": (0, 4), "y2": (0,), "rgba8": (0, 4)}
    # refusals of the tensor form
    dev = f"cuda:{renderer.device}"
    with pytest.raises(ValueError, match="contiguous"):
        renderer.radiance_rays(rays=torch.zeros((4, 7), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="the context on"):
        renderer.radiance_rays(rays=torch.zeros((4, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="keys must be"):
        renderer.radiance_rays(rays=torch.zeros((4, 8), dtype=torch.float32, device=dev), keys=np.zeros((4, 4), np.uint32))
    with pytest.raises(ValueError, match="keys must be"):
        renderer.radiance_rays(rays=torch.zeros((4, 8), dtype=torch.float32, device=dev), keys=torch.zeros((4, 3), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="keys must be"):
        renderer.radiance_rays(rays=torch.zeros((4, 8), dtype=torch.float32, device=dev), keys=torch.zeros((4, 4), dtype=torch.float32, device=dev))


# ------------------------------------------------------------------ 7. the first segment
@pytest.mark.parametrize("builder", ("bvh2", "none"))
def test_first_segment_limit_and_exclude(renderer, orc, builder):
    ps, o, d, keys, want = both(orc, "tri")
    renderer.upload(ps).build_accel(builder)
    n = len(o)
    fin = want["finite"]
    base = renderer.radiance_rays(o, d, keys)
    check(base, want, f"tri / {builder}")
    q = renderer.query_rays(o, d, planes=("hit", "prim", "t"))
    hit = (q["hit"] == 1) & fin
    assert hit.sum() > 800 and ((q["hit"] == 0) & fin).sum() > 50
    # the oracle's value of a path whose first segment misses: every miss of the set agrees on it
    miss = np.flatnonzero((q["hit"] == 0) & fin)
    zero = {p: raw(base[p][miss[:1]]) for p in base}
    assert all((raw(base[p][miss]) == zero[p]).all() for p in base) and not zero["xyz"].any() and not zero["y2"].any()

    def same(a, b, sel, what):
        for p in a:
            assert np.array_equal(raw(a[p][sel]), raw(b[p][sel])), f"{what}: {p}"

    def is_miss(g, sel, what):
        for p in g:
            assert (raw(g[p][sel]) == zero[p]).all(), f"{what}: {p} is not a missed path's"

    # a limit that cannot bite: the hit's own t (the end is inclusive), anything above it, +inf
    t = q["t"]
    for name, L in (("t_max = t", t), ("t_max = 2 t", (t * F(2)).astype(F)), ("t_max = +inf", np.full(n, np.inf, F))):
        same(renderer.radiance_rays(o, d, keys, t_max=L), base, fin, name)
    # just below the hit: the first segment misses
    below = np.nextafter(t, F(0)).astype(F)
    g = renderer.radiance_rays(o, d, keys, t_max=below)
    assert not renderer.query_rays(o, d, t_max=below, planes=("hit",))["hit"][hit].any()
    is_miss(g, hit, "t_max just below the hit")
    same(g, base, (q["hit"] == 0) & fin, "t_max below nothing")
    # a NaN or negative limit: a miss
    for name, v in (("NaN", np.nan), ("negative", -1.0), ("-inf", -np.inf)):
        is_miss(renderer.radiance_rays(o, d, keys, t_max=np.full(n, v, F)), fin, f"t_max {name}")
    # an exclude that cannot bite: a primitive the first segment does not end on
    other = np.where(q["prim"] == 0, 1, 0).astype(np.uint32)
    same(renderer.radiance_rays(o, d, keys, exclude=other), base, fin, "exclude of another primitive")
    # the first hit excluded: the first segment's hit is crt_query_rays' -- where that misses, a missed path; where it
    # ends on a light, that light's spectrum at the key's wavelengths, which any path that sees it first agrees on
    ex = np.where(hit, q["prim"], MAXU).astype(np.uint32)
    g = renderer.radiance_rays(o, d, keys, exclude=ex)
    q2 = renderer.query_rays(o, d, exclude=ex, planes=("hit", "prim"))
    gone = hit & (q2["hit"] == 0)
    assert gone.sum() > 50, "vacuous: behind every first hit lies another primitive"
    is_miss(g, gone, "exclude = the first hit, nothing behind it")
    same(g, base, (q["hit"] == 0) & fin, "exclude = nothing")
    changed = hit & (q2["hit"] == 1) & (q2["prim"] != q["prim"])
    assert changed.sum() > 100 and (bits(g["xyz"][changed]) != bits(base["xyz"][changed])).any(axis=1).sum() > 50
    # both at once, per ray, mixed in one batch
    mix_L = np.where(np.arange(n) % 2 == 0, below, R.NO_LIMIT).astype(F)
    mix_E = np.where(np.arange(n) % 3 == 0, ex, MAXU).astype(np.uint32)
    gm = renderer.radiance_rays(o, d, keys, t_max=mix_L, exclude=mix_E)
    qm = renderer.query_rays(o, d, t_max=mix_L, exclude=mix_E, planes=("hit", "prim"))
    is_miss(gm, fin & (qm["hit"] == 0), "mixed batch, missed")
    same(gm, base, fin & (qm["hit"] == 1) & (qm["prim"] == q["prim"]) & (q["hit"] == 1), "mixed batch, unchanged first hit")


@pytest.mark.parametrize("builder", ("bvh2", "lbvh", "none"))
def test_an_excluded_first_hit_with_a_light_behind_it(renderer, orc, builder):
    """The exact case of the first-segment extensions (radiance_ref.behind_the_ceiling): straight down through the
    excluded ceiling onto a triangle light, with the key of a ray that sees a light of that emission first."""
    ps, o, d, ex, keys, xyz, ceiling, lights = R.behind_the_ceiling(orc)
    renderer.upload(ps).build_accel(builder)
    q = renderer.query_rays(o, d, exclude=ex, planes=("hit", "prim"))
    assert q["hit"].all() and sorted(set(q["prim"].tolist())) == lights
    assert (renderer.query_rays(o, d, planes=("prim",))["prim"] == ceiling).all()
    got = renderer.radiance_rays(o, d, keys, exclude=ex)
    with np.errstate(invalid="ignore"):
        want = (F(0.0) + xyz).astype(F)
    bad = np.flatnonzero((bits(got["xyz"][:, :3]) != bits(want)).any(axis=1))
    assert not len(bad), f"{builder}: {len(bad)} of {len(o)} rays; first {int(bad[0])}: kernel {got['xyz'][bad[0]].tolist()}, oracle {want[bad[0]].tolist()}"
    assert np.array_equal(bits(got["y2"]), bits(R.y2_of(want))) and np.array_equal(got["rgba8"], R.oracle_rgba8(orc, got["xyz"], 1))
    # without the exclude the path starts on the ceiling instead, and a limit that ends before the light is a miss
    plain = renderer.radiance_rays(o, d, keys)
    assert (bits(plain["xyz"][:, :3]) != bits(want)).any(axis=1).sum() > len(o) // 2
    cut = renderer.radiance_rays(o, d, keys, exclude=ex, t_max=np.full(len(o), 45.5, F))
    assert not cut["xyz"].view(np.uint32).any()


@pytest.mark.parametrize("builder", ("bvh2", "ploc", "none"))
def test_paths_that_reach_the_depth_cap(renderer, orc, builder):
    """radiance_ref.DEEP: inside the glass sphere most paths are reflected back for ever and end at kMaxDepthPath."""
    ps, rs = R.deep_rays(orc)
    renderer.upload(ps).build_accel(builder)
    assert (rs.segments == 101).sum() >= 100 and rs.finite.all()
    e = R.expected(rs)
    keys = np.concatenate([rs.keys, np.zeros((len(rs.keys), 1), np.uint32)], axis=1)
    want = dict(xyz=e.xyz, y2=e.y2, rgba8=e.rgba8, has8=e.has8, finite=rs.finite)
    check(renderer.radiance_rays(rs.o, rs.d, keys), want, f"deep / {builder}")
    # two samples per ray: the second path starts after a first that ran to the cap
    two = renderer.radiance_rays(rs.o, rs.d, keys, n_samples=2, planes=("xyz",))
    k2 = keys.copy()
    k2[:, 2] += 1
    nxt = renderer.radiance_rays(rs.o, rs.d, k2, planes=("xyz",))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits(two["xyz"][:, :3]), bits((e.xyz + nxt["xyz"][:, :3]).astype(F)))


@pytest.mark.parametrize("builder", ("bvh2", "none"))
def test_non_finite_caller_rays_give_zeros(renderer, orc, builder):
    ps, o, d, keys, want = both(orc, "sphere")
    renderer.upload(ps).build_accel(builder)
    k = np.flatnonzero(want["finite"])[:30]
    base = renderer.radiance_rays(o[k], d[k], keys[k], n_samples=2)
    assert base["rgba8"][:, 3].all() and base["xyz"].any()
    bo, bd = o[k].copy(), d[k].copy()
    for j, v in enumerate([np.inf, -np.inf, np.nan, 3.0e38, -3.0e38] * 6):
        (bo, bd)[j % 2][j, (j // 2) % 3] = v
    got = renderer.radiance_rays(bo, bd, keys[k], n_samples=2)
    for p in got:
        assert not got[p].view(np.uint8).any(), f"{p} of a non-finite ray is not zero"
    # between good rays, each keeps its own
    mo, md = o[k].copy(), d[k].copy()
    mo[::3], md[::3] = bo[::3], bd[::3]
    mixed = renderer.radiance_rays(mo, md, keys[k], n_samples=2)
    good = np.arange(30) % 3 != 0
    for p in mixed:
        assert not mixed[p][~good].view(np.uint8).any() and np.array_equal(mixed[p][good].view(np.uint8), base[p][good].view(np.uint8)), p
    # the largest finite-by-the-rule magnitude is walked
    assert renderer.radiance_rays(np.full((1, 3), 2.9e38, F), d[k[:1]], keys[k[:1]])["rgba8"][0, 3] == 255


# ------------------------------------------------------------------ 8. the camera
def test_the_context_camera_does_not_enter(renderer, orc):
    ps, o, d, keys, want = both(orc, "tri_only")
    renderer.upload(ps).build_accel("bvh2")
    pad = renderer.debug_hit_pad
    check(renderer.radiance_rays(o, d, keys), want, "tri_only, probe 0's camera")
    renderer.set_camera(R.with_probe(ps, R.PROBES[1]).camera)
    assert renderer.debug_hit_pad == pad
    check(renderer.radiance_rays(o, d, keys), want, "tri_only, probe 1's camera")
    # neither do the tile, the sample offset or samples already traced
    try:
        renderer.set_sample_offset(11)
        renderer.set_tile(8, 8, 16, 24)
        renderer.frame(2).sync()
        check(renderer.radiance_rays(o, d, keys), want, "tri_only, under a tile and a sample offset, at sample 2")
    finally:
        renderer.set_tile(0, 0, R.W, R.H)
        renderer.upload(ps)                                      # (returns the offset to 0)


# ------------------------------------------------------------------ 9. refusals
def _raw(r, rays, keys, n, n_samples, planes, device=False):
    from computeraytracer_amd import _lib
    p = None if planes is None else _lib.RadiancePlanes(**{k: (v if isinstance(v, int) else v.ctypes.data) for k, v in planes.items()})
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data
    arg = None if p is None else C.byref(p)
    if device:
        return r._lib.crt_radiance_rays_device(r._h, ptr(rays), ptr(keys), n, n_samples, arg, None)
    return r._lib.crt_radiance_rays(r._h, ptr(rays), ptr(keys), n, n_samples, arg)


def test_refusals(orc):
    from computeraytracer_amd import Renderer
    from computeraytracer_amd._lib import CrtError
    from computeraytracer_amd.renderer import pack_keys, pack_rays
    ps, o, d, keys, want = both(orc, "patch")
    rays, k = pack_rays(o[:8], d[:8]), pack_keys(keys[:8, 0], keys[:8, 1], keys[:8, 2])
    xyz, y2, rgba = np.full((9, 4), -7.0, F), np.full(8, -7.0, F), np.full((8, 4), 9, np.uint8)
    with Renderer(0) as r:
        err = lambda: r._lib.crt_last_error(r._h)
        for _ in range(2):                                       # no scene; a scene without a tree
            for dev in (False, True):
                assert _raw(r, rays, k, 8, 1, dict(xyz=xyz), dev) == ESTATE and b"scene + accel required" in err()
            r.upload(ps)
        r.build_accel("bvh2")
        for dev in (False, True):
            assert _raw(r, rays, k, 8, 1, None, dev) == EINVAL and b"out is NULL" in err()
            assert _raw(r, rays, k, 8, 1, {}, dev) == EINVAL and b"every plane is NULL" in err()
            assert _raw(r, None, k, 8, 1, dict(xyz=xyz), dev) == EINVAL and b"rays is NULL" in err()
            assert _raw(r, rays.ctypes.data + 4, k, 7, 1, dict(xyz=xyz), dev) == EINVAL and b"16-byte aligned" in err()
            assert _raw(r, rays, k.ctypes.data + 4, 7, 1, dict(xyz=xyz), dev) == EINVAL and b"16-byte aligned" in err()
            assert _raw(r, rays, k, 8, 1, dict(xyz=xyz.ctypes.data + 4), dev) == EINVAL and b"16-byte aligned" in err()
            assert _raw(r, rays, k, 1 << 32, 1, dict(xyz=xyz), dev) == EINVAL and b"2^32" in err()
            assert _raw(r, rays, k, 8, 0, dict(xyz=xyz), dev) == EINVAL and b"n_samples" in err()
            assert _raw(r, rays, k, 0, 1, dict(xyz=xyz), dev) == 0          # n == 0 succeeds and does nothing
            assert _raw(r, None, None, 0, 1, dict(y2=y2), dev) == 0
        assert (xyz == -7.0).all() and (y2 == -7.0).all() and (rgba == 9).all()
        # y2 and rgba8 need no alignment; each plane alone
        assert _raw(r, rays, k, 8, 1, dict(y2=y2.ctypes.data + 4, rgba8=rgba.ctypes.data + 4)) == 0
        assert _raw(r, rays, k, 8, 1, dict(xyz=xyz, y2=y2, rgba8=rgba)) == 0
        assert np.array_equal(bits(xyz[:8, :3]), bits(want["xyz"][:8])) and (xyz[8] == -7.0).all() and (rgba[:, 3] == 255).all()
        # a stale tree
        r.update_primitives(0, r.read_primitives(0, 1))
        for dev in (False, True):
            assert _raw(r, rays, k, 8, 1, dict(xyz=xyz), dev) == ESTATE and b"crt_refit_accel" in err()
        with pytest.raises(CrtError, match="crt_refit_accel"):
            r.radiance_rays(o[:8], d[:8], keys[:8])
        r.refit_accel()
        check(r.radiance_rays(o, d, keys), want, "after the refit")


def test_failed_allocations_leave_nothing_behind(orc):
    """Each staging allocation of a fresh context's first crt_radiance_rays fails in turn: CRT_ENOMEM, the outputs as
    prefilled, and the next call correct."""
    from computeraytracer_amd import Renderer
    from computeraytracer_amd.renderer import pack_keys, pack_rays
    ps, o, d, keys, want = both(orc, "patch")
    rays, k = pack_rays(o, d), pack_keys(keys[:, 0], keys[:, 1], keys[:, 2])
    n = len(rays)
    failed, done = 0, False
    for nth in range(1, 12):
        with Renderer(0) as r:
            r.upload(ps).build_accel("bvh2")
            out = dict(xyz=np.full((n, 4), 0x5A5A5A5A, np.uint32), y2=np.full(n, 0x5A5A5A5A, np.uint32), rgba8=np.full((n, 4), 0x5A, np.uint8))
            try:
                r.set_option("debug_fail_alloc", nth)
                rc = _raw(r, rays, k, n, 1, out)
            finally:
                r.set_option("debug_fail_alloc", 0)
            if rc == 0:
                check(dict(xyz=out["xyz"].view(F), y2=out["y2"].view(F), rgba8=out["rgba8"]), want, "the call no allocation of which fails")
                done = True
                break
            assert rc == ENOMEM, (nth, rc, r._lib.crt_last_error(r._h))
            failed += 1
            assert (out["xyz"] == 0x5A5A5A5A).all() and (out["y2"] == 0x5A5A5A5A).all() and (out["rgba8"] == 0x5A).all(), \
                f"allocation {nth} failed and the call wrote to its outputs"
            check(r.radiance_rays(rays=rays, keys=k), want, f"the call after allocation {nth} failed")
    assert done and failed == 5, f"{failed} allocations failed in turn; the call makes 5 (the rays, the keys, three planes)"


def test_staging_grows_by_half_and_is_released_by_an_upload(orc):
    from computeraytracer_amd import Renderer
    ps, o, d, keys, want = both(orc, "patch")
    with Renderer(0) as r:
        r.upload(ps).build_accel("bvh2")
        r.radiance_rays(o[:100], d[:100], keys[:100])
        # 101 rays grow each buffer to 150: the next 150 allocate nothing, so a failing "next allocation" never fires
        r.radiance_rays(o[:101], d[:101], keys[:101])
        try:
            r.set_option("debug_fail_alloc", 1)
            check(r.radiance_rays(o[:150], d[:150], keys[:150]), want, "150 rays in buffers grown by half", np.arange(150))
        finally:
            r.set_option("debug_fail_alloc", 0)
        r.upload(ps).build_accel("bvh2")                         # releases the staging: the next call allocates again
        r.set_option("debug_fail_alloc", 1)
        try:
            from computeraytracer_amd._lib import CrtError
            with pytest.raises(CrtError) as e:
                r.radiance_rays(o[:10], d[:10], keys[:10])
            assert e.value.code == ENOMEM
        finally:
            r.set_option("debug_fail_alloc", 0)


def test_panorama(renderer, orc):
    ps = R.scene("patch")
    renderer.upload(ps).build_accel("bvh2")
    xyz, rgba = renderer.panorama(32, 16, (278, 273, 280), n_samples=4, first_sample=3)
    assert xyz.shape == (16, 32, 4) and rgba.shape == (16, 32, 4) and xyz.dtype == F and rgba.dtype == np.uint8
    rays, keys = renderer.panorama_rays(32, 16, (278, 273, 280), 3)
    again = renderer.radiance_rays(rays=rays, keys=keys, n_samples=4)
    assert np.array_equal(bits(again["xyz"]), bits(xyz.reshape(-1, 4))) and np.array_equal(again["rgba8"], rgba.reshape(-1, 4))
    # from the middle of the box, which is open at the front only, five directions of six end on a wall, and the walls are lit
    assert (rgba[..., 3] == 255).all() and np.isfinite(xyz).all()
    seen = renderer.query_rays(rays=rays, planes=("hit",))["hit"].reshape(16, 32) == 1
    assert 0.7 < seen.mean() < 0.95 and not xyz[~seen][:, :3].any() and (xyz[seen][:, 1] > 0).mean() > 0.5
    assert not seen[:, :4].all() and seen[:, 12:20].all(), "the open front is behind the viewer (-z): the image's left and right edges"
