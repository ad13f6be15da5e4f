"""GPU tests of crt_accel_quality and option "refit_rebuild_pct" (include/crt.h "Scene edits"; run with -m gpu
on an MI355X).

  1 kernel    the four values against accel_quality_ref.py (a numpy float64 restatement, anchored on the CPU by
              test_accel_quality_cpu.py) evaluated on the nodes read back with crt_debug_read_accel: every builder, float
              and quantised 4-wide trees, node counts on both sides of a 64-lane wave and of a 256-thread block, more than
              256 blocks (the second stage loops), one-leaf trees, the 8-wide case; a second call returns the same bits
  2 refit     a stale tree shows its old boxes; after the refit the current values follow the re-read nodes, the as-built
              ones stay bit for bit, the refits are counted, crt_build_accel starts over
  3 policy    with P above the measured ratio a refit stays a refit, with P below it the tree is rebuilt by the builder
              that made it, and what lies on the device then is what crt_build_accel makes of the same records
  4 option    values outside 0, 100..100000 are refused and leave the context usable
  5 camera    the refit inside crt_set_camera does not apply the policy

The tolerance of every comparison with the restatement.  Both sides evaluate the same float64 expression per term on
the same inputs; the terms are >= 0.  A sum of N non-negative terms in any order has a relative error of at most
(N - 1) u, u = 2^-53, so two orders differ by at most 2 (N - 1) u = (N - 1) 2^-52 relative.  Within a term the two sides
may differ by a fused multiply-add (A has two additions and three products, the weight one more product: under 6 u), and
each side divides once (u each): 8 x 2^-52 covers that.  Hence |device - restatement| <= (N + 8) 2^-52 x restatement, N the
number of terms of that sum: nodes for `boxes`, leaf children for `prims`."""
import math

import numpy as np
import pytest

import accel_quality_ref as QR
from conftest import bits

pytestmark = pytest.mark.gpu

DEFAULTS = dict(pipeline=1, quantize=1, wf_width=4, wf_trace_form=2, refit_rebuild_pct=0)
BUILDER = {"bvh2": "sah-host", "lbvh": "lbvh-gpu", "ploc": "ploc-gpu"}
CRT_EINVAL = -1


@pytest.fixture(scope="module")
def r():
    from computeraytracer_amd import Renderer
    ctx = Renderer(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def other():
    """A second context: the fresh upload and build that a rebuilt tree is compared with."""
    from computeraytracer_amd import Renderer
    ctx = Renderer(0)
    yield ctx
    ctx.close()


def options(ctx, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        ctx.set_option(k, v)


_SCENES = {}


def soup(n, w=64, h=64):
    """scenes_synth.soup: the six Cornell walls and n random triangles."""
    if (n, w, h) not in _SCENES:
        from computeraytracer_amd.scenes_synth import soup as make
        _SCENES[(n, w, h)] = make(n, w, h)
    return _SCENES[(n, w, h)]


def few(k):
    """k = 1: the light patch alone (no tree has an inner node); k = 3: the first three patches, the light among them (a
    4-wide root with an empty slot and nothing below it)."""
    from computeraytracer_amd.scene import PackedScene, lights_of
    ps = soup(1)
    prims = (ps.primitives[2:3] if k == 1 else ps.primitives[:k]).copy()
    prims["data4"][:, 3] = np.arange(len(prims), dtype=np.uint32)
    lights = lights_of(prims)
    assert len(lights) == 1
    return PackedScene(prims, lights, ps.camera, ps.spectra, ps.cie)


def cornell64():
    """The Cornell box: patches and both spheres."""
    from computeraytracer_amd import cornell
    return cornell(64, 64)


def with_records(ps, prims):
    from computeraytracer_amd.scene import PackedScene
    return PackedScene(prims, ps.lights, ps.camera, ps.spectra, ps.cie)


def tol(n):
    return (n + 8) * 2.0 ** -52


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def assert_close(got, want, terms, what):
    for k in range(4):
        print(f"{what}: [{k}] device {got[k]!r} restatement {want[k]!r} terms {terms[k]}")
        if np.isnan(want[k]):
            assert np.isnan(got[k]), (what, k, got[k])
        elif want[k] == 0.0:
            assert got[k] == 0.0, (what, k, got[k])
        else:
            assert np.isfinite(want[k]) and want[k] > 0.0, (what, k, want[k])
            assert abs(got[k] - want[k]) <= tol(terms[k]) * want[k], (what, k, got[k], want[k], abs(got[k] - want[k]) / want[k], tol(terms[k]))


def restated(ctx):
    A = ctx.debug_read_accel()
    want, terms, has4 = QR.quality(A)
    return A, want, terms, has4


def move_tenth(ps, shift=(600.0, 300.0, 0.0), thirds=1):
    """One op: a contiguous tenth of the primitives, starting `thirds` thirds of the way in, moved far away."""
    n = len(ps.primitives)
    return [(thirds * n // 3, n // 10, np.hstack([np.eye(3), np.asarray(shift, np.float64)[:, None]]))]


# ------------------------------------------------------------------ 1. the kernel against the restatement
# soup(n) holds n + 6 primitives.  An LBVH / PLOC tree has one inner node less than primitives: 59, 60, 251 and 252 give 64,
# 65, 256 and 257 inner nodes; the other sizes put the SAH builder's and the 4-wide trees' counts elsewhere around them.
SOUPS = [1, 2, 5, 59, 60, 65, 251, 252, 256, 257, 258]
SCENES = {**{f"soup{n}": (lambda n=n: soup(n)) for n in SOUPS}, "one": lambda: few(1), "three": lambda: few(3),
          "cornell": lambda: cornell64()}
CASES = [(s, b) for s in SCENES for b in BUILDER] + [("soup70001", "lbvh"), ("soup70001", "ploc")]
SCENES["soup70001"] = lambda: soup(70001)


@pytest.mark.parametrize("scene, builder", CASES)
def test_values_equal_the_restatement(r, scene, builder):
    ps = SCENES[scene]()
    try:
        for quantize in (1, 0):
            what = f"{scene} / {builder} / quantize={quantize}"
            options(r, quantize=quantize)
            r.upload(ps).build_accel(builder)
            A, want, terms, has4 = restated(r)
            n = len(ps.primitives)
            if scene == "one":
                assert A["n2"] == 0 and A["n4"] == 0, what                   # one leaf
            else:
                assert A["n2"] >= 1 and A["n4"] >= 1 and has4, what
                assert (A["live4q"], A["live4"] or A["device_route"]) == ((1, 1) if quantize else (0, 1)), (what, A["live4q"], A["live4"])
                assert terms[0] == A["n2"] and terms[2] == A["n4"] and terms[1] >= 1 and terms[3] >= 1
                if builder != "bvh2" and n >= 2:
                    assert r.accel_stats()["builder"] == BUILDER[builder] and A["n2"] == n - 1 and terms[1] == terms[3] == n, what
            if scene == "soup70001":
                assert A["n2"] > 256 * 256 and (A["n4"] + 255) // 256 > 1, what   # the second stage loops over its input
            raw = r.accel_quality()["raw"]
            assert_close(raw[0:4], want, terms, what)
            assert same_bits(raw[4:8], raw[0:4]), (what, raw)
            assert raw[8] == 0 and raw[10] == 1 and raw[11] == 0, (what, raw)
            again = r.accel_quality()["raw"]
            assert same_bits(again, raw), (what, raw, again)
            if A["n2"] == 0:
                assert same_bits(raw[0:8], np.zeros(8)), (what, raw)
    finally:
        options(r)


def test_no_structure_and_no_tree(r):
    from computeraytracer_amd._lib import CrtError
    ps = soup(5)
    options(r)
    r.upload(ps)
    with pytest.raises(CrtError) as e:
        r.accel_quality()
    assert e.value.code == -3 and "accel" in str(e.value)        # CRT_ESTATE
    r.build_accel("none")
    raw = r.accel_quality()["raw"]
    assert same_bits(raw[0:8], np.zeros(8)) and raw[8] == 0 and raw[10] == 1, raw
    assert r.refit_accel() is False and r.accel_quality()["raw"][8] == 0


@pytest.mark.parametrize("builder", ["bvh2", "lbvh"])
def test_the_8_wide_tree_has_no_4_wide_values(r, builder):
    ps = soup(257)
    try:
        options(r, wf_width=8)
        r.upload(ps).build_accel(builder)
        A, want, terms, has4 = restated(r)
        assert A["live8q"] == 1 and not has4 and r.accel_stats()["width"] == 8
        q = r.accel_quality()
        raw = q["raw"]
        assert_close(raw[0:4], want, terms, f"soup257 / {builder} / wf_width=8")
        assert np.isnan(raw[2:4]).all() and np.isnan(raw[6:8]).all() and raw[10] == 0 and q["has4"] is False
        assert same_bits(raw[4:6], raw[0:2])
        assert same_bits(r.accel_quality()["raw"], raw)
        # a refit of an 8-wide tree is a rebuild: nothing counts as a refit, and the policy has nothing finite to compare
        r.set_option("refit_rebuild_pct", 100)
        r.transform_primitives(move_tenth(ps))
        assert r.refit_accel() is True
        raw = r.accel_quality()["raw"]
        assert raw[8] == 0 and raw[9] == q["rebuilds"] and raw[10] == 0
    finally:
        options(r)


# ------------------------------------------------------------------ 2. refit
@pytest.mark.parametrize("builder, quantize, first_asked", [("lbvh", 1, "built"), ("lbvh", 1, "stale"), ("lbvh", 1, "refitted"),
                                                            ("ploc", 1, "refitted"), ("bvh2", 1, "stale"), ("bvh2", 0, "built"),
                                                            ("lbvh", 0, "refitted")])
def test_refit_moves_the_current_values_only(r, builder, quantize, first_asked):
    """first_asked: when crt_accel_quality is called first -- on the tree as built, on the stale tree (both take the
    as-built values there), or only after the refit (they were taken by the refit's once-per-tree set-up)."""
    ps = soup(4099)
    what = f"soup4099 / {builder} / quantize={quantize} / first asked when {first_asked}"
    try:
        options(r, quantize=quantize)
        r.upload(ps).build_accel(builder)
        A0, want0, terms0, _ = restated(r)
        raw0 = r.accel_quality()["raw"] if first_asked == "built" else None
        r.transform_primitives(move_tenth(ps))
        As = r.debug_read_accel()
        assert As["stale"] == 1
        for k in ("nodes2", "nodes4", "nodes4q"):
            assert np.array_equal(As[k].view(np.uint32), A0[k].view(np.uint32)), (what, k)
        if first_asked in ("built", "stale"):
            raws = r.accel_quality()["raw"]                      # works on a stale tree, shows the old boxes
            assert_close(raws[0:4], want0, terms0, what + " / stale")
            assert same_bits(raws[4:8], raws[0:4]) and raws[8] == 0, (what, raws)
            assert raw0 is None or same_bits(raws, raw0), (what, raw0, raws)
            raw0 = raws
        assert r.refit_accel() is False
        A1, want1, terms1, _ = restated(r)
        assert terms1 == terms0 and A1["stale"] == 0
        raw1 = r.accel_quality()["raw"]
        assert_close(raw1[0:4], want1, terms1, what + " / refitted")
        assert_close(raw1[4:8], want0, terms0, what + " / as built")
        assert raw0 is None or same_bits(raw1[4:8], raw0[0:4]), (what, raw0, raw1)
        assert raw1[8] == 1, (what, raw1)
        # the values moved where, and in the direction, the restatement says: the boxes of the nodes that now span the
        # gap grew against the root's, the leaves' shrank against it
        assert want1[0] > want0[0] and want1[2] > want0[2] and want1[1] < want0[1] and want1[3] < want0[3], (what, want0, want1)
        for k in range(4):
            assert (raw1[k] > raw1[4 + k]) == (want1[k] > want0[k]) and (raw1[k] < raw1[4 + k]) == (want1[k] < want0[k]), (what, k, raw1)
        assert r.refit_accel() is False
        raw2 = r.accel_quality()["raw"]
        assert raw2[8] == 2 and same_bits(raw2[0:8], raw1[0:8]), (what, raw1, raw2)
        r.build_accel(builder)                                   # starts over: [4..8]
        Af, wantf, termsf, _ = restated(r)
        rawf = r.accel_quality()["raw"]
        assert_close(rawf[0:4], wantf, termsf, what + " / built again")
        assert same_bits(rawf[4:8], rawf[0:4]) and rawf[8] == 0, (what, rawf)
        assert not same_bits(rawf[4:8], raw1[4:8]), (what, rawf, raw1)
    finally:
        options(r)


# ------------------------------------------------------------------ 3. the policy
def canonical4q(nodes4q):
    """A quantised 4-wide node array renumbered breadth-first from the root with the children in slot order.  The device
    collapse numbers the nodes of one level in the order its threads arrive (an atomic counter), so two builds of the same
    records give the same tree under two numberings; this is the tree without the numbering."""
    nd = np.ascontiguousarray(nodes4q, np.uint32).reshape(-1, 16)
    refs = nd[:, 12:16].copy().view(np.int32)
    order, at = [0], 0                                           # (the root is node 0: the caller asserts root4 == 0)
    while at < len(order):
        order += [int(c) for c in refs[order[at]] if c > 0]
        at += 1
    assert sorted(order) == list(range(len(nd))), "not every node is reached once from the root"
    newid = np.zeros(len(nd), np.int32)
    newid[order] = np.arange(len(nd), dtype=np.int32)
    out = nd[order].copy()
    r = refs[order]
    out[:, 12:16] = np.where(r > 0, newid[np.maximum(r, 0)], r).astype(np.int32).view(np.uint32)
    return out


def frame(ctx):
    ctx.frame(2).sync()
    return ctx.read_accum(), ctx.read_rgba8()


@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
def test_policy_rebuilds_past_the_threshold_only(r, other, builder):
    ps = soup(4099, 32, 32)
    try:
        options(r)
        options(other)
        r.upload(ps).build_accel(builder)
        A0, want0, terms0, _ = restated(r)
        assert A0["live4q"] == 1 and A0["device_route"] == 1
        rebuilds0 = r.accel_quality()["rebuilds"]
        r.transform_primitives(move_tenth(ps))
        assert r.refit_accel() is False                          # P = 0 never rebuilds
        A1, want1, terms1, _ = restated(r)
        ratio = (want1[2] + want1[3]) / (want0[2] + want0[3])     # Q of the walked tree: the 4-wide one
        q = r.accel_quality()
        print(f"soup4099 / {builder}: Q built {want0[2] + want0[3]!r}, refitted {want1[2] + want1[3]!r}, ratio {ratio!r}; device {q['q_built']!r}, {q['q_now']!r}")
        assert ratio >= 1.05, ratio
        assert abs(q["q_now"] / q["q_built"] - ratio) <= 1e-9 * ratio
        assert q["refits"] == 1 and q["rebuilds"] == rebuilds0
        moved = r.read_primitives()

        r.set_option("refit_rebuild_pct", math.ceil(100 * ratio) + 1)
        assert r.refit_accel() is False
        q = r.accel_quality()
        assert q["refits"] == 2 and q["rebuilds"] == rebuilds0
        assert np.array_equal(r.debug_read_accel()["nodes4q"], A1["nodes4q"])

        r.set_option("refit_rebuild_pct", max(100, math.floor(100 * ratio) - 1))
        assert r.refit_accel() is True
        assert r.accel_stats()["builder"] == BUILDER[builder]
        q = r.accel_quality()
        assert q["refits"] == 0 and q["rebuilds"] == rebuilds0 + 1, q
        assert same_bits(q["raw"][4:8], q["raw"][0:4])
        Ar, wantr, termsr, _ = restated(r)
        assert_close(q["raw"][0:4], wantr, termsr, f"soup4099 / {builder} / rebuilt by the policy")
        assert wantr[2] + wantr[3] < want1[2] + want1[3]         # what the rebuild is for
        assert np.array_equal(r.read_primitives().view(np.uint8), moved.view(np.uint8))
        assert r.refit_accel() is False                          # a fresh tree is not past its own cost (P >= 100)
        assert r.accel_quality()["rebuilds"] == rebuilds0 + 1
        got = frame(r)

        # bit for bit the image of a fresh upload and build of the records as they lie on the device
        other.upload(with_records(ps, moved)).build_accel(builder)
        acc, rgba = frame(other)
        assert np.array_equal(bits(got[0])[..., :3], bits(acc)[..., :3]) and np.array_equal(got[1], rgba)
        # and, part for part, the structure of an explicit crt_build_accel of the same records (the 4-wide nodes up to
        # their numbering within a level, which no two device builds share: canonical4q)
        r.set_option("refit_rebuild_pct", 0)
        r.build_accel(builder)
        Ab = r.debug_read_accel()
        assert Ab.keys() == Ar.keys() and Ar["root4"] == 0 and Ab["root4"] == 0
        for k in Ab:
            if k == "overflow_allocated":                        # (the walks' stack area, allocated by the first trace: no part of the tree)
                continue
            a, b = (canonical4q(Ar[k]), canonical4q(Ab[k])) if k == "nodes4q" else (np.asarray(Ar[k]), np.asarray(Ab[k]))
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{builder}: part {k} differs after the policy's rebuild"

        # P = 0 never rebuilds, however far the tree has decayed
        r.transform_primitives(move_tenth(ps, (0.0, 2500.0, 1500.0), thirds=2))      # (another tenth, another way)
        assert r.refit_accel() is False
        q = r.accel_quality()
        assert q["q_now"] > 1.05 * q["q_built"] and q["refits"] == 1 and q["rebuilds"] == rebuilds0 + 1
    finally:
        options(r)
        options(other)


# ------------------------------------------------------------------ 4. the option's range
def test_option_range(r):
    from computeraytracer_amd._lib import CrtError
    options(r)
    r.upload(soup(65)).build_accel("lbvh")
    assert r.refit_accel() is False
    before = r.accel_quality()["raw"]
    assert before[8] == 1
    for bad in (1, 99, -1, 100001):
        with pytest.raises(CrtError) as e:
            r.set_option("refit_rebuild_pct", bad)
        assert e.value.code == CRT_EINVAL and "refit_rebuild_pct" in str(e.value), bad
        assert same_bits(r.accel_quality()["raw"], before), bad     # the context is usable and as it was
        assert r.refit_accel() is False                          # (the option is still 0)
        before[8] += 1
    for good in (100, 100000, 0):
        r.set_option("refit_rebuild_pct", good)
    assert same_bits(r.accel_quality()["raw"], before)


# ------------------------------------------------------------------ 5. crt_set_camera
def test_the_camera_refit_does_not_apply_the_policy(r):
    ps = soup(4099)
    far = ps.camera.copy()
    far[0:3] = ps.camera[0:3] * np.float32(6)
    try:
        options(r)
        r.upload(ps).build_accel("lbvh")
        r.transform_primitives(move_tenth(ps))
        assert r.refit_accel() is False
        q0 = r.accel_quality()
        assert q0["q_now"] > 1.05 * q0["q_built"] and q0["refits"] == 1
        r.set_option("refit_rebuild_pct", 100)                   # would fire at the next crt_refit_accel
        pad = r.debug_hit_pad
        r.set_camera(far)                                        # a larger pad: the boxes are refitted inside the call
        assert r.debug_hit_pad > pad
        A = r.debug_read_accel()
        assert A["tree_pad"] == A["hit_pad"] and A["stale"] == 0
        q1 = r.accel_quality()
        assert q1["refits"] == 2 and q1["rebuilds"] == q0["rebuilds"], (q0, q1)
        assert same_bits(q1["raw"][4:8], q0["raw"][4:8])
        assert r.refit_accel() is True                           # the same P does fire here
        q2 = r.accel_quality()
        assert q2["refits"] == 0 and q2["rebuilds"] == q0["rebuilds"] + 1
    finally:
        options(r)


# ------------------------------------------------------------------ 6. Node and the command line
SCRIPT = r"""
const { Main } = require(process.argv[1] + '/host/main.js');
const r = Main({ width: 64, height: 64, accel: 'lbvh' });
const built = r.accelQuality();
r.transformPrimitives([{ first: 16, count: 2, m: [1, 0, 0, 300, 0, 1, 0, 200, 0, 0, 1, 0] }]);
const rebuilt0 = r.refitAccel();
const refitted = r.accelQuality();
r.setOption('refit_rebuild_pct', 100);
const rebuilt1 = r.refitAccel();
const after = r.accelQuality();
let refused = false;
try { r.setOption('refit_rebuild_pct', 99); } catch (e) { refused = /refit_rebuild_pct/.test(String(e)); }
console.log(JSON.stringify({ built, refitted, after, rebuilt0, rebuilt1, refused }));
r.destroy();
"""


def test_node_accel_quality_equals_the_python_path(r):
    """The addon's accelQuality is the same twelve numbers (JSON keeps a double's bits), through the same policy."""
    import json
    import shutil
    import subprocess
    from conftest import ROOT
    node = shutil.which("node")
    if node is None:
        pytest.skip("node not installed")
    out = subprocess.run([node, "-e", SCRIPT, ROOT], capture_output=True, text=True, check=True, cwd=ROOT)
    js = json.loads(out.stdout.strip().splitlines()[-1])
    try:
        options(r)
        r.upload(cornell64()).build_accel("lbvh")
        built = r.accel_quality()["raw"]
        r.transform_primitives([(16, 2, np.float64([[1, 0, 0, 300], [0, 1, 0, 200], [0, 0, 1, 0]]))])
        assert r.refit_accel() is False and js["rebuilt0"] is False
        refitted = r.accel_quality()["raw"]
        assert refitted[2] + refitted[3] > built[2] + built[3]
        r.set_option("refit_rebuild_pct", 100)
        assert r.refit_accel() is True and js["rebuilt1"] is True
        after = r.accel_quality()["raw"]
        assert after[8] == 0 and after[9] == built[9] + 1
        for name, want in (("built", built), ("refitted", refitted), ("after", after)):
            got = np.float64(js[name])
            got[9] += built[9]                                   # (this context has a history of its own)
            assert same_bits(got, want), (name, got, want)
        assert js["refused"] is True
    finally:
        options(r)


def test_cli_rebuild_pct(tmp_path):
    """--animate-device --rebuild-pct P: the option is set, the refits and the policy's rebuilds are printed, and the frames
    are the same bytes whatever P is (a rebuilt tree is another tree over the same primitives)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT

    def run(tag, *extra):
        out = subprocess.run([sys.executable, "-m", "computeraytracer_amd", "--width", "48", "--height", "32", "--spp", "2", "--orbit", "3",
                              "--denoise", "2", "--temporal", "--animate-device", *extra, "--out", str(tmp_path / f"{tag}.png")],
                             cwd=ROOT, check=True, capture_output=True, text=True)
        info = json.loads(out.stdout.strip().splitlines()[-1])
        return info, [open(f, "rb").read() for f in info["out"]]

    plain, frames = run("a")
    assert "refits" not in plain and "rebuilds" not in plain and len(frames) == 3
    never, f_never = run("b", "--rebuild-pct", "100000")
    assert (never["rebuild_pct"], never["refits"], never["rebuilds"]) == (100000, 2, 0) and f_never == frames
    eager, f_eager = run("c", "--rebuild-pct", "100")
    assert (eager["rebuild_pct"], eager["refits"]) == (100, 2) and f_eager == frames     # (how many of them fire is the scene's matter)
    bad = subprocess.run([sys.executable, "-m", "computeraytracer_amd", "--width", "48", "--height", "32", "--spp", "2", "--orbit", "2",
                          "--denoise", "2", "--temporal", "--animate-device", "--rebuild-pct", "99", "--out", str(tmp_path / "d.png")],
                         cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode != 0 and "refit_rebuild_pct" in bad.stderr
