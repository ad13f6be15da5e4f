"""The oracle's loop over every primitive against float64 geometry (CPU only).

Every other test holds the kernels to the oracle bit for bit; this one holds the oracle (orc.Scene.intersect) to
geometry_truth.py: on six scenes x 13-15 seeded ray classes of 2000 rays, every ray the reference calls CLEAR must come
back with the expected primitive (or as a miss), t within mu_t of the true distance.  No tolerance on the decision.
An edit of the oracle's intersection tests that keeps the kernels in lockstep passes every parity suite; it does not
pass here.

What keeps the test from hiding a failure: the share of clear rays per (scene, class) is a property of the rays and
the reference alone; it is pinned below as a floor 0.02 under the measured value and asserted before anything is
compared.  The classes aimed at exact edges and vertices are unclear by construction: they are counted, not compared.

Classes that cannot keep half of their rays clear under K = 16 (beside sigma = 0, sigma = 1e-6 r and the vertices),
measured, all for the same reason -- the margin's T holds the largest coordinate, 300 here, against a feature of size
r = 1, a t of 0.001 or a cosine below 1e-3:
  near_tmin            every scene (M1-M3 0.08-0.09, M4 0.07, P1 0.11, S1 0.47): mu_t is about 1e-6 x the coordinates, 1e-3
                       for the meshes, so only the factors 0.5 and 2 can be clear; M4's two plain triangles at the origin
                       are where t_min x {0.999, 1.001, 1.005} is clear
  edge_0.0001          M2 (0.00 / 0.03): sigma = 1e-4 of r = 1 is 1e-4 units, mu_u is 8e-4 units there
  grazing              M2 (0.00) and M4 (0.17: needles and slivers)

The leak zone (rays from inside a closed mesh that come back as a miss) is counted per sigma for M1-M3 and every leak
must be UNCLEAR by the reference; DESIGN.md 2 ("Accuracy against geometry") holds the table."""
import numpy as np
import pytest

import geometry_truth as G
import traversal_cases as TC

SCENES = {s.name: s for s in G.scenes()}

# share of clear rays per (scene, class), measured with SEED = 20261 and K = 16, minus 0.02 (0: nothing to assert)
FLOORS = {
    "M1": {"random_in": 0.980, "random_out": 0.979, "edge_0_in": 0.000, "edge_0_out": 0.014, "edge_1e-06_in": 0.000,
           "edge_1e-06_out": 0.027, "edge_0.0001_in": 0.861, "edge_0.0001_out": 0.821, "edge_0.01_in": 0.979,
           "edge_0.01_out": 0.977, "vertex_in": 0.000, "vertex_out": 0.002, "grazing": 0.706, "near_tmin": 0.061,
           "random_in_excl": 0.980},
    "M2": {"random_in": 0.939, "random_out": 0.927, "edge_0_in": 0.000, "edge_0_out": 0.008, "edge_1e-06_in": 0.000,
           "edge_1e-06_out": 0.019, "edge_0.0001_in": 0.000, "edge_0.0001_out": 0.009, "edge_0.01_in": 0.855,
           "edge_0.01_out": 0.833, "vertex_in": 0.000, "vertex_out": 0.000, "grazing": 0.000, "near_tmin": 0.072,
           "random_in_excl": 0.948},
    "M3": {"random_in": 0.980, "random_out": 0.979, "edge_0_in": 0.000, "edge_0_out": 0.014, "edge_1e-06_in": 0.000,
           "edge_1e-06_out": 0.027, "edge_0.0001_in": 0.861, "edge_0.0001_out": 0.821, "edge_0.01_in": 0.979,
           "edge_0.01_out": 0.977, "vertex_in": 0.000, "vertex_out": 0.002, "grazing": 0.706, "near_tmin": 0.061,
           "random_in_excl": 0.980},
    "M4": {"random_in": 0.928, "random_out": 0.972, "edge_0_in": 0.000, "edge_0_out": 0.025, "edge_1e-06_in": 0.007,
           "edge_1e-06_out": 0.029, "edge_0.0001_in": 0.797, "edge_0.0001_out": 0.846, "edge_0.01_in": 0.927,
           "edge_0.01_out": 0.976, "vertex_in": 0.000, "vertex_out": 0.040, "grazing": 0.148, "near_tmin": 0.050,
           "random_in_excl": 0.934},
    "P1": {"random_in": 0.923, "random_out": 0.935, "edge_0_in": 0.418, "edge_0_out": 0.530, "edge_1e-06_in": 0.429,
           "edge_1e-06_out": 0.547, "edge_0.0001_in": 0.906, "edge_0.0001_out": 0.887, "edge_0.01_in": 0.951,
           "edge_0.01_out": 0.954, "vertex_in": 0.334, "vertex_out": 0.440, "grazing": 0.895, "near_tmin": 0.086,
           "random_in_excl": 0.927},
    "S1": {"random_in": 0.980, "random_out": 0.894, "edge_0_in": 0.980, "edge_0_out": 0.021, "edge_1e-06_in": 0.980,
           "edge_1e-06_out": 0.014, "edge_0.0001_in": 0.980, "edge_0.0001_out": 0.594, "edge_0.01_in": 0.980,
           "edge_0.01_out": 0.636, "grazing": 0.829, "near_tmin": 0.454, "random_in_excl": 0.980},
}
HALF_EXEMPT = {("M2", "edge_0.0001_in"), ("M2", "edge_0.0001_out"), ("M2", "grazing"), ("M4", "grazing")} | {(s, "near_tmin") for s in SCENES}
LOW_BY_DESIGN = ("edge_0_", "edge_1e-06_", "vertex_")


_ANSWER = {}


def oracle_answer(orc, b):
    if b.sc.name not in _ANSWER:
        _ANSWER[b.sc.name] = TC.oracle_reference(orc, b.sc.packed())(b.o, b.d, b.ex)
    return _ANSWER[b.sc.name]


def assert_floors(b):
    sh = b.shares()
    assert set(sh) == set(FLOORS[b.sc.name]), (b.sc.name, sorted(sh))
    for c, v in sh.items():
        assert v >= FLOORS[b.sc.name][c], f"{b.sc.name} / {c}: {v:.3f} of the rays are clear, the floor is {FLOORS[b.sc.name][c]:.3f}"
        if not c.startswith(LOW_BY_DESIGN) and (b.sc.name, c) not in HALF_EXEMPT:
            assert v >= 0.5, f"{b.sc.name} / {c}: only {v:.3f} of the rays are clear"
    return sh


def fmt_leaks(leaks):
    return ", ".join(f"{c} {n} / {of}" for c, (n, _, of) in leaks.items())


@pytest.mark.parametrize("name", list(SCENES))
def test_the_reference_agrees_with_exact_arithmetic(name):
    """200 seeded rays of the scene, each with the nearest primitive it does not clearly miss and a random one: wherever
    the float64 classification says clear hit (and which root of a sphere) or clear miss, exact Fraction arithmetic on the
    same float32 inputs decides the same."""
    b = G.batch(SCENES[name])
    rng = np.random.default_rng(G.SEED + 1)
    rays = rng.choice(len(b.o), 200, replace=False)
    o, d = b.o[rays], b.d[rays]
    state, ts, _, _ = G.classify(b.sc.prims, o, d)
    near = np.where(state != G.MISS, np.where(np.isnan(ts), np.inf, np.abs(ts)), np.inf).argmin(1)
    pairs = [(i, int(near[i])) for i in range(200)] + [(i, int(j)) for i, j in enumerate(rng.integers(0, len(b.sc.prims), 200))]
    bad, nh, nm = G.self_check(b.sc.prims, o, d, pairs)
    print(f"self-check {name}: {nh} clear hits and {nm} clear misses of {len(pairs)} pairs decided exactly")
    assert not bad, f"{name}: {len(bad)} pairs the reference calls clear are decided otherwise exactly; first (ray, primitive, state, root, exact): {bad[0]}"
    assert nh >= 20 and nm >= 100, (name, nh, nm)                  # (not vacuous: both kinds of clear pair were checked)


@pytest.mark.parametrize("name", list(SCENES))
def test_the_oracles_loop_decides_every_clear_ray_as_geometry_does(orc, name):
    b = G.batch(SCENES[name])
    sh = assert_floors(b)                                       # before anything is compared
    t, i = oracle_answer(orc, b)
    msg, rel, leaks = G.report(b, t, i, f"{name} / oracle")
    print(f"clear shares {name}: " + ", ".join(f"{c} {v:.3f}" for c, v in sh.items()))
    print(f"largest |t - t*| / (2^-24 s_t) {name}: {rel:.3f}" + (f"; leaks from inside: {fmt_leaks(leaks)}" if leaks else ""))
    assert msg is None, msg
    assert rel <= G.K


@pytest.mark.parametrize("name", ["M1", "M2", "M3"])
def test_every_leak_of_a_closed_mesh_is_an_unclear_ray(orc, name):
    """The leak zone of the binary32 edge test, written down: rays from inside the closed mesh that miss it, per class.
    Geometry gives one thing for free: no clear ray leaks."""
    b = G.batch(SCENES[name])
    assert_floors(b)
    t, i = oracle_answer(orc, b)
    _, _, leaks = G.report(b, t, i, name)
    assert set(leaks) == {"random_in", "vertex_in"} | {f"edge_{s:g}_in" for s in G.SIGMAS}
    print(f"leaks {name}: {fmt_leaks(leaks)}")
    for c, (n, unclear, of) in leaks.items():
        assert of == G.N
        assert n == unclear, f"{name} / {c}: {n} of {of} rays from inside leak, {n - unclear} of them CLEAR by the reference"
