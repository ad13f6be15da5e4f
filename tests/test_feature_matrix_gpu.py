"""GPU tests of the pipeline's features in pairs (run with -m gpu on an MI355X): one test per row of the covering matrix
of tests/feature_matrix.py -- every pair of levels of scene, builder, tree form, rectangle, sample offset, sampling,
wf_defer_nee, gen culling, driver, frame ring, counters and scene state that the library accepts occurs in some row --
rendered at 100 x 76 and held to the oracle bit for bit: the f32 accumulator and every rgba8 byte (per tile count in the
adaptive rows, with the counts and errors of tests/adaptive_ref.py), the frames of the ring, the counters, and the
first-hit G-buffer.  Each row asserts the tree and the kernel it ran on (accel_stats, crt_debug_trace_rays' report), the
records after its edit against tests/scene_transform_ref.py and tests/scene_topology_ref.py, and what crt_refit_accel
returns.  A refusal met here is a failure: the rules of feature_matrix.py say what the library accepts.
tests/test_feature_matrix_cpu.py asserts that the rows cover what they claim and that the oracle alone leaves different
counts in every adaptive row.

Measured on one MI355X: see DESIGN.md 3 (test list) for this file's time."""
from types import SimpleNamespace

import numpy as np
import pytest

import adaptive_ref
import denoise_ref
import feature_matrix as FM
import traversal_cases as TC
from conftest import bits
from test_adaptive_gpu import Truth, run_rounds
from test_adaptive_temporal_gpu import assert_pixels_are_the_oracles
from test_denoise_gpu import assert_gbuffer
from test_material_matrix_gpu import BUILDER
from test_traversal_rays_gpu import FORMS as TREE_FORMS, expected_tree

pytestmark = pytest.mark.gpu
F = np.float32
ROWS = FM.rows()
ROUNDS = 4                                        # 2 samples each up to max_samples 6, and the call that finds no tile

_SCENE, _ORACLE, _GBUFFER, _TRUTH = {}, {}, {}, {}


# ------------------------------------------------------------------ the oracle's side, each piece computed once
def oracle_scene(orc, name, state):
    """The oracle's scene of the EXPECTED records of a scene state (never of a read-back)."""
    if (name, state) not in _SCENE:
        _SCENE[name, state] = orc.Scene.from_packed(FM.edit(name, state)["ps"])
    return _SCENE[name, state]


def tone_mapped(sc, acc, n):
    """The oracle's rgba8 of an accumulator of n samples (its filter with no pass: the guides are not read)."""
    return sc.denoise(acc, int(n), np.zeros(acc.shape[:2] + (8,), F), iterations=0)[1]


def oracle_frame(orc, name, state, first, count, rect):
    """(accumulator, rgba8, counters) of samples first .. first + count - 1 in rect, full-size arrays; left unchanged.
    Under an offset the rgba8 is the tone map with `count`, not the oracle's own with first + count - 1: crt.h "Sample
    offset", "everything that COUNTS samples keeps counting from the reset: crt_sample_count, the tone map's divisor,
    the indices of the frame ring" (tests/test_sample_offset_gpu.py takes its rgba8 the same way)."""
    key = (name, state, first, count, rect)
    if key not in _ORACLE:
        sc = oracle_scene(orc, name, state)
        out = sc.render(count, first_sample=first, rect=rect)
        if first != 1:
            out = (out[0], tone_mapped(sc, out[0], count), out[2])
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def oracle_gbuffer(orc, name, state):
    if (name, state) not in _GBUFFER:
        _GBUFFER[name, state] = denoise_ref.oracle_gbuffer(orc, FM.edit(name, state)["ps"], (0, 0, FM.W, FM.H))
    return _GBUFFER[name, state]


class OffsetTruth(Truth):
    """test_adaptive_gpu.Truth under a sample offset B: a tile holding n samples holds the oracle's samples B+1 .. B+n,
    while the counts, the tone map's divisor and E keep counting from the reset (crt.h "Sample offset")."""

    def __init__(self, orc, ps, rows, cols, offset):
        super().__init__(orc, ps, rows, cols)
        self.offset = int(offset)

    def frame(self, n):
        if n not in self._frames:
            acc, rgba, _ = self.sc.render(n, first_sample=self.offset + 1, rect=self.rect)
            if self.offset:
                rgba = tone_mapped(self.sc, acc, n)
            self._frames[n] = (self._cut(acc), self._cut(rgba))
        return self._frames[n]

    def sums(self, counts):
        npx = adaptive_ref.pixel_counts(counts, *self.S[0].shape)
        while len(self.S) <= int(npx.max()):
            acc, _, _ = self.sc.render(1, first_sample=self.offset + len(self.S), rect=self.rect)
            s, q = adaptive_ref.accumulate(self._cut(acc)[None, ..., 1], self.S[-1], self.Q[-1])
            self.S.append(s)
            self.Q.append(q)
        S, Q = np.stack(self.S), np.stack(self.Q)
        ii, jj = np.indices(npx.shape)
        return S[npx, ii, jj], Q[npx, ii, jj]


def truth_of(orc, row):
    key = (row["scene"], row["state"], row["offset"], row["rect"])
    if key not in _TRUTH:
        rows_, cols, _ = FM.rectangle(row)
        _TRUTH[key] = OffsetTruth(orc, FM.edit(row["scene"], row["state"])["ps"], rows_, cols, row["offset"])
    return _TRUTH[key]


def oracle_rounds(truth):
    """run_rounds on the oracle alone: the counts the rule of tests/adaptive_ref.py leaves with FM.ADAPTIVE and the median
    of the finite errors after the first round as the threshold."""
    p = FM.ADAPTIVE
    ty, tx = (len(truth.rows) + 7) // 8, (len(truth.cols) + 7) // 8
    counts = np.full((ty, tx), p["samples"], np.uint32)
    thr = None
    for _ in range(1, ROUNDS):
        errors = truth.errors(counts)
        if thr is None:
            thr = F(np.median(errors[np.isfinite(errors)]))
        grow = adaptive_ref.active(counts, errors, p["min_samples"], p["max_samples"], thr)
        if not grow.any():
            break
        counts = counts + p["samples"] * grow.astype(np.uint32)
    return counts


# ------------------------------------------------------------------ the checks
def assert_image(acc, rgba, acc_o, rgba_o, what):
    """test_gpu_parity.assert_same_image; should the oracle hold NaN, the rule of test_material_matrix_gpu.assert_frame:
    the same NaN mask, bit-identical elsewhere (NaN payloads are not part of the contract), rgba8 equal everywhere."""
    assert acc.shape == acc_o.shape and rgba.shape == rgba_o.shape, (what, acc.shape, acc_o.shape)
    nan_o = np.isnan(acc_o[..., :3]).any(-1)
    assert np.array_equal(np.isnan(acc[..., :3]), np.isnan(acc_o[..., :3])), f"{what}: the NaN pixels differ"
    bad = (bits(acc)[..., :3] != bits(acc_o)[..., :3]).any(-1) & ~nan_o
    assert not bad.any(), f"{what}: {int(bad.sum())} accumulator pixels differ, first at {np.argwhere(bad)[0][::-1]}"
    assert np.array_equal(rgba, rgba_o), f"{what}: {int((rgba != rgba_o).sum())} rgba8 bytes differ"


def assert_tree(r, row, prims, camera, what):
    """accel_stats shows the builder and the width the row asks for, and an empty crt_debug_trace_rays names the kernel
    test_traversal_rays_gpu.expected_tree predicts: no silent fallback passes for coverage."""
    if row["builder"] == "none":
        return
    st = r.accel_stats()
    form = row["form"] if row["form"] in TREE_FORMS else "defaults"          # ("pipeline=0" is no tree form)
    case = SimpleNamespace(name=row["id"], eye=np.asarray(camera[0:3], np.float32))
    kernel, width, bpb, _, _ = expected_tree(case, prims, row["builder"], form, st["nodes"] == 0)
    if not FM.wavefront(row):
        width, bpb = 2, 32                                                    # the single kernel walks the BVH2
    assert st["builder"] == BUILDER[row["builder"]], (what, st)
    assert (st["width"], st["bytes_per_box"]) == (width, bpb), (what, st)
    if FM.wavefront(row):
        rep = r.debug_trace_rays(np.zeros((0, 3), F), np.zeros((0, 3), F))[3]
        assert rep["kernel"] == kernel and rep["width"] == (8 if width == 8 else 4), (what, rep)
        assert rep["counting"] == bool(row["counters"]), (what, rep)


def edit_scene(r, row, ps):
    """The row's scene state: the edit, crt_refit_accel's answer, the records on the device.  Returns the records."""
    plan = FM.edit(row["scene"], row["state"])
    tree = row["builder"] != "none"
    if row["state"] == "transformed":
        eye = ps.camera[0:3]
        assert TC.quantisable(ps.primitives, eye) and TC.quantisable(plan["prims"], eye)
        r.transform_primitives(plan["ops"])
        # crt.h: rebuilt "for an 8-wide tree (option "wf_width" = 8) or when the refitted boxes cannot be quantised"
        assert r.refit_accel() is (tree and row["form"] == "wf_width=8"), "crt_refit_accel's *rebuilt after the transform"
    elif row["state"] == "removed_appended":
        r.remove_primitives(plan["ranges"])                      # lights = NULL: the light list follows
        r.append_primitives(plan["records"])
        assert r.refit_accel() is tree, "crt_refit_accel's *rebuilt after the removal and the append"
        assert r.scene.lights.tobytes() == plan["lights"].tobytes(), "the binding's light list"
    if row["state"] != "fresh":
        got = r.read_primitives(0, len(plan["prims"]))
        bad = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, plan["prims"])])
        assert len(bad) == 0, f"records {bad[:8]} differ from the restatement"
        assert_tree(r, row, plan["prims"], ps.camera, "after the refit")
    return plan["prims"]


def render_uniform(r, orc, row):
    name, state, B = row["scene"], row["state"], row["offset"]
    rows_, cols, rect = FM.rectangle(row)

    def cut(a):
        return a[rows_][:, cols]
    r.reset_counters()
    for n in ((FM.SPP,) if row["sampling"] == "fused" else FM.CALLS):
        r.frame(n)                                               # (no sync between the calls)
    early, late = FM.RING_READS
    if row["frame_ring"]:                                        # a frame of the ring while the run may still be in flight
        early_frame = r.read_sample_rgba8(early)
    r.sync()
    assert r.sample == FM.SPP
    acc_o, rgba_o, cnt = oracle_frame(orc, name, state, B + 1, FM.SPP, rect)
    assert_image(r.read_accum(), r.read_rgba8(), cut(acc_o), cut(rgba_o), f"{FM.SPP} samples from index {B + 1}")
    if row["frame_ring"]:
        assert r.latest_sample == FM.SPP
        assert np.array_equal(early_frame, cut(oracle_frame(orc, name, state, B + 1, early, rect)[1])), f"frame {early} of the ring"
        assert np.array_equal(r.read_sample_rgba8(late), cut(rgba_o)), f"frame {late} of the ring"
    if row["counters"] and row["rect"] != "bands":
        c = r.counters()
        assert (c["rays"], c["paths"], c["bounces"], c["shadow"]) == (int(cnt[0]), int(cnt[2]), int(cnt[3]), int(cnt[4])), (c, cnt)
        if FM.wavefront(row):                                    # (crt.h CRT_CNT_WALKED: "wavefront pipeline only")
            assert 0 < c["walked"] <= c["rays"], c


def render_adaptive(r, orc, row):
    truth = truth_of(orc, row)
    p = FM.ADAPTIVE
    r.reset_counters()
    counts, _ = run_rounds(r, truth, p["samples"], p["min_samples"], p["max_samples"], ROUNDS)
    assert np.array_equal(counts, oracle_rounds(truth))
    assert len(np.unique(counts)) >= 2, "tiles should retire at different counts"
    if row["offset"] and row["rect"] == "whole":
        assert_pixels_are_the_oracles(r, truth.sc, lambda n: truth.frame(n)[0], counts)
    if row["rect"] != "bands":
        r.reset().frame(1).sync()                                # (crt_read_gbuffer wants a uniform sample)


def run(r, orc, row):
    ps = FM.scene(row["scene"])
    # 1. configure and upload
    for k, v in FM.options(row).items():
        r.set_option(k, v)
    r.enable_counters(bool(row["counters"]))
    r.upload(ps)
    if row["rect"] == "tile":
        r.set_tile(*FM.TILE)
    elif row["rect"] == "bands":
        r.set_row_bands(*FM.BANDS)
    r.build_accel(row["builder"])
    rows_, cols, _ = FM.rectangle(row)
    assert r.tile[2:] == (len(cols), len(rows_))
    assert_tree(r, row, ps.primitives, ps.camera, "after the build")
    # 2. scene state
    edit_scene(r, row, ps)
    # 3. offset: after the edit, at sample 0
    if row["offset"]:
        r.set_sample_offset(row["offset"])
    # 4 - 6. render, the ring, the counters
    if row["sampling"] == "adaptive":
        render_adaptive(r, orc, row)
    else:
        render_uniform(r, orc, row)
    # 7. the G-buffer kernel's walk of this tree (a sync point that only reads; row bands have no G-buffer)
    if row["rect"] != "bands":
        want, hit = oracle_gbuffer(orc, row["scene"], row["state"])
        assert_gbuffer(r.read_gbuffer(), want[rows_][:, cols], hit[rows_][:, cols])


def restore(r):
    for k, v in FM.OPTION_DEFAULTS.items():
        r.set_option(k, v)
    r.enable_counters(False)
    if r.scene is not None:
        r.set_tile(0, 0, *r.image_size)
        r.reset().set_sample_offset(0)


@pytest.mark.parametrize("row", ROWS, ids=[row["id"] for row in ROWS])
def test_row_matches_the_oracle(renderer, orc, row):
    try:
        run(renderer, orc, row)
    except Exception as e:
        raise AssertionError(f"{row['id']}: {type(e).__name__}: {e}\n    row: {row}") from e
    finally:
        restore(renderer)
