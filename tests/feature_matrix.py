"""The pairwise covering matrix of the render pipeline's features (a helper module, not collected by pytest; no GPU).

Every feature of the pipeline came with tests that cross it with some of the older ones and leave the rest at their
defaults.  Here every feature is a FACTOR with its levels (default first), RULES say which combinations the library
accepts (each with the sentence of include/crt.h or the refusal of csrc/crt_api.cpp behind it), and rows() is a small
seeded set of legal configurations in which every pair of levels that some legal configuration holds occurs at least
once.  tests/test_feature_matrix_cpu.py checks that claim by an enumeration of its own; tests/test_feature_matrix_gpu.py
renders every row and holds it to the oracle.  scene(), options(), rectangle() and edit() say what a level means, for
both files.  Standard library only, but for the numpy records of scene() and edit()."""
import itertools
import random

W, H = 100, 76                                   # ragged against 8 x 8 tiles and 16 x 16 blocks on both edges
SPP = 5
OFFSET = 1000
TILE = (5, 3, 77, 61)                            # no edge on a multiple of 8
BANDS = (8, 3, 1)                                # crt_set_row_bands(band_rows, parts, part)
CALLS = (1, 2, 1, 1)
ADAPTIVE = dict(samples=2, min_samples=2, max_samples=6)
RING = 8
RING_READS = (3, 5)

# factor -> levels, the default first; SHORT: what a level that is off its default adds to the row's id
FACTORS = {
    "scene": ("cornell", "tri", "tri_only"),
    "builder": ("bvh2", "lbvh", "ploc", "none"),
    "form": ("defaults", "wf_trace_form=1", "quantize=0", "wf_width=8", "pipeline=0"),
    "rect": ("whole", "tile", "bands"),
    "offset": (0, OFFSET),
    "sampling": ("fused", "calls", "adaptive"),
    "wf_defer_nee": (1, 0),
    "cull": ("both", "classes0", "off"),
    "driver": ("defaults", "pipes1", "pipes4"),
    "frame_ring": (0, RING),
    "counters": (0, 1),
    "state": ("fresh", "transformed", "removed_appended"),
}
NAMES = tuple(FACTORS)
DEFAULT = {f: levels[0] for f, levels in FACTORS.items()}
SHORT = {"form": {"wf_trace_form=1": "form1", "quantize=0": "quantize0", "wf_width=8": "width8", "pipeline=0": "pipeline0"},
         "offset": {OFFSET: "offset"}, "wf_defer_nee": {0: "nee0"}, "cull": {"classes0": "classes0", "off": "cull0"},
         "frame_ring": {RING: "ring"}, "counters": {1: "counting"}, "state": {"transformed": "moved", "removed_appended": "regrown"}}
# what belongs to the wavefront pipeline alone (crt.h "Sample offset": "Wavefront pipeline only: with a non-zero offset
# crt_trace under "pipeline" = 0 or CRT_ACCEL_NONE, and crt_trace_adaptive, return CRT_ESTATE"; crt_read_sample_rgba8:
# "frames are kept by the wavefront pipeline only"; the wf_ options are read by the wavefront driver and kernels only)
WAVEFRONT_ONLY = ("offset", "wf_defer_nee", "cull", "driver", "frame_ring")


def wavefront(row):
    """The wavefront kernels render this row: a tree and option "pipeline" = 1."""
    return row["builder"] != "none" and row["form"] != "pipeline=0"


def broken(row):
    """The names of the rules this row breaks.  `row` may be partial: a rule that needs a factor the row does not hold
    yet is not broken."""
    has = row.__contains__
    out = []
    # no-tree: quantize, wf_width and wf_trace_form shape a tree, CRT_ACCEL_NONE has none
    if has("builder") and has("form") and row["builder"] == "none" and row["form"] not in ("defaults", "pipeline=0"):
        out.append("no-tree")
    # wavefront-only: elsewhere the option would be ignored (or, for the offset and the ring, refused: "a sample offset
    # needs the wavefront pipeline", "frames are kept by the wavefront pipeline only") and the pair would count as covered
    if (has("builder") and row["builder"] == "none") or (has("form") and row["form"] == "pipeline=0"):
        if any(has(f) and row[f] != DEFAULT[f] for f in WAVEFRONT_ONLY):
            out.append("wavefront-only")
    # adaptive and the frame ring: crt.h "In the adaptive state crt_trace, ... crt_read_sample_rgba8 ... return CRT_ESTATE"
    if has("sampling") and has("frame_ring") and row["sampling"] == "adaptive" and row["frame_ring"] != 0:
        out.append("adaptive-ring")
    # (adaptive and the offset: legal with option "adaptive_temporal" = 1, which options() sets; adaptive and row bands:
    # legal, crt_trace_adaptive refuses a crt_comm_partition of other bands, not crt_set_row_bands; BANDS holds 8 rows)
    return out


def _extendable(part):
    """Some legal row holds this partial row: as a rule the one that leaves every other factor at its default, else a
    search."""
    if broken(part):
        return False
    if not broken({**DEFAULT, **part}):
        return True
    f = next(f for f in NAMES if f not in part)
    return any(_extendable({**part, f: v}) for v in FACTORS[f])


def pairs_of(row):
    """The pairs of levels a row holds: ((factor, level), (factor, level)), factors in table order."""
    return {((a, row[a]), (b, row[b])) for a, b in itertools.combinations(NAMES, 2)}


def required_pairs():
    """Every pair of levels that some legal row holds."""
    out = set()
    for a, b in itertools.combinations(NAMES, 2):
        for va in FACTORS[a]:
            for vb in FACTORS[b]:
                if _extendable({a: va, b: vb}):
                    out.add(((a, va), (b, vb)))
    return out


def _key(pair):
    """A sort key without hash order: the positions in the table."""
    (a, va), (b, vb) = pair
    return NAMES.index(a), FACTORS[a].index(va), NAMES.index(b), FACTORS[b].index(vb)


def row_id(k, row):
    """r07-ploc-width8-tile-adaptive: the row's number and its levels that are off their defaults."""
    words = [SHORT.get(f, {}).get(row[f], str(row[f])) for f in NAMES if row[f] != DEFAULT[f]]
    return "-".join([f"r{k:02d}"] + (words or ["defaults"]))


def rows(seed=20261020, candidates=400):
    """The covering rows: greedy, seeded, deterministic.  Until every required pair is covered: build `candidates` rows,
    each from a pair that is still uncovered, completed factor by factor (in a random order) with the level that covers
    the most uncovered pairs with the factors already set, among the levels that leave the row extendable to a legal one;
    keep the candidate that covers the most.  Each row is a dict of the factors plus "id"."""
    rng = random.Random(seed)
    uncovered = required_pairs()
    out = []
    while uncovered:
        todo = sorted(uncovered, key=_key)
        best, best_gain = None, -1
        for _ in range(candidates):
            (a, va), (b, vb) = rng.choice(todo)
            row = {a: va, b: vb}
            rest = [f for f in NAMES if f not in row]
            rng.shuffle(rest)
            for f in rest:
                scored = []
                for v in FACTORS[f]:
                    if not _extendable({**row, f: v}):
                        continue
                    gain = 0
                    for g, vg in row.items():
                        p = ((f, v), (g, vg)) if NAMES.index(f) < NAMES.index(g) else ((g, vg), (f, v))
                        gain += p in uncovered
                    scored.append((gain, v))
                top = max(g for g, _ in scored)
                row[f] = rng.choice([v for g, v in scored if g == top])
            gain = len(pairs_of(row) & uncovered)
            if gain > best_gain:
                best, best_gain = row, gain
        assert best_gain > 0 and not broken(best)
        uncovered -= pairs_of(best)
        out.append(best)
    return [dict({f: r[f] for f in NAMES}, id=row_id(k, r)) for k, r in enumerate(out)]


# ------------------------------------------------------------------ what the levels mean
# every option a row touches, at its default (csrc/crt_ctx.h)
OPTION_DEFAULTS = dict(pipeline=1, quantize=1, wf_width=4, wf_trace_form=2, wf_pipes=2, spp_per_launch=0, wf_pool=0,
                       wf_finish_at=32768, wf_cohort=16, wf_defer_nee=1, wf_cull_classes=1, wf_cull_miss=1, frame_ring=0,
                       adaptive_temporal=0)
_FORM = {"defaults": {}, "wf_trace_form=1": dict(wf_trace_form=1), "quantize=0": dict(quantize=0), "wf_width=8": dict(wf_width=8),
         "pipeline=0": dict(pipeline=0)}
_CULL = {"both": {}, "classes0": dict(wf_cull_classes=0), "off": dict(wf_cull_classes=0, wf_cull_miss=0)}
_DRIVER = {"defaults": {}, "pipes1": dict(wf_pipes=1), "pipes4": dict(wf_pipes=4, wf_pool=65536, wf_finish_at=512)}


def options(row):
    """option -> value for crt_set_option: every option of OPTION_DEFAULTS, as the row wants it."""
    o = dict(OPTION_DEFAULTS)
    o.update(_FORM[row["form"]])
    o.update(_CULL[row["cull"]])
    o.update(_DRIVER[row["driver"]])
    o["wf_defer_nee"] = row["wf_defer_nee"]
    o["frame_ring"] = row["frame_ring"]
    if row["sampling"] == "calls":
        o["wf_cohort"] = 1                       # every call its own batch
    if row["sampling"] == "adaptive" and row["offset"]:
        o["adaptive_temporal"] = 1               # crt.h: "With option "adaptive_temporal" = 1 crt_trace_adaptive takes the offset too"
    return o


def rectangle(row):
    """(the global rows of the context's pixels, in local order; its columns; the rectangle (x0, y0, x1, y1) that holds
    them, which is what the oracle renders)."""
    import numpy as np
    if row["rect"] == "tile":
        x0, y0, x1, y1 = TILE
        return np.arange(y0, y1), np.arange(x0, x1), TILE
    if row["rect"] == "bands":
        from computeraytracer_amd.partition import band_rows
        band, parts, part = BANDS
        rows_ = np.asarray(band_rows(H, parts, part, band))
        return rows_, np.arange(W), (0, int(rows_.min()), W, int(rows_.max()) + 1)
    return np.arange(H), np.arange(W), (0, 0, W, H)


_SCENES = {}


def scene(name):
    """The PackedScene of a scene level, W x H, made once."""
    if name not in _SCENES:
        if name == "cornell":
            from computeraytracer_amd import cornell
            _SCENES[name] = cornell(W, H)
        else:
            import material_matrix_scenes as MM
            _SCENES[name] = MM.build(name, W, H)
    return _SCENES[name]


# scene -> (two runs that move, [first, count, is a run of spheres]; the two primitives that go and come back)
_EDITS = {"cornell": (((6, 5, False), (16, 2, True)), (7, 12)),            # a box's five patches; both spheres
          "tri": (((11, 12, False), (5, 6, False)), (8, 14)),                # the glass triangle cube; the glass patch box
          "tri_only": (((10, 6, False), (16, 6, False)), (3, 15))}           # the glass cube, in halves


def _about(R, centre, shift, scale=1.0):
    """The 12 floats of p -> R s (p - centre) + centre + shift."""
    import numpy as np
    import scene_transform_ref as xref
    R, c = np.asarray(R, np.float64), np.asarray(centre, np.float64)
    return xref.matrix(R, c + np.asarray(shift, np.float64) - scale * (R @ c), scale)


def _rotation(axis, angle):
    import numpy as np
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


_PLANS = {}


def edit(name, state):
    """What a scene-state level does to scene(name) and what must come of it, from the restatements
    tests/scene_transform_ref.py and tests/scene_topology_ref.py:
      dict(ops=...)                     transformed: one crt_transform_primitives call of two ops -- a rotation about the
                                        run's own centre plus a translation, and a similarity (scale 0.9) of the sphere
                                        run where the scene has spheres, else a second rigid move
      dict(ranges=..., records=...)     removed_appended: two primitives that are no emitters go, with lights = NULL, and
                                        come back at the end of the list, moved
    plus prims / lights, the records after the edit, and ps, the PackedScene of them (the oracle's scene)."""
    import numpy as np
    import scene_topology_ref as tref
    import scene_transform_ref as xref
    from computeraytracer_amd.scene import PackedScene
    if (name, state) in _PLANS:
        return _PLANS[name, state]
    ps = scene(name)
    prims, lights = ps.primitives, ps.lights
    n = len(prims)
    emitters = set(int(i) for i in lights["data4"][:, 3])
    plan = {}
    if state == "transformed":
        ops = []
        for k, (first, count, spheres) in enumerate(_EDITS[name][0]):
            run = prims[first:first + count]
            assert first + count <= n and not emitters & set(range(first, first + count))
            assert ((run["category"] == 1) == spheres).all()
            centre = run["data1"].astype(np.float64).mean(0)
            if spheres:
                ops.append((first, count, _about(np.eye(3), centre, (-14.0, 6.0, 9.0), 0.9), np.float32(0.9)))
            else:
                ops.append((first, count, _about(_rotation((0.3, 1.0, -0.2), 0.35 - 0.6 * k), centre, (9.0 - 20.0 * k, 4.0, -11.0))))
        assert xref.valid(ops, n)
        plan.update(ops=ops, prims=xref.apply(prims, ops), lights=lights)
    elif state == "removed_appended":
        gone = _EDITS[name][1]
        ranges = [(gone[1], 1), (gone[0], 1)]                   # (unsorted, as the call allows)
        assert not emitters & set(gone) and n // 8 <= gone[0] < gone[1] < n - 1
        assert tref.valid(ranges, n, lights["data4"][:, 3])
        kept, new_lights = tref.remove(prims, ranges, lights)
        rec = xref.apply(tref.concat(prims[gone[0]:gone[0] + 1], prims[gone[1]:gone[1] + 1]),
                         [(0, 2, xref.matrix(np.eye(3), (12.0, 7.5, -9.0)))])
        rec["data4"][:, 3] = np.arange(n - 2, n, dtype=np.uint32)
        plan.update(ranges=ranges, records=rec, prims=tref.append(kept, rec), lights=new_lights)
    else:
        assert state == "fresh"
        plan.update(prims=prims, lights=lights)
    plan["ps"] = PackedScene(plan["prims"], plan["lights"], ps.camera, ps.spectra, ps.cie)
    _PLANS[name, state] = plan
    return plan
