"""The covering matrix of tests/feature_matrix.py is what it claims (no GPU): every row is legal, every pair of levels
that some legal configuration holds occurs in a row -- the required set recomputed here by plain enumeration of all
233 280 configurations under a second statement of the rules --, the rows are few and deterministic, the scene states
are the restatements' and stay quantisable, and the oracle alone leaves different counts in every adaptive row."""
import itertools

import numpy as np

import feature_matrix as FM

REQUIRED_PAIRS = 539                              # a rule that removes pairs shows here
EXCLUDED_PAIRS = 18                               # ... of the 557 there are: DESIGN.md 3 lists them by rule
MAX_ROWS = 32
ROWS = FM.rows()


def legal(row):
    """The rules once more, on a complete row, each as one sentence (include/crt.h has the contract behind them)."""
    tree = row["builder"] != "none"
    wavefront = tree and row["form"] != "pipeline=0"
    if not tree and row["form"] in ("wf_trace_form=1", "quantize=0", "wf_width=8"):
        return False                              # no tree, no tree form
    if not wavefront and (row["offset"], row["wf_defer_nee"], row["cull"], row["driver"], row["frame_ring"]) != (0, 1, "both", "defaults", 0):
        return False                              # the wavefront pipeline's alone
    if row["sampling"] == "adaptive" and row["frame_ring"]:
        return False                              # crt_read_sample_rgba8 refuses in the adaptive state
    return True


def enumerate_required():
    names = list(FM.FACTORS)
    duos = list(itertools.combinations(range(len(names)), 2))
    out = set()
    for levels in itertools.product(*(FM.FACTORS[f] for f in names)):
        if legal(dict(zip(names, levels))):
            out.update(((names[a], levels[a]), (names[b], levels[b])) for a, b in duos)
    return out


def test_every_row_satisfies_every_rule():
    rows = ROWS
    assert len({r["id"] for r in rows}) == len(rows)
    for k, r in enumerate(rows):
        assert set(r) == set(FM.FACTORS) | {"id"} and r["id"].startswith(f"r{k:02d}-") and r["id"].isprintable() and " " not in r["id"]
        assert all(r[f] in FM.FACTORS[f] for f in FM.FACTORS), r
        assert legal(r) and FM.broken(r) == [], r
        if not FM.wavefront(r):                   # else a pair would count as covered while the option is ignored
            assert all(r[f] == FM.DEFAULT[f] for f in FM.WAVEFRONT_ONLY), r


def test_every_required_pair_is_covered_by_few_rows():
    rows = ROWS
    required = enumerate_required()
    assert required == FM.required_pairs()
    covered = set().union(*(FM.pairs_of(r) for r in rows))
    missing = sorted(required - covered, key=str)
    print(f"{len(required)} required pairs, {len(rows)} rows; uncovered: {missing}")
    assert not missing
    assert covered <= required
    assert len(rows) <= MAX_ROWS
    assert len(required) == REQUIRED_PAIRS
    every = sum(len(FM.FACTORS[a]) * len(FM.FACTORS[b]) for a, b in itertools.combinations(FM.FACTORS, 2))
    assert every - len(required) == EXCLUDED_PAIRS


def test_the_generator_is_deterministic():
    assert FM.rows() == ROWS
    assert FM.rows(seed=1, candidates=20) != FM.rows(candidates=20)      # (the seed is used)


def test_options_and_rectangles():
    for r in ROWS:
        o = FM.options(r)
        assert set(o) == set(FM.OPTION_DEFAULTS)
        if not FM.wavefront(r):
            off = {k for k in o if o[k] != FM.OPTION_DEFAULTS[k]} - {"pipeline", "wf_cohort"}
            assert not off, (r, off)
        assert o["adaptive_temporal"] == int(r["sampling"] == "adaptive" and r["offset"] != 0)
        rows_, cols, rect = FM.rectangle(r)
        assert rect[0] == cols[0] and rect[2] == cols[-1] + 1 and rect[1] == rows_.min() and rect[3] == rows_.max() + 1
    assert FM.options(FM.DEFAULT) == FM.OPTION_DEFAULTS
    x0, y0, x1, y1 = FM.TILE
    assert all(v % 8 for v in FM.TILE) and x1 <= FM.W and y1 <= FM.H and FM.W % 8 and FM.H % 8 and FM.W % 16 and FM.H % 16
    rows_, _, _ = FM.rectangle(dict(FM.DEFAULT, rect="bands"))
    assert FM.BANDS[0] == 8 and rows_.tolist() == [y for y in range(FM.H) if (y // 8) % 3 == 1]   # what adaptive sampling accepts


def test_scene_states_are_the_restatements_and_stay_quantisable():
    import scene_transform_ref as xref
    import traversal_cases as TC
    for name in FM.FACTORS["scene"]:
        ps = FM.scene(name)
        n = len(ps.primitives)
        assert (ps.width, ps.height) == (FM.W, FM.H)
        assert (name == "tri_only") == (not (ps.primitives["category"] == 0).any())     # the npatch == 0 shade path
        moved = FM.edit(name, "transformed")
        assert len(moved["ops"]) == 2 and xref.valid(moved["ops"], n)
        changed = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(moved["prims"], ps.primitives)])
        assert len(changed) == sum(op[1] for op in moved["ops"])
        assert any(len(op) > 3 for op in moved["ops"]) == bool((ps.primitives["category"] == 1).any())
        regrown = FM.edit(name, "removed_appended")
        assert len(regrown["prims"]) == n and len(regrown["ranges"]) == 2 and len(regrown["records"]) == 2
        assert regrown["prims"]["data4"][:, 3].tolist() == list(range(n))
        gone = sorted(first for first, _ in regrown["ranges"])
        before = (ps.lights["data4"][:, 3].astype(np.int64))
        want = before - (before > gone[0]) - (before > gone[1])                       # the documented renumbering
        assert regrown["lights"]["data4"][:, 3].tolist() == want.tolist()
        for plan in (moved, regrown):
            assert TC.quantisable(plan["prims"], ps.camera[0:3]) and TC.quantisable(ps.primitives, ps.camera[0:3])
            emit = plan["prims"][plan["lights"]["data4"][:, 3]]
            assert (emit["data4"][:, 2] == 1).all()
            for f in ("data1", "data2", "data3"):                                     # the emitters lie where their light records say
                assert np.array_equal(emit[f][:, :3], plan["lights"][f][:, :3])


def test_the_oracle_alone_leaves_different_counts_in_every_adaptive_row(orc):
    from test_feature_matrix_gpu import oracle_rounds, truth_of
    seen = set()
    for r in ROWS:
        if r["sampling"] != "adaptive":
            continue
        counts = oracle_rounds(truth_of(orc, r))
        print(r["id"], dict(zip(*np.unique(counts, return_counts=True))))
        assert len(np.unique(counts)) >= 2, r
        assert counts.min() == FM.ADAPTIVE["min_samples"] and counts.max() <= FM.ADAPTIVE["max_samples"]
        seen.add(r["scene"])
    assert seen == set(FM.FACTORS["scene"])       # an adaptive row per scene
