"""Bit pins of the preview filters (run with -m gpu on an MI355X): SHA-256 of the raw bytes of every output of crt_denoise,
crt_denoise_adaptive, crt_denoise_temporal and crt_denoise_svgf (crt_debug_read_moments included) and of crt_read_motion
on the renders and call sequences of tests/golden/make_denoise_pins.py equal tests/golden/denoise_pins.json, which that
script wrote.  The sequences are those in which the two history slots and their guides change hands: a frame filtered by
crt_denoise alone, a G-buffer rebuilt between two calls of one frame, a slot without moments between two with, two
frames that share one G-buffer, and primitive edits (two updates before one refit; an edit before a frame that
crt_denoise_temporal never sees).  The renders are the oracle's bit for bit, and the library is compiled without
contraction or fast-math, so there is no tolerance: the other tests hold the adaptive, temporal and svgf filters and the
motion map to 1e-4 of their float64 restatements, this one shows that a change which rearranges them, or the bookkeeping
around them, moves no bit."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("make_denoise_pins", os.path.join(GOLDEN, "make_denoise_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_output_of_the_three_filters_has_the_pinned_bits(renderer):
    gen = _generator()
    with open(gen.OUT) as f:
        want = json.load(f)
    got = gen.pins(renderer)
    assert sorted(got) == sorted(want), "the cases are not those of the pinned file"
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, f"{len(differ)} of {len(want)} outputs differ from the pinned bits: {differ}"
    # 100 x 76: 2 x 3 x 2 temporal, 2 x 3 adaptive (3 planes each), 1 plain (2) = 56; 64 x 48: 2 x 3 x 2 svgf (5 planes) = 60,
    # slots 4 + 7 + 3 x 5 + 3 = 29, motion 4 + 6 + 4 = 14
    assert len(want) == 56 + 60 + 29 + 14
