"""Bit pins of the three preview filters (run with -m gpu on an MI355X): SHA-256 of the raw bytes of every output of
crt_denoise, crt_denoise_adaptive and crt_denoise_temporal on the renders of tests/golden/make_denoise_pins.py equal
tests/golden/denoise_pins.json, which that script wrote.  The renders are the oracle's bit for bit, and the library is
compiled without contraction or fast-math, so there is no tolerance: the other tests hold the adaptive and temporal
filters to 1e-4 of their float64 restatements, this one shows that a change which rearranges them moves no bit."""
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
    assert len(want) == 56                                     # 2 x 3 x 2 temporal, 2 x 3 adaptive (3 planes each), 1 plain (2)
