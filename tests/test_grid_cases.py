"""The inputs of the grid-medium function pins (tests/grid_cases.py), checked with the float64 yardstick alone: every segment
stays within the device's step bound (so the yardstick is the reference for it), every category and target kind is there and
means what its name says, and at most 1 % of the segments are ties that float32 may decide either way."""
import numpy as np
import pytest

import grid_cases


@pytest.mark.parametrize("name", sorted(grid_cases.query_grids()))
def test_segments_cover_the_cases_and_stay_under_the_tie_limit(name):
    (a, b, target), (category, kind), expected = grid_cases.query_inputs(name)
    assert a.shape == b.shape == (grid_cases.N_SEGMENTS, 3) and a.dtype == b.dtype == target.dtype == np.float32
    assert not expected["hit_bound"].any()
    assert np.isfinite(expected["transmittance"]).all() and (expected["transmittance"] <= 1.0).all()
    crossing = expected["exponent"] >= grid_cases.THIN
    for k, label in enumerate(grid_cases.CATEGORIES):
        chosen = category == k
        assert chosen.sum() >= grid_cases.N_SEGMENTS // len(grid_cases.CATEGORIES)
        assert crossing[chosen].mean() > 0.3, label   # a good part of them meets the grid
    names = grid_cases.TARGET_KINDS
    for k, label in enumerate(names):
        chosen = kind == k
        assert (chosen & crossing).sum() > 300, label
        assert expected["valid"][chosen].all() == (label in ("met", "just-met")) and expected["valid"][chosen].any() == (label in ("met", "just-met")), label
    assert (expected["distance"][~expected["valid"]] == -1.0).all() and (expected["distance"][expected["valid"]] >= 0.0).all()
    skipped = grid_cases.ambiguous(expected, grid_cases.QUERY_BOUND)
    print("%s: %d of %d segments within %.3e of their target" % (name, skipped.sum(), len(skipped), grid_cases.QUERY_BOUND))
    assert skipped.mean() <= 0.01
    assert grid_cases.QUERY_BOUND < 0.5 * grid_cases.JUST   # "just met" and "just missed" are decided, not ties
