"""The float64 yardstick of the grid medium (tests/grid_reference.py) against the reference's own fixtures: every case of the
reference's test/grid_medium_test.cpp, restated as numbers (grid_reference.reference_fixtures), to Catch's default Approx
(relative 100 x FLT_EPSILON).  No GPU: this pins the yardstick the GPU tests are held against."""
import numpy as np
import pytest

import grid_reference
from grid_reference import GridReference

FIXTURES = grid_reference.reference_fixtures()


def fixture_grid(cells, bounds, density, dtype=np.float64):
    return GridReference(np.full((cells[2], cells[1], cells[0]), density), bounds, dtype=dtype)


def test_the_fixture_list_covers_the_reference_file():
    names = [case[0] for case in FIXTURES]
    assert len(names) == len(set(names)) == 31
    for wanted in ("2x2x2 across", "resolution 2x2x2 find full", "resolution 20x5x20 find full", "full 20x5x20 across", "extents find fraction", "threshold not met, exits outside",
                   "threshold not met, exits inside", "miss", "unclamped start", "unclamped end", "exit inside", "start inside",
                   "fully inside", "33x33x33 fully inside"):
        assert wanted in names


def check_fixture(case, dtype):
    """runs one case; returns None when it holds, else (why, |accumulated exponent - target exponent| / target exponent) of a
    findTransmittance case whose validity differs from the reference's"""
    name, cells, bounds, density, entry, leave, kind, argument, expected = case
    grid = fixture_grid(cells, bounds, density, dtype)
    if kind == "T":
        value, _, hit_bound = grid.transmittance([entry], [leave])
        assert not hit_bound.any()
        assert value.dtype == dtype and grid_reference.approx(float(value[0]), expected), (value[0], expected)
        return None
    valid, distance, exponent, target_exponent, hit_bound = grid.find_transmittance([entry], [leave], [argument])
    assert not hit_bound.any() and distance.dtype == dtype
    if bool(valid[0]) != (expected is not None):
        return "validity", abs(float(exponent[0]) - float(target_exponent[0])) / float(target_exponent[0])
    if expected is None:
        assert distance[0] == -1.0
    else:
        assert grid_reference.approx(float(distance[0]), expected), (distance[0], expected)
    return None


@pytest.mark.parametrize("case", FIXTURES, ids=[case[0] for case in FIXTURES])
def test_yardstick_meets_the_reference_fixture(case):
    """Every case holds in float64, with one kind of exception that float64 itself explains: the two "find full" cases whose
    target is exp(-sigma_t x length) exactly (REQUIRE(result.isValid) on a tie).  The target was rounded to a float, its
    exponent is 1.2e-8 and 1.3e-8 ABOVE the accumulated one (0.03 and 0.006 of FLT_EPSILON relative), so exact arithmetic says
    "not met" and float32, where -logf(target) rounds onto the accumulated exponent, says "met".  Such a case must be a tie
    to well within one float32 rounding, and the same code in float32 -- the reference's own precision -- must give the
    reference's answer."""
    outcome = check_fixture(case, np.float64)
    if outcome is not None:
        assert case[0] in ("2x2x2 find full", "extents find full"), case[0]
        assert outcome[1] < 0.5 * float(np.finfo(np.float32).eps), outcome
    assert check_fixture(case, np.float32) is None


def test_trilinear_lookup_and_its_range():
    """UniformGrid::interpolate: the corner values at the corners, the mean in the middle, 0 outside [0, cells - 1]"""
    rng = np.random.default_rng(3)
    data = rng.uniform(0.0, 2.0, (5, 4, 3))
    grid = GridReference(data, (0, 0, 0, 1, 1, 1))
    corners = np.array([(x, y, z) for z in (1, 2) for y in (2, 3) for x in (0, 1)], dtype=np.float64)
    assert np.array_equal(grid.interpolate(corners), data[corners[:, 2].astype(int), corners[:, 1].astype(int), corners[:, 0].astype(int)])
    assert np.isclose(grid.interpolate(np.array([[0.5, 2.5, 1.5]]))[0], data[1:3, 2:4, 0:2].mean())
    outside = np.array([[-1e-9, 1, 1], [2.0000001, 1, 1], [1, 3.0000001, 1], [1, 1, 4.0000001], [np.nan, 1, 1]])
    assert np.array_equal(grid.interpolate(outside), np.zeros(5))
    assert grid.interpolate(np.array([[2.0, 3.0, 4.0]]))[0] == data[4, 3, 2]


def test_the_step_bound_is_reported():
    """a walk cut off by max_steps says so; a clipped segment never needs more than cells x + y + z + 3 steps"""
    grid = fixture_grid((20, 5, 20), (0, 0, 0, 1, 1, 1), 0.6)
    a, b = [(0.0, 0.013, 0.021)], [(1.0, 0.987, 0.979)]
    _, _, hit_bound = grid.transmittance(a, b, max_steps=5)
    assert hit_bound[0]
    value, exponent, hit_bound = grid.transmittance(a, b)
    assert not hit_bound[0]
    assert np.isclose(exponent[0], 0.6 * np.linalg.norm(np.subtract(b, a)), rtol=1e-12)
