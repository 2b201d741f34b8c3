"""The grid medium's device functions (pathed_amd/csrc/grid_medium.h: gridTransmittance, gridFindTransmittance and below them
the box clip, the regular tracker and the trilinear lookup), pinned through the hook pathed_hip_grid_queries, below the image.

  1. the cases of the reference's test/grid_medium_test.cpp (grid_reference.reference_fixtures), to Catch's default Approx;
  2. 4 096 random segments on each of three grids (grid_cases.query_inputs: both ends outside, one inside, both inside,
     axis-parallel, through an edge, through a corner, in a cell face; targets met, just met, just missed, far missed) against
     the float64 yardstick, to QUERY_BOUND; validity must agree except for ties (grid_cases.ambiguous), of which there are
     at most 1 %.

QUERY_MEASURED (grid_cases.py) is the largest relative difference, of transmittance or distance, that an MI355X showed over
all of 2.; the bound is four times it.
"""
import numpy as np
import pytest

import grid_cases
import grid_reference
import volume_scenes as vs
from scene_builder import BuiltScene

pytestmark = pytest.mark.gpu


def _scene():
    """any scene with a medium slot: the hook runs on the slot's grid, the geometry does not matter"""
    from pathed_amd.integrator import HipScene
    built = BuiltScene(8, 8, (0, 0, 5), (0, 0, 0), fov_degrees=30)
    vs.enclosure(built)
    built.box((-1, -1, -1), (1, 1, 1), vs.passthrough(built), medium=vs.gas(built, 0.0))
    return HipScene(built.finish(), device=0)


@pytest.fixture(scope="module")
def scene():
    return _scene()


def test_reference_fixtures_on_the_device(scene):
    failures = []
    for name, cells, bounds, density, entry, leave, kind, argument, expected in grid_reference.reference_fixtures():
        grid_cases.GridCase(np.full((cells[2], cells[1], cells[0]), density), bounds).set_on(scene, 0)   # replaces the slot's grid
        transmittance, distance = scene.grid_queries(0, [entry], [leave], [0.5 if argument is None else argument])
        if kind == "T":
            ok = grid_reference.approx(float(transmittance[0]), expected)
            print("%-40s transmittance %.9g expected %.9g" % (name, transmittance[0], expected))
        elif expected is None:
            ok = distance[0] == -1.0
            print("%-40s distance %.9g expected invalid" % (name, distance[0]))
        else:
            ok = grid_reference.approx(float(distance[0]), expected)
            print("%-40s distance %.9g expected %.9g" % (name, distance[0], expected))
        if not ok:
            failures.append(name)
    assert not failures, failures


@pytest.mark.parametrize("name", sorted(grid_cases.query_grids()))
def test_random_segments_against_the_yardstick(scene, name):
    (a, b, target), (category, kind), expected = grid_cases.query_inputs(name)
    grid_cases.query_grids()[name].set_on(scene, 0)
    transmittance, distance = scene.grid_queries(0, a, b, target)
    assert np.isfinite(transmittance).all() and np.isfinite(distance).all()

    relative_t = np.abs(transmittance.astype(np.float64) - expected["transmittance"]) / expected["transmittance"]
    valid = distance != -1.0
    skipped = grid_cases.ambiguous(expected, grid_cases.QUERY_BOUND)
    both = valid & expected["valid"]
    relative_d = np.zeros(len(a))
    relative_d[both] = np.abs(distance[both].astype(np.float64) - expected["distance"][both]) / expected["distance"][both]
    for k, label in enumerate(grid_cases.CATEGORIES):
        chosen = category == k
        print("%s %-15s transmittance %.3e  distance %.3e" % (name, label, relative_t[chosen].max(), relative_d[chosen].max()))
    disagree = (valid != expected["valid"]) & ~skipped
    with np.errstate(all="ignore"):
        closeness = np.abs(expected["exponent"] - expected["target_exponent"]) / np.abs(expected["target_exponent"])
    print("%s: largest relative difference %.4e (transmittance %.4e, distance %.4e); ties skipped %d; validity differs on %d (closest tie %.3e)"
          % (name, max(relative_t.max(), relative_d.max()), relative_t.max(), relative_d.max(), skipped.sum(), disagree.sum(),
             closeness[valid != expected["valid"]].min() if (valid != expected["valid"]).any() else np.inf))
    assert skipped.mean() <= 0.01
    assert not disagree.any()
    assert relative_t.max() <= grid_cases.QUERY_BOUND and relative_d.max() <= grid_cases.QUERY_BOUND


def test_hook_refuses_a_slot_without_a_grid():
    from pathed_amd.integrator import PathedError
    scene = _scene()
    with pytest.raises(PathedError, match="holds no grid"):
        scene.grid_queries(0, [(0, 0, 0)], [(1, 0, 0)], [0.5])


def test_set_grid_medium_errors():
    """index out of range, cells < 2, non-finite bounds or data, struct_size, a scene without media"""
    import ctypes
    from pathed_amd import _capi
    from pathed_amd.integrator import HipScene, PathedError
    scene = _scene()
    data = np.ones((2, 2, 2), dtype=np.float32)
    unit = (0, 0, 0, 1, 1, 1)
    with pytest.raises(PathedError, match="out of range"):
        scene.set_grid_medium(1, data=data, bounds=unit)
    with pytest.raises(PathedError, match="out of range"):
        scene.set_grid_medium(-1, data=data, bounds=unit)
    with pytest.raises(PathedError, match="at least 2 cells"):
        scene.set_grid_medium(0, data=np.ones((2, 1, 2), dtype=np.float32), bounds=unit)
    with pytest.raises(PathedError, match="bounds must be finite"):
        scene.set_grid_medium(0, data=data, bounds=(0, 0, 0, 1, np.inf, 1))
    bad = data.copy()
    bad[1, 0, 1] = np.nan
    with pytest.raises(PathedError, match="data must be finite"):
        scene.set_grid_medium(0, data=bad, bounds=unit)
    grid = _capi.PathedGridMedium()
    lib = _capi.load_hip()
    grid.struct_size = ctypes.sizeof(_capi.PathedGridMedium) - 4
    assert lib.pathed_hip_scene_set_grid_medium(scene._handle, 0, ctypes.byref(grid)) == -1
    assert b"struct_size" in lib.pathed_hip_last_error()
    built = BuiltScene(8, 8, (0, 0, 5), (0, 0, 0), fov_degrees=30)
    vs.enclosure(built)
    with pytest.raises(PathedError, match="no media"):
        HipScene(built.finish(), device=0).set_grid_medium(0, data=data, bounds=unit)
    # nothing of the failures stuck: the slot still holds no grid
    with pytest.raises(PathedError, match="holds no grid"):
        scene.grid_queries(0, [(0, 0, 0)], [(1, 0, 0)], [0.5])
