"""tests/multiple_scattering_reference.py, the float64 random walk that stands in for an oracle of the BasicVolumeIntegrator
(tests/test_gpu_basic_volume.py), held to the one closed form there is: the white furnace.  A medium of albedo 1 inside a
constant environment of radiance 1 neither adds nor removes light, so every pixel is 1 once all scattering orders count."""
import numpy as np

import multiple_scattering_reference as reference


def test_white_furnace():
    """sphere R = 1, sigma = 2, albedo 1, D = 5, fov 24 degrees, window (0, 40): the mean is 1 within 5 of its own standard
    errors (2 * 10^6 walks gave 1.0002 +- 0.0005 when the walk was written; what the window cuts off is below 1e-4)."""
    walks = 400000
    values, info = reference.walk(reference.Scene(radius=1.0, sigma=2.0, albedo=1.0, distance=5.0, fov_degrees=24.0), walks, (40,))
    mean, deviation = reference.mean_and_deviation(values[40])
    error = deviation / np.sqrt(walks)
    print("white furnace: %.5f +- %.5f" % (mean, error), info)
    assert info["dropped"] == 0 and info["surface_counted"] == 0
    assert abs(mean - 1.0) <= 5.0 * error and error <= 0.002


def test_an_absorbing_medium_loses_light_and_single_scattering_is_darker():
    values, _ = reference.walk(reference.Scene(albedo=0.8), 200000, (2, 12))
    white, _ = reference.walk(reference.Scene(albedo=1.0), 200000, (2, 12))
    assert values[2].mean() < values[12].mean() < white[12].mean() < 1.0
    assert np.array_equal(values[2] <= values[12], np.ones(200000, dtype=bool))      # further orders only add


def test_the_stack_rule_matters_with_a_nested_container():
    """leaving the inner container: the stack is back in the outer gas, the single pointer in none"""
    scene = reference.Scene(inner="container", inner_radius=0.45, inner_sigma=6.0)
    stack, _ = reference.walk(scene, 200000, (12,))
    clear, _ = reference.walk(scene, 200000, (12,), stack_rule="clear")
    assert stack[12].mean() - clear[12].mean() >= 0.03


def test_a_window_that_starts_late_keeps_the_missed_rays_and_the_scatter_terms():
    """window (40, 40): no bounce-0 term behind the container, but the rays that miss everything and every scatter term"""
    scene = reference.Scene(inner="lambertian", rho=0.5)
    late, info = reference.walk(scene, 100000, (40,), start_bounce=40)
    full, _ = reference.walk(scene, 100000, (40,), start_bounce=0)
    assert info["surface_counted"] == 0
    assert 0.276 - 0.01 <= (late[40] == 1.0).mean() <= 0.276 + 0.01      # the frame around the sphere's silhouette
    assert late[40].mean() < full[40].mean()
