"""The float64 walk over Henyey-Greenstein media (tests/anisotropic_scattering_reference.py) held to what does not depend on
any kernel, before tests/test_gpu_anisotropic.py holds the device to the walk:
  * the white furnace: a constant environment, albedo 1, window (0, 60) -- whatever g, every pixel sees radiance 1;
  * the sample's mean cosine is g (the defining property of the function), on a lattice of sample numbers;
  * the sample is distributed as the value says (the pdf is the value): lattice moments of the second Legendre polynomial, g^2;
  * g = -0.7, 0 and +0.7 are told apart under the back-lit environment by at least five tolerances.
Tolerance: tests/test_gpu_basic_volume.py's rule, 7.5 x the walk's own deviation x sqrt(1 / (128 x 128 x 64) + 1 / 10^6)."""
import numpy as np
import pytest

import anisotropic_scattering_reference as reference

SIZE, SPP = 128, 64


def _tolerance(deviation):
    return 7.5 * deviation * np.sqrt(1.0 / (SIZE * SIZE * SPP) + 1.0 / reference.WALKS)


@pytest.mark.parametrize("g", [0.7, -0.7])
def test_white_furnace(g):
    mean, deviation = reference.shared_walk((60,), g)[60]
    print("g %+.1f: %.5f  tolerance %.5f" % (g, mean, _tolerance(deviation)))
    assert _tolerance(deviation) <= 0.03      # the comparison means something
    assert abs(mean - 1.0) <= _tolerance(deviation), (g, mean, deviation)


@pytest.mark.parametrize("g", [0.7, -0.7, 0.3, -0.9, 0.05])
def test_lattice_moments_of_the_sample(g):
    """Midpoint lattice over (u1, u2), 4 096 x 16, about four directions w (both branches of the frame).  The integral of c over
    u1 is g exactly and that of P2(c) = (3 c^2 - 1) / 2 is g^2 (the Legendre moments of Henyey-Greenstein); the midpoint rule's
    error is h^2 / 24 x max |d^2/du1^2|, below 2e-5 for |g| <= 0.9 at h = 1 / 4096 (c'' <= 12 |g| s^2 / d^2 with s <= 1 + |g|,
    d >= 1 - |g|: 4 300 at 0.9, 4 300 / 24 / 4096^2 = 1.1e-5)."""
    steps_1, steps_2 = 4096, 16
    u1 = np.repeat((np.arange(steps_1) + 0.5) / steps_1, steps_2)
    u2 = np.tile((np.arange(steps_2) + 0.5) / steps_2, steps_1)
    for w in ([0.0, 0.0, -1.0], [0.6, 0.0, 0.8], [0.48, 0.6, -0.64], [-0.1, 0.9949874371066199, 0.0]):
        w = np.tile(np.asarray(w, dtype=np.float64), (len(u1), 1))
        direction = reference.hg_direction(g, w, u1, u2)
        cosine = np.einsum("ij,ij->i", w, direction)
        assert np.abs(np.linalg.norm(direction, axis=1) - 1.0).max() <= 1e-12
        assert abs(cosine.mean() - g) <= 2e-5, (g, cosine.mean())
        assert abs((1.5 * cosine * cosine - 0.5).mean() - g * g) <= 1e-4, g
        # ... and the azimuth is uniform about w: the mean direction is g w
        assert np.abs(direction.mean(axis=0) - g * w[0]).max() <= 2e-5
    # the value integrates to 1 over the sphere and is the sample's density: d c / d u1 = 1 / (2 pi p(c))
    cosine, _ = reference.hg_cosine(g, (np.arange(steps_1) + 0.5) / steps_1)
    slope = np.gradient(cosine, 1.0 / steps_1)[8:-8]
    assert np.allclose(slope * 2.0 * np.pi * reference.hg_value(g, cosine[8:-8]), 1.0, rtol=2e-3)


def test_back_lit_environment_tells_the_mean_cosines_apart():
    windows = (2, 12)
    found = {g: reference.shared_walk(windows, g, "back-lit") for g in (-0.7, 0.0, 0.7)}
    for last in windows:
        means = [found[g][last][0] for g in (-0.7, 0.0, 0.7)]
        tolerances = [_tolerance(found[g][last][1]) for g in (-0.7, 0.0, 0.7)]
        print("window (0, %d): means %s  tolerances %s" % (last, means, tolerances))
        assert means[0] < means[1] < means[2]      # forward scattering carries the light behind the medium to the camera
        for a, b in ((0, 1), (1, 2)):
            assert means[b] - means[a] >= 5.0 * max(tolerances[a], tolerances[b]), (last, means, tolerances)


def test_the_environment_is_the_texel_rule():
    """the two-tone map read through the walk's frame: radiance 2 on directions with z < 0, 0 on the others, up to the split"""
    environment = reference.texel_environment(reference.back_lit_map(), reference.TO_MAP)
    rng = np.random.default_rng(5)
    direction = rng.normal(size=(4096, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    assert np.array_equal(environment(direction), np.where(direction[:, 2] < 0.0, 2.0, 0.0))
