"""A float64 reference for the BasicVolumeIntegrator over Henyey-Greenstein media (k_path_aniso / k_path_aniso_grid, DESIGN.md
§4.4g): the random walk of tests/multiple_scattering_reference.py -- its scene family, its accounting, its unchanged helpers --
with the two statements the phase function enters restated (pathed_amd/csrc/volume.h):

  * the light sample of a scatter point: a uniformly drawn direction wi towards the environment (pdf 1 / 4 pi) carries
    environment(wi) * p(w, wi) / (1 / 4 pi), with p the Henyey-Greenstein value
        x = (1 + g^2) - 2 g c,   p = (1 - g^2) / (x sqrt(x)) / (4 pi),   c = w . wi,
    and w the unit propagation direction of the segment the event lies on;
  * the direction after the event is drawn from p:
        s = (1 - g^2) / ((1 - g) + 2 g u1),   c = ((1 + g^2) - s^2) / (2 g) clamped to [-1, 1],   phi = 2 pi u2,
        direction = x_axis sin(theta) cos(phi) + w c + z_axis sin(theta) sin(phi)
    in the frame normalToWorldSpace1(w) of pathed_amd/csrc/shading.h: x_axis = normalized(-w.z, 0, w.x) where |w.x| > |w.y|,
    normalized(0, -w.z, w.y) otherwise, z_axis = w x x_axis.  The pdf is the value: the weight after the sample is 1.
  * a medium with |g| < 1e-3 scatters isotropically (the kernels' threshold).

The environment is a FUNCTION of the direction a ray leaves in (None: radiance 1 everywhere).  `texel_environment` makes one
from a latitude-longitude map by the texel rule of the device's envEmit (theta from +y, phi = atan2(z, x), floor(size * angle /
range) clamped to the last texel), so a map that is constant on each half is the same function on both sides.

g is one number per medium of the scene family (outer container, inner container)."""
import functools

import numpy as np

from multiple_scattering_reference import STACK_DEPTH, T_LIGHT, Scene, _closest, _cosine_hemisphere, _events, _uniform_sphere, mean_and_deviation  # noqa: F401

ISOTROPIC_BELOW = 1e-3


def texel_environment(radiance, to_map=np.eye(3)):
    """radiance: (height, width) texel values; to_map: the 3 x 3 rotation from the walk's frame into the map's"""
    radiance = np.asarray(radiance, dtype=np.float64)
    height, width = radiance.shape
    to_map = np.asarray(to_map, dtype=np.float64)

    def environment(direction):
        local = direction @ to_map.T
        local = local / np.linalg.norm(local, axis=1, keepdims=True)
        phi = np.arctan2(local[:, 2], local[:, 0])
        phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
        theta = np.arccos(np.clip(local[:, 1], -1.0, 1.0))
        column = np.minimum(np.floor(width * np.clip(phi / (2.0 * np.pi), 0.0, 1.0)).astype(np.int64), width - 1)
        row = np.minimum(np.floor(height * np.clip(theta / np.pi, 0.0, 1.0)).astype(np.int64), height - 1)
        return radiance[row, column]
    return environment


def hg_value(g, cosine):
    """p(w, wi) for c = w . wi; g and cosine broadcast"""
    g = np.asarray(g, dtype=np.float64)
    x = (1.0 + g * g) - 2.0 * g * cosine
    return (1.0 - g * g) / (x * np.sqrt(x)) / (4.0 * np.pi)


def hg_cosine(g, u1):
    """the sampled cosine; g != 0"""
    g = np.asarray(g, dtype=np.float64)
    s = (1.0 - g * g) / ((1.0 - g) + 2.0 * g * u1)
    return np.clip(((1.0 + g * g) - s * s) / (2.0 * g), -1.0, 1.0), s


def frame(w):
    """(x_axis, z_axis) of normalToWorldSpace1(w), rows of unit vectors"""
    wide = np.abs(w[:, 0]) > np.abs(w[:, 1])
    zero = np.zeros(len(w))
    x_axis = np.where(wide[:, None], np.stack([-w[:, 2], zero, w[:, 0]], axis=1), np.stack([zero, -w[:, 2], w[:, 1]], axis=1))
    x_axis = x_axis / np.linalg.norm(x_axis, axis=1, keepdims=True)
    return x_axis, np.cross(w, x_axis)


def hg_direction(g, w, u1, u2):
    """the sampled direction about the unit vectors w (n, 3); g (n,) or a number, |g| >= ISOTROPIC_BELOW"""
    cosine, _ = hg_cosine(g, u1)
    sine = np.sqrt(np.maximum(0.0, 1.0 - cosine * cosine))
    phi = 2.0 * np.pi * u2
    x_axis, z_axis = frame(w)
    return x_axis * (sine * np.cos(phi))[:, None] + w * cosine[:, None] + z_axis * (sine * np.sin(phi))[:, None]


def _phase_sample(rng, g, w):
    isotropic = np.abs(g) < ISOTROPIC_BELOW
    direction = hg_direction(np.where(isotropic, 0.5, g), w, rng.random(len(w)), rng.random(len(w)))
    direction[isotropic] = _uniform_sphere(rng, int(isotropic.sum()))
    return direction


def _phase_times_four_pi(g, w, wi):
    isotropic = np.abs(g) < ISOTROPIC_BELOW
    return np.where(isotropic, 1.0, hg_value(np.where(isotropic, 0.0, g), np.einsum("ij,ij->i", w, wi)) * (4.0 * np.pi))


def walk(scene, n, last_bounces, g=(0.0, 0.0), environment=None, start_bounce=0, seed=1):
    """n walks.  Returns ({last bounce: per-walk values (n,)}, info), as multiple_scattering_reference.walk (its "stack" rule)."""
    g = np.broadcast_to(np.asarray(g, dtype=np.float64), (2,)) if np.ndim(g) == 0 else np.asarray(g, dtype=np.float64)
    emitted = environment if environment is not None else (lambda direction: np.ones(len(direction)))
    last_bounces = sorted(int(last) for last in last_bounces)
    assert last_bounces[0] >= max(1, start_bounce)
    rng = np.random.default_rng(seed)
    half = np.tan(np.radians(scene.fov_degrees) / 2.0)
    direction = np.stack([half * (2.0 * rng.random(n) - 1.0), half * (2.0 * rng.random(n) - 1.0), -np.ones(n)], axis=1)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    origin = np.tile([0.0, 0.0, scene.distance], (n, 1))

    value = np.zeros(n)
    snapshots, info = {}, {"surface_counted": 0, "dropped": 0}
    counts = lambda bounce, last: start_bounce <= bounce <= last

    # ---- the camera ray, bounce 0 (SampleIntegrator::samplePixel)
    t, surface, entering = _closest(scene, origin, direction)
    hit = np.isfinite(t)
    value[~hit] = emitted(direction[~hit])
    if start_bounce == 0:
        container = hit & ((surface == 0) | (scene.inner == "container"))
        count, t0, t1, blocked, medium0 = _events(scene, origin, direction, np.where(hit, np.inf, 0.0))
        sigma0 = scene.sigma[medium0]
        with np.errstate(invalid="ignore"):      # (inf - inf where there are no two events)
            through = np.where(count >= 2, np.exp(-sigma0 * (t1 - t0)), np.where(count == 1, np.exp(-sigma0 * t0), 1.0))
        value += np.where(container & ~blocked, through * emitted(direction), 0.0)

    # ---- BasicVolumeIntegrator::L on the walks that hit something; state is kept for the live walks only
    alive = np.nonzero(hit)[0]
    position = origin[alive] + direction[alive] * t[alive][:, None]
    direction, surface, entering = direction[alive], surface[alive], entering[alive]
    weight = np.ones(len(alive))
    stack = np.full((len(alive), STACK_DEPTH), -1, dtype=np.int64)
    depth = np.zeros(len(alive), dtype=np.int64)
    on_surface = np.ones(len(alive), dtype=bool)      # interaction.isSurface
    crossing = np.zeros(len(alive), dtype=bool)       # the surface interaction changes sides (wo, wi on different sides)

    def at_surface(bounce, surface, position, direction):
        """a vertex on a surface: the BSDF sample.  Returns (new direction, crosses, weight after the NEXT segment is found)"""
        ball = (surface == 1) & (scene.inner == "lambertian")
        if ball.any():
            if any(counts(bounce, last) for last in last_bounces):
                info["surface_counted"] += int(ball.sum())
            normal = position[ball] / scene.inner_radius
            direction = direction.copy()
            direction[ball] = _cosine_hemisphere(rng, normal)
        return direction, ~ball, np.where(ball, scene.rho, 1.0)

    direction, crossing, pending = at_surface(1, surface, position, direction)
    if 1 in last_bounces:
        snapshots[1] = value.copy()
    for bounce in range(2, last_bounces[-1] + 1):
        if len(alive) == 0:
            break
        t, next_surface, next_entering = _closest(scene, position, direction)
        keep = np.isfinite(t)
        weight = np.where(on_surface, weight * pending, weight)
        keep &= weight > 0.0
        # updateMediumPtrs: `surface` / `entering` describe the surface the interaction lies on
        change = keep & on_surface & crossing
        medium = np.where(surface == 0, 0, 1 if scene.inner == "container" else -1)
        push = change & entering
        full = push & (depth >= STACK_DEPTH)
        info["dropped"] += int(full.sum())
        value[alive[full]] = 0.0
        for last in snapshots:
            snapshots[last][alive[full]] = 0.0
        keep &= ~full
        push &= ~full
        stack[push, depth[push]] = medium[push]
        depth[push] += 1
        leave = np.nonzero(change & ~entering)[0]
        if len(leave):
            equal = (stack[leave] == medium[leave][:, None]) & (np.arange(STACK_DEPTH) < depth[leave][:, None])
            found = equal.any(axis=1)
            first = np.argmax(equal, axis=1)
            rows, at = leave[found], first[found]
            columns = np.arange(STACK_DEPTH)
            source = np.minimum(columns + (columns >= at[:, None]), STACK_DEPTH - 1)      # the entries above `at` move down
            moved = stack[rows[:, None], source]
            moved[:, -1] = -1
            stack[rows] = moved
            depth[rows] -= 1

        # compaction: the walks that go on
        index = np.nonzero(keep)[0]
        alive, position, direction, t = alive[index], position[index], direction[index], t[index]
        surface, entering, weight = next_surface[index], next_entering[index], weight[index]
        stack, depth = stack[index], depth[index]
        m = len(alive)
        current = np.where(depth > 0, stack[np.arange(m), np.maximum(depth - 1, 0)], -1)

        # scatter(current medium, interaction.point(), hit point)
        sigma = np.where(current >= 0, scene.sigma[np.maximum(current, 0)], 0.0)
        with np.errstate(divide="ignore"):
            sample_t = np.where(sigma > 0.0, -np.log(1.0 - rng.random(m)) / sigma, np.inf)
        scatters = (current >= 0) & (sample_t < t)
        position = position + direction * np.where(scatters, sample_t, t)[:, None]

        rows = np.nonzero(scatters)[0]
        weight[rows] *= scene.albedo[current[rows]]
        mean_cosine = g[current[rows]]
        along = direction[rows]      # w: the segment's propagation direction
        towards = _uniform_sphere(rng, len(rows))
        count, t0, t1, blocked, _ = _events(scene, position[rows], towards, np.full(len(rows), T_LIGHT))
        sigma_here = sigma[rows]
        with np.errstate(invalid="ignore"):
            shadow = np.where(count >= 2, np.exp(-sigma_here * (t1 - t0)), np.where(count == 1, np.exp(-sigma_here * t0), 0.0))
        lit = emitted(towards) * _phase_times_four_pi(mean_cosine, along, towards)
        value[alive[rows]] += np.where(blocked, 0.0, shadow) * lit * weight[rows]      # not gated by the window
        direction[rows] = _phase_sample(rng, mean_cosine, along)

        # ... or the surface at the segment's end becomes the interaction
        on_surface = ~scatters
        stays = np.nonzero(on_surface)[0]
        new_direction, crosses, factor = at_surface(bounce, surface[stays], position[stays], direction[stays])
        direction[stays] = new_direction
        crossing = np.zeros(m, dtype=bool)
        crossing[stays] = crosses
        pending = np.ones(m)
        pending[stays] = factor
        if bounce in last_bounces:
            snapshots[bounce] = value.copy()
    for last in last_bounces:
        snapshots.setdefault(last, value.copy())
    return snapshots, info


# ---- the configurations the tests share: computed once per process, never changed afterwards
WALKS = 1000000
DISTANCE, FOV = 5.0, 24.0
BACK_LIT_ROWS = 32      # the two-tone map: theta >= pi / 2 (map y < 0) reads 2, the rest 0; the split is the edge of row 16
TO_MAP = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])      # walk (x, y, z) -> map (x, z, -y): the walk's +z is the map's pole


def back_lit_map(width=64):
    radiance = np.zeros((BACK_LIT_ROWS, width))
    radiance[BACK_LIT_ROWS // 2:] = 2.0
    return radiance


@functools.lru_cache(maxsize=None)
def shared_walk(last_bounces, g, environment="constant", **scene):
    """{last bounce: (mean, standard deviation)} of 10^6 walks of Scene(**scene) with the outer medium's mean cosine g under the
    "constant" (radiance 1) or the "back-lit" environment (radiance 2 on directions with z < 0, the camera is on +z)"""
    assert environment in ("constant", "back-lit")
    emitted = texel_environment(back_lit_map(), TO_MAP) if environment == "back-lit" else None
    values, info = walk(Scene(distance=DISTANCE, fov_degrees=FOV, **scene), WALKS, last_bounces, g=(g, 0.0), environment=emitted)
    assert info["dropped"] == 0 and info["surface_counted"] == 0, info
    return {last: mean_and_deviation(values[last]) for last in last_bounces}
