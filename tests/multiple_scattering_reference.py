"""A float64 reference for the BasicVolumeIntegrator (reference src/basic_volume_integrator.cpp:25-197): a vectorised numpy
random walk over one small family of scenes.  It restates the estimator's ACCOUNTING -- the bounce counter and the bounce
window, the stack of media, which boundary crossings become volume events, what bounce 0 adds -- and none of the kernel's
arithmetic: the geometry is analytic (a sphere or a box, not triangles), the numbers are float64, the random numbers numpy's.

The scene family
  * one convex container around the origin, a sphere of radius `radius` or the axis-aligned box `box` = (lo, hi), holding
    medium 0 (sigma, albedo); its surface is a passthrough surface: it takes a bounce and leaves direction and weight alone;
  * optionally a concentric inner sphere of radius `inner_radius`: a second container holding medium 1 (`inner` =
    "container") or an opaque Lambertian ball of reflectance `rho` (`inner` = "lambertian");
  * a constant environment of radiance 1, no other light; a pinhole at (0, 0, distance) looking at the origin, whose rays go
    through points drawn uniformly over the square frame -- the distribution of jittered camera rays summed over a square image.

The estimator, as the reference states it
  * a camera ray that hits nothing sees the environment, whatever the bounce window (src/sample_integrator.cpp:20-23);
  * bounce 0 (counted when the window starts at 0): a container seen first adds "what is seen through it"
    (src/sample_integrator.cpp:35-51) -- the environment times rayTransmission with NO current medium
    (src/volume_helper.cpp:100-118), zero where an opaque surface is behind it;
  * every surface the path meets is a vertex and takes a bounce, containers included; a path that changes sides at a surface
    pushes the surface's medium ("none" for a surface without one) going in and erases the first equal entry going out
    (updateMediumPtrs, :145-174); the current medium is the top of the stack;
  * every segment samples a distance -log(1 - u) / sigma in the current medium; short of the segment's end the path scatters:
    weight *= albedo, the point is lit (below), the path turns into a uniformly drawn direction, and the bounce is used up;
  * the light sample of a scatter point (src/volume_helper.cpp:12-69): a uniformly drawn direction towards the environment
    (pdf 1 / 4 pi, phase function 1 / 4 pi: the two cancel), zero when an opaque surface is in the way, otherwise the
    transmittance of the CURRENT medium between the events -- the boundary crossings of containers along the ray, sorted by t,
    the nearest two used: one event exp(-sigma t0), two events exp(-sigma (t1 - t0)), no event 0;
  * scatter points are lit whatever the bounce window says (:99-101); surface lighting is window-gated, is zero on a container,
    and is NOT restated for the Lambertian ball: `surface_counted` reports how many walks stood on the ball at a bounce the
    window counts, and a comparison is meaningful only where that is zero;
  * every query ignores hits with t <= 1e-3, the project's ray interval, so that the paths that leak through a boundary they
    start on are the same ones.

`stack_rule="clear"` replaces the stack by VolumePathTracer's single pointer (src/volume_path_tracer.cpp:43-51): entering sets
it, leaving ANYTHING clears it.  It exists so that a test can show the two rules apart before it relies on the right one."""
import numpy as np

T_NEAR = 1e-3
T_LIGHT = 1e4 - 1e-3      # the environment's sample point lies 1e4 away; the occlusion query stops 1e-3 short of it
STACK_DEPTH = 4


class Scene:
    def __init__(self, radius=1.0, box=None, sigma=2.0, albedo=1.0, inner=None, inner_radius=0.45, inner_sigma=6.0,
                 inner_albedo=1.0, rho=0.5, distance=5.0, fov_degrees=24.0):
        assert inner in (None, "container", "lambertian")
        self.radius, self.box = float(radius), box
        self.sigma = np.array([sigma, inner_sigma], dtype=np.float64)
        self.albedo = np.array([albedo, inner_albedo], dtype=np.float64)
        self.inner, self.inner_radius, self.rho = inner, float(inner_radius), float(rho)
        self.distance, self.fov_degrees = float(distance), float(fov_degrees)


def _sphere_roots(o, d, radius):
    """both crossings of the unit-direction rays (o, d) with the sphere |x| = radius: (n, 2), inf where there is none"""
    b = np.einsum("ij,ij->i", o, d)
    c = np.einsum("ij,ij->i", o, o) - radius * radius
    disc = b * b - c
    root = np.sqrt(np.where(disc >= 0.0, disc, 0.0))
    roots = np.stack([-b - root, -b + root], axis=1)
    roots[disc < 0.0] = np.inf
    return roots


def _box_roots(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (np.asarray(lo, dtype=np.float64) - o) / d
        t1 = (np.asarray(hi, dtype=np.float64) - o) / d
    near = np.nanmax(np.fmin(t0, t1), axis=1)
    far = np.nanmin(np.fmax(t0, t1), axis=1)
    roots = np.stack([near, far], axis=1)
    roots[near > far] = np.inf
    return roots


def _crossings(scene, o, d):
    """(outer roots, inner roots): (n, 2) each, column 0 is the crossing INTO the convex body, column 1 the one out of it"""
    outer = _box_roots(o, d, *scene.box) if scene.box is not None else _sphere_roots(o, d, scene.radius)
    inner = _sphere_roots(o, d, scene.inner_radius) if scene.inner else np.full_like(outer, np.inf)
    return outer, inner


def _usable(roots):
    return np.where(roots > T_NEAR, roots, np.inf)


def _closest(scene, o, d):
    """Scene::testIntersect: (t, surface 0 outer / 1 inner, entering); t = inf on a miss"""
    outer, inner = _crossings(scene, o, d)
    both = _usable(np.concatenate([outer, inner], axis=1))      # columns: outer in, outer out, inner in, inner out
    column = np.argmin(both, axis=1)
    t = both[np.arange(len(both)), column]
    return t, column >> 1, (column & 1) == 0


def _events(scene, o, d, limit):
    """the two nearest container crossings in (1e-3, limit): (count, t0, t1, opaque surface in the way, medium of event 0)"""
    outer, inner = _crossings(scene, o, d)
    blocked = np.zeros(len(o), dtype=bool)
    if scene.inner == "lambertian":
        ball = _usable(inner).min(axis=1)
        blocked = np.isfinite(ball) & (ball <= limit)
        crossings, media = _usable(outer), np.zeros_like(outer, dtype=np.int64)
    else:
        crossings = _usable(np.concatenate([outer, inner], axis=1))
        media = np.broadcast_to(np.array([0, 0, 1, 1]), crossings.shape)
    crossings = np.where(crossings < limit[:, None], crossings, np.inf)
    order = np.argsort(crossings, axis=1)[:, :2]
    rows = np.arange(len(o))[:, None]
    nearest = crossings[rows, order]
    count = np.isfinite(nearest).sum(axis=1)
    return count, nearest[:, 0], nearest[:, 1], blocked, np.asarray(media)[rows, order][:, 0]


def _uniform_sphere(rng, n):
    z = 2.0 * rng.random(n) - 1.0
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = 2.0 * np.pi * rng.random(n)
    return np.stack([r * np.cos(phi), z, r * np.sin(phi)], axis=1)


def _cosine_hemisphere(rng, normal):
    """a cosine-distributed direction about `normal` (the Lambertian's sample: throughput * cos / pdf = rho)"""
    u = rng.random(len(normal))
    r, phi = np.sqrt(u), 2.0 * np.pi * rng.random(len(normal))
    helper = np.where(np.abs(normal[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    tangent = np.cross(normal, helper)
    tangent /= np.linalg.norm(tangent, axis=1, keepdims=True)
    bitangent = np.cross(normal, tangent)
    return tangent * (r * np.cos(phi))[:, None] + bitangent * (r * np.sin(phi))[:, None] + normal * np.sqrt(1.0 - u)[:, None]


def walk(scene, n, last_bounces, start_bounce=0, seed=1, stack_rule="stack"):
    """n walks.  Returns ({last bounce: per-walk values (n,)}, info) for the bounce windows (start_bounce, last) of
    `last_bounces`: one walk serves them all, since a window's last bounce only decides where the same path stops.
    info: "surface_counted" (see above) and "dropped" (walks that would have pushed a fifth medium: value 0, as a dropped sample)."""
    assert stack_rule in ("stack", "clear")
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
    value[~hit] = 1.0
    if start_bounce == 0:
        container = hit & ((surface == 0) | (scene.inner == "container"))
        count, t0, t1, blocked, medium0 = _events(scene, origin, direction, np.where(hit, np.inf, 0.0))
        # the volumetric closest query: the events in front of the nearest opaque surface, which is black (zero) if there
        sigma0 = scene.sigma[medium0]
        with np.errstate(invalid="ignore"):      # (inf - inf where there are no two events)
            through = np.where(count >= 2, np.exp(-sigma0 * (t1 - t0)), np.where(count == 1, np.exp(-sigma0 * t0), 1.0))
        value += np.where(container & ~blocked, through, 0.0)

    # ---- BasicVolumeIntegrator::L on the walks that hit something; state is kept for the live walks only
    alive = np.nonzero(hit)[0]
    position = origin[alive] + direction[alive] * t[alive][:, None]
    direction, surface, entering = direction[alive], surface[alive], entering[alive]
    weight = np.ones(len(alive))
    stack = np.full((len(alive), STACK_DEPTH), -1, dtype=np.int64)
    depth = np.zeros(len(alive), dtype=np.int64)
    on_surface = np.ones(len(alive), dtype=bool)      # interaction.isSurface
    crossing = np.zeros(len(alive), dtype=bool)       # the surface interaction changes sides (wo, wi on different sides)

    def at_surface(bounce, surface, entering, position, direction, weight):
        """a vertex on a surface: the BSDF sample.  Returns (new direction, crosses, weight after the NEXT segment is found)"""
        ball = (surface == 1) & (scene.inner == "lambertian")
        if ball.any():
            if any(counts(bounce, last) for last in last_bounces):
                info["surface_counted"] += int(ball.sum())
            normal = position[ball] / scene.inner_radius
            direction = direction.copy()
            direction[ball] = _cosine_hemisphere(rng, normal)
        return direction, ~ball, np.where(ball, scene.rho, 1.0)

    direction, crossing, pending = at_surface(1, surface, entering, position, direction, weight)
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
        if stack_rule == "clear":
            stack[push, 0], depth[push] = medium[push], 1
            depth[change & ~entering] = 0
        else:
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
        towards = _uniform_sphere(rng, len(rows))
        count, t0, t1, blocked, _ = _events(scene, position[rows], towards, np.full(len(rows), T_LIGHT))
        sigma_here = sigma[rows]
        with np.errstate(invalid="ignore"):
            shadow = np.where(count >= 2, np.exp(-sigma_here * (t1 - t0)), np.where(count == 1, np.exp(-sigma_here * t0), 0.0))
        value[alive[rows]] += np.where(blocked, 0.0, shadow) * weight[rows]      # not gated by the window
        direction[rows] = _uniform_sphere(rng, len(rows))

        # ... or the surface at the segment's end becomes the interaction
        on_surface = ~scatters
        stays = np.nonzero(on_surface)[0]
        new_direction, crosses, factor = at_surface(bounce, surface[stays], entering[stays], position[stays], direction[stays], weight[stays])
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


def mean_and_deviation(values):
    return float(values.mean()), float(values.std(ddof=1))
