"""Inputs of the grid-medium tests (a plain module, no fixtures): the three grids and their 4 096 random segments each for
the function pins (tests/test_gpu_grid_queries.py; checked against the yardstick alone in tests/test_grid_cases.py), and the
scenes of tests/test_gpu_grid_images.py, built in the emissive room of volume_scenes.py.

Everything a test hands to the device is rounded to float32 HERE, and the yardstick (grid_reference.GridReference, float64) is
given those rounded numbers: the two sides compute on the same inputs.
"""
import functools

import numpy as np

import volume_scenes as vs
from grid_reference import GridReference
from pathed_amd import _capi
from scene_builder import BuiltScene

N_SEGMENTS = 4096
CATEGORIES = ("both-outside", "one-inside", "both-inside", "axis-parallel", "through-edge", "through-corner", "in-face")
TARGET_KINDS = ("met", "just-met", "just-missed", "far-missed")
THIN = 0.02
JUST = 2e-3   # "just": the target exponent is this far (relative) from the exponent of the whole segment

# The largest relative difference of the float32 device functions against the float64 yardstick over the fixture cases and the
# 3 x 4 096 random segments, measured on an MI355X (tests/test_gpu_grid_queries.py prints both), and the bound: four times it,
# for libm and summation-order differences between boxes -- not for the code under test.
QUERY_MEASURED = 5.3887e-05
QUERY_BOUND = 4.0 * QUERY_MEASURED


def rotation(degrees_x=0.0, degrees_y=0.0, degrees_z=0.0, translate=(0.0, 0.0, 0.0)):
    """model_to_world = T Ry Rx Rz as a float64 4x4"""
    x, y, z = np.radians([degrees_x, degrees_y, degrees_z])
    rx = np.array([[1, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    rz = np.array([[np.cos(z), -np.sin(z), 0], [np.sin(z), np.cos(z), 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ rz
    m[:3, 3] = translate
    return m


class GridCase:
    """a grid as the device gets it (float32 everywhere) and its yardstick"""

    def __init__(self, data, bounds, model_to_world=None, albedo=1.0, scale=1.0):
        self.data = np.ascontiguousarray(data, dtype=np.float32)   # (cells_z, cells_y, cells_x)
        self.bounds = np.asarray(bounds, dtype=np.float32)
        model_to_world = np.eye(4) if model_to_world is None else np.asarray(model_to_world, dtype=np.float64)
        self.model_to_world = model_to_world.astype(np.float32)
        self.world_to_model = np.linalg.inv(model_to_world).astype(np.float32)
        self.albedo, self.scale = float(np.float32(albedo)), float(np.float32(scale))
        self.reference = GridReference(self.data, self.bounds, self.world_to_model, self.scale)

    @property
    def cells(self):
        return self.data.shape[::-1]

    def set_on(self, scene, medium_index):
        scene.set_grid_medium(medium_index, data=self.data, bounds=self.bounds, albedo=self.albedo, scale=self.scale,
                              world_to_model=self.world_to_model, model_to_world=self.model_to_world)


@functools.lru_cache(maxsize=None)
def query_grids():
    rng = np.random.default_rng(20)
    return {
        "2x2x2": GridCase(rng.uniform(0.3, 2.5, (2, 2, 2)), (0, 0, 0, 1, 1, 1)),
        # (moved, not turned: a segment "in a cell face" has to stay in it, to the bit, on its way into model space.  On an axis
        # the segment does not move along, the tracker never steps; one that leaves the plane by a rounding error steps once, at
        # a time that rounding decides, and the reference's midpoint rule over the two halves of a cell is another number than
        # over the whole cell -- in float64 as in float32.  Turned grids are pinned by the images.)
        "3x4x5": GridCase(rng.uniform(0.3, 2.5, (5, 4, 3)), (-1.0, -0.5, -2.0, 1.0, 1.5, 0.5), rotation(translate=(0.3, -0.55, 0.125)), scale=1.5),
        "20x5x20": GridCase(rng.uniform(0.3, 2.5, (20, 5, 20)), (-2.0, 0.0, -2.0, 2.0, 1.0, 2.0)),
    }


def _segments(case, rng, n):
    """n model-space segments and their category indices"""
    lo, hi = case.bounds[:3].astype(np.float64), case.bounds[3:].astype(np.float64)
    size = hi - lo
    cells = np.array(case.cells)
    cell = size / (cells - 1)
    margin = 0.45 * cell   # an unclipped walk that starts less than half a cell outside stays within the step bound

    def inside(count):
        return lo + size * rng.uniform(0.02, 0.98, (count, 3))

    def outside(count):
        """in the shell of half a cell around the box, beyond a random face"""
        points = lo - margin + (size + 2 * margin) * rng.uniform(0.0, 1.0, (count, 3))
        axis = rng.integers(0, 3, count)
        high = rng.random(count) < 0.5
        depth = rng.uniform(0.05, 1.0, count)
        rows = np.arange(count)
        points[rows, axis] = np.where(high, hi[axis] + depth * margin[axis], lo[axis] - depth * margin[axis])
        return points

    def lattice(count, interior_only=False):
        """random grid vertices, as model points"""
        index = np.stack([rng.integers(1 if (interior_only and c > 2) else 0, (c - 1) if (interior_only and c > 2) else c, count) for c in cells], axis=1)
        return lo + index * cell

    def through(points, count):
        """segments through `points` along random directions, ending inside the shell"""
        direction = rng.normal(size=(count, 3))
        direction /= np.linalg.norm(direction, axis=1)[:, None]
        reach = 0.5 * np.linalg.norm(size)
        a = points - direction * rng.uniform(0.1, 1.0, (count, 1)) * reach
        b = points + direction * rng.uniform(0.1, 1.0, (count, 1)) * reach
        return np.clip(a, lo - margin, hi + margin), np.clip(b, lo - margin, hi + margin)

    per = n // len(CATEGORIES)
    counts = [per] * len(CATEGORIES)
    counts[0] += n - per * len(CATEGORIES)
    starts, ends, kinds = [], [], []
    for k, (name, count) in enumerate(zip(CATEGORIES, counts)):
        if name == "both-outside":
            a, b = outside(count), outside(count)
        elif name == "one-inside":
            a, b = outside(count), inside(count)
            swap = rng.random(count) < 0.5
            a, b = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
        elif name == "both-inside":
            a, b = inside(count), inside(count)
        elif name == "axis-parallel":
            a = np.where(rng.random((count, 1)) < 0.5, outside(count), inside(count))
            b = a.copy()
            axis = rng.integers(0, 3, count)
            rows = np.arange(count)
            b[rows, axis] = (lo - margin + (size + 2 * margin) * rng.uniform(0.0, 1.0, (count, 3)))[rows, axis]
        elif name == "through-edge":
            points = lattice(count)   # a point of a grid line: a vertex moved along one axis
            axis = rng.integers(0, 3, count)
            rows = np.arange(count)
            points[rows, axis] = (lo + size * rng.uniform(0.0, 1.0, (count, 3)))[rows, axis]
            a, b = through(points, count)
        elif name == "through-corner":
            a, b = through(lattice(count), count)
        else:   # in-face: both ends in one grid plane (an interior one where the axis has any; the 2-cell axes have the box's own)
            a, b = inside(count), inside(count)
            plane = lattice(count, interior_only=True)
            axis = rng.integers(0, 3, count)
            rows = np.arange(count)
            a[rows, axis] = plane[rows, axis]
            b[rows, axis] = plane[rows, axis]
        starts.append(a)
        ends.append(b)
        kinds.append(np.full(count, k))
    return np.concatenate(starts), np.concatenate(ends), np.concatenate(kinds)


@functools.lru_cache(maxsize=None)
def query_inputs(name):
    """(a, b, target) float32 as handed to the device, (category, target kind) indices, and the yardstick's results on exactly
    those numbers: dict(transmittance, valid, distance, exponent, target_exponent, hit_bound)"""
    case = query_grids()[name]
    rng = np.random.default_rng(sum(case.cells))
    a_model, b_model, category = _segments(case, rng, N_SEGMENTS)
    m = case.model_to_world.astype(np.float64)
    a = (a_model @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
    b = (b_model @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
    reference = case.reference
    # the exponent of the whole walk decides what "met" means for each segment
    _, _, whole, _, _ = reference.find_transmittance(a, b, np.full(N_SEGMENTS, 0.5))
    kind = rng.integers(0, len(TARGET_KINDS), N_SEGMENTS)
    factor = np.choose(kind, [rng.uniform(0.05, 0.95, N_SEGMENTS), np.full(N_SEGMENTS, 1.0 - JUST), np.full(N_SEGMENTS, 1.0 + JUST),
                              rng.uniform(1.5, 3.0, N_SEGMENTS)])
    # a segment that meets next to no medium (exponent below THIN) gets the target 1/2, far missed: next to 1 a float32 target
    # cannot say "just"
    thin = ~(whole >= THIN)
    kind = np.where(thin, TARGET_KINDS.index("far-missed"), kind)
    target = np.where(thin, 0.5, np.exp(-factor * whole)).astype(np.float32)
    transmittance, _, bound_t = reference.transmittance(a, b)
    valid, distance, exponent, target_exponent, bound_f = reference.find_transmittance(a, b, target)
    expected = dict(transmittance=transmittance, valid=valid, distance=distance, exponent=exponent, target_exponent=target_exponent,
                    hit_bound=bound_t | bound_f)
    return (a, b, target), (category, kind), expected


def ambiguous(expected, bound):
    """where float32 may decide validity either way: the accumulated exponent of the whole walk lies within `bound` (relative)
    of the target's"""
    with np.errstate(all="ignore"):
        return np.abs(expected["exponent"] - expected["target_exponent"]) <= bound * np.abs(expected["target_exponent"])


# --------------------------------------------------------------------------------------------------- image scenes

IMAGE_SIZE = (32, 24)


def _room(origin, target, fov):
    built = BuiltScene(IMAGE_SIZE[0], IMAGE_SIZE[1], origin, target, fov_degrees=fov)
    vs.enclosure(built)
    return built


@functools.lru_cache(maxsize=None)
def image_grid():
    rng = np.random.default_rng(345)
    return rng.uniform(0.2, 1.6, (5, 4, 3))


def image_scene(name):
    """(BuiltScene, {medium slot: GridCase}, containers) for the window-0..0 pins.  containers: [(lo, hi, medium slot)] of
    the axis-aligned container boxes, in declaration order; homogeneous media are ('sigma', value) in the dict"""
    if name == "outside":
        built = _room((0.3, 0.2, 5.0), (0.0, 0.0, 0.0), 22.0)
        lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
        slot = vs.gas(built, 0.0)
        built.box(lo, hi, vs.passthrough(built), medium=slot)
        return built, {slot: GridCase(image_grid(), lo + hi, albedo=0.8)}, [(lo, hi, slot)]
    if name == "inside":
        built = _room((0.2, 0.1, 0.3), (-0.4, 0.3, -2.0), 60.0)
        lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
        slot = vs.gas(built, 0.0)
        built.box(lo, hi, vs.passthrough(built), medium=slot)
        return built, {slot: GridCase(image_grid(), lo + hi, albedo=0.8)}, [(lo, hi, slot)]
    if name == "transformed":
        # the grid's box (model space) is smaller than the container and sits in it turned and shifted
        built = _room((0.3, 0.2, 5.0), (0.0, 0.0, 0.0), 28.0)
        lo, hi = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)
        slot = vs.gas(built, 0.0)
        built.box(lo, hi, vs.passthrough(built), medium=slot)
        grid = GridCase(image_grid(), (-0.75, -0.5, -0.625, 0.5, 0.75, 0.625), rotation(25.0, 35.0, 15.0, (0.125, -0.25, 0.0625)), scale=2.0)
        return built, {slot: grid}, [(lo, hi, slot)]
    if name == "behind-slab":
        # four events on a ray: the two nearest are the homogeneous slab's faces, the grid behind it contributes nothing
        built = _room((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), 14.0)
        material = vs.passthrough(built)
        grid_slot = vs.gas(built, 0.0)
        slab_slot = vs.gas(built, 0.9)
        grid_box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
        slab_box = ((-2.0, -2.0, 2.0), (2.0, 2.0, 2.5))
        built.box(grid_box[0], grid_box[1], material, medium=grid_slot)
        built.box(slab_box[0], slab_box[1], material, medium=slab_slot)
        return (built, {grid_slot: GridCase(image_grid(), grid_box[0] + grid_box[1]), slab_slot: ("sigma", 0.9)},
                [(grid_box[0], grid_box[1], grid_slot), (slab_box[0], slab_box[1], slab_slot)])
    raise KeyError(name)


IMAGE_SCENES = ("outside", "inside", "transformed", "behind-slab")


def _box_crossings(origin, direction, lo, hi):
    """distances t > 1e-3 at which the ray crosses the surface of the axis-aligned box, float64 (0, 1 or 2 of them)"""
    with np.errstate(all="ignore"):
        near = (np.asarray(lo) - origin) / direction
        far = (np.asarray(hi) - origin) / direction
    t0 = np.nanmax(np.minimum(near, far))
    t1 = np.nanmin(np.maximum(near, far))
    if not t0 < t1:
        return []
    return [t for t in (t0, t1) if t > 1e-3]


def expected_window0(name, seed, spp):
    """The float64 image (sums over spp samples) of window 0..0: SampleIntegrator::samplePixel, src/sample_integrator.cpp:10-51,
    along the ORACLE's camera rays (oracle_eval camera_ray with the oracle's jitter), the room and the container boxes
    intersected analytically, rayTransmission (src/volume_helper.cpp:71-123, medium = none) over the yardstick's
    transmittance.  Also returns the shortest chord t1 - t0 any ray cut from a container (how close a ray came to a silhouette;
    the image is continuous there: a vanishing chord transmits everything, like a miss)."""
    import oracle_lib
    built, media, containers = image_scene(name)
    width, height = IMAGE_SIZE
    camera = built.desc.camera
    head = list(camera.origin) + list(camera.target) + list(camera.up) + [camera.vertical_fov, width, height, camera.flip_handedness]
    image = np.zeros((height, width, 3))
    closest_silhouette = np.inf
    rays = []
    for row in range(height):
        for col in range(width):
            for sample in range(spp):
                pixel = row * width + col
                jitter_x = np.float32(oracle_lib.rng(seed, pixel, sample, 0)) - np.float32(0.5)
                jitter_y = np.float32(oracle_lib.rng(seed, pixel, sample, 1)) - np.float32(0.5)
                out = oracle_lib.evaluate("camera_ray", head + [np.float32(row + jitter_y), np.float32(col + jitter_x)], 6)
                rays.append((row, col, np.asarray(out[:3], dtype=np.float64), np.asarray(out[3:6], dtype=np.float64)))
    for row, col, origin, direction in rays:
        # the room: the wall the ray leaves through
        with np.errstate(all="ignore"):
            exits = np.where(direction > 0, (10.0 - origin) / direction, (-10.0 - origin) / direction)
        axis = int(np.argmin(exits))
        wall = ("-x", "+x", "-y", "+y", "-z", "+z")[2 * axis + (1 if direction[axis] > 0 else 0)]
        emit = np.asarray(vs.WALL_EMIT[wall], dtype=np.float64)
        events = []
        for lo, hi, slot in containers:
            crossings = _box_crossings(origin, direction, lo, hi)
            if len(crossings) == 2:
                closest_silhouette = min(closest_silhouette, crossings[1] - crossings[0])
            events += [(t, slot) for t in crossings]
        events.sort()
        if not events:
            image[row, col] += emit   # the wall is the first hit
            continue
        # the first hit is a container (emits nothing); what is seen through it, times rayTransmission(medium = none)
        if len(events) >= 2:
            start, end, slot = origin + direction * events[0][0], origin + direction * events[1][0], events[0][1]
        else:
            start, end, slot = origin, origin + direction * events[0][0], events[0][1]
        medium = media[slot]
        if isinstance(medium, tuple):
            transmittance = np.exp(-medium[1] * np.linalg.norm(end - start))
        else:
            # the kernel forms the two points in float32 (o + d * t); the yardstick takes them as the float64 they round from
            transmittance = float(medium.reference.transmittance([start], [end])[0][0])
        image[row, col] += emit * transmittance
    return image, closest_silhouette
