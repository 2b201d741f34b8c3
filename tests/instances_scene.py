"""The scenes and rays of the instancing tests (test_gpu_instances.py): a world floor and emitter, prototype P (a 320-triangle
sphere with vertex normals and uvs) and prototype Q (a 12-triangle box), both modelled away from the origin, under two sets
of placements, plus the float64 brute force the hits are judged against.  No test lives here."""
import numpy as np

from pathed_amd import _capi
from scene_builder import BuiltScene


def icosphere(center, radius, subdivisions=2):
    """(vertices, faces, normals, uvs) of a closed sphere mesh: 20 * 4^subdivisions triangles, outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    vertices = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
                (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    vertices = [np.asarray(v, dtype=np.float64) / np.linalg.norm(v) for v in vertices]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        cache, refined = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                point = vertices[a] + vertices[b]
                vertices.append(point / np.linalg.norm(point))
                cache[key] = len(vertices) - 1
            return cache[key]

        for a, b, c in faces:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            refined += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = refined
    unit = np.asarray(vertices)
    positions = (np.asarray(center, dtype=np.float64) + radius * unit).astype(np.float32)
    uvs = np.stack([0.5 + np.arctan2(unit[:, 2], unit[:, 0]) / (2 * np.pi), 0.5 + np.arcsin(np.clip(unit[:, 1], -1, 1)) / np.pi], axis=1)
    return positions, faces, unit.astype(np.float32), uvs.astype(np.float32)


def rotation(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    angle = np.radians(degrees)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def affine(linear=None, translation=(0, 0, 0)):
    """row-major 3 x 4, float32"""
    out = np.zeros((3, 4))
    out[:, :3] = np.eye(3) if linear is None else linear
    out[:, 3] = translation
    return out.astype(np.float32).reshape(12)


# prototype indices
P, Q = 0, 1

# uniform power-of-two scales, no translation: every transformed coordinate is an exact multiple of the prototype's
EXACT_PLACEMENTS = [(P, affine()), (Q, affine()), (P, affine(0.5 * np.eye(3))), (P, affine(2.0 * np.eye(3))),
                    (Q, affine(2.0 * np.eye(3))), (Q, affine(0.5 * np.eye(3)))]

P_CENTRE, Q_CENTRE = np.array([3.0, 2.0, 1.0]), np.array([-3.0, 1.0, 2.0])


def placed(linear, world_centre, prototype_centre):
    """the transform with this linear part that takes the prototype's centre to world_centre"""
    linear = np.asarray(linear, dtype=np.float64)
    return affine(linear, np.asarray(world_centre, dtype=np.float64) - linear @ prototype_centre)


# a rotation about a skew axis, a non-uniform scale, translations of a few units, a mirrored placement (det < 0) and one
# 1 000 units from the origin (large, so that it still covers its share of the image)
GENERAL_PLACEMENTS = [
    (P, placed(1.6 * rotation((1.0, 2.0, 0.5), 37.0), (-4.3, 1.8, 2.0), P_CENTRE)),
    (P, placed(np.diag([2.0, 1.3, 1.6]), (-1.4, 3.1, 1.0), P_CENTRE)),
    (Q, placed(2.6 * rotation((0.2, 1.0, 0.1), 25.0), (1.5, 1.4, 3.0), Q_CENTRE)),
    (P, placed(1.6 * np.diag([-1.0, 1.0, 1.0]) @ rotation((0.3, 0.1, 1.0), 20.0), (4.5, 3.6, 2.0), P_CENTRE)),
    (P, placed(150.0 * rotation((0.5, 1.0, 0.2), 70.0), (0.0, 300.0, -988.0), P_CENTRE)),
]
CAMERA = dict(origin=(0.0, 3.0, 12.0), target=(0.0, 3.0, 0.0), fov_degrees=50.0)


def build(placements, width, height, with_prototypes=True):
    """(BuiltScene, desc pointer, prototypes, instances): the description carries the prototypes as its last two geoms."""
    scene = BuiltScene(width, height, **CAMERA)
    floor = scene.material(diffuse=(0.6, 0.6, 0.55))
    light = scene.material(diffuse=(0.0, 0.0, 0.0), emit=(14.0, 13.0, 11.0))
    skin = scene.material(diffuse=(0.7, 0.35, 0.25))
    shell = scene.material(_capi.MAT_PLASTIC, diffuse=(0.25, 0.4, 0.7), alpha=0.2)
    scene.quad([(-14, 0, -14), (-14, 0, 14), (14, 0, 14), (14, 0, -14)], floor)
    scene.quad([(-3, 11, -3), (3, 11, -3), (3, 11, 3), (-3, 11, 3)], light)
    world_geoms = len(scene.geoms)
    if with_prototypes:
        positions, faces, normals, uvs = icosphere((3.0, 2.0, 1.0), 1.0)
        scene.mesh(positions, faces, skin, normals=normals, uvs=uvs)
        scene.box((-3.5, 0.5, 1.5), (-2.5, 1.5, 2.5), shell)
    pointer = scene.finish()
    prototypes = [(world_geoms, 1), (world_geoms + 1, 1)] if with_prototypes else []
    return scene, pointer, prototypes, list(placements)


def triangles_of(flat):
    """(n, 3, 3) float64 corners of a FlattenedScene's triangles, from its float32 vertices"""
    return flat.positions[flat.indices.astype(np.int64)].astype(np.float64)


def brute_force(triangles, rays, chunk=256):
    """float64 Moeller-Trumbore of every ray (n, 8 float32: o, tnear, d, tfar) against every triangle.  Per ray: nearest t, its
    primitive (-1: none), the smallest barycentric of that hit and the second-nearest t (inf: none)."""
    rays = np.asarray(rays, dtype=np.float64)
    v0, e1, e2 = triangles[:, 0], triangles[:, 1] - triangles[:, 0], triangles[:, 2] - triangles[:, 0]
    n = len(rays)
    nearest, prim, margin, second = np.full(n, np.inf), np.full(n, -1, dtype=np.int64), np.zeros(n), np.full(n, np.inf)
    for begin in range(0, n, chunk):
        block = rays[begin:begin + chunk]
        o, d = block[:, None, 0:3], block[:, None, 4:7]
        pvec = np.cross(d, e2[None])
        det = (e1[None] * pvec).sum(-1)
        ok = det != 0.0
        inv = 1.0 / np.where(ok, det, 1.0)
        tvec = o - v0[None]
        u = (tvec * pvec).sum(-1) * inv
        qvec = np.cross(tvec, e1[None])
        v = (d * qvec).sum(-1) * inv
        t = (e2[None] * qvec).sum(-1) * inv
        hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > block[:, None, 3]) & (t <= block[:, None, 7])
        t = np.where(hit, t, np.inf)
        order = np.argsort(t, axis=1)[:, :2]
        rows = np.arange(len(block))
        first = order[:, 0]
        nearest[begin:begin + chunk] = t[rows, first]
        second[begin:begin + chunk] = t[rows, order[:, 1]]
        found = np.isfinite(t[rows, first])
        prim[begin:begin + chunk] = np.where(found, first, -1)
        margin[begin:begin + chunk] = np.minimum(np.minimum(u[rows, first], v[rows, first]), 1.0 - u[rows, first] - v[rows, first])
    return nearest, prim, margin, second


def exact_rays(flat, count, seed):
    """Closest-hit and any-hit rays for the exact class: random origins, origins ON surfaces, targets inside triangles, on edge
    midpoints and on corners.  No coordinate is a negative zero (sums with +0.0)."""
    rng = np.random.default_rng(seed)
    triangles = triangles_of(flat)
    pick = rng.integers(0, len(triangles), count)
    kind = rng.integers(0, 4, count)
    bary = rng.dirichlet((1.0, 1.0, 1.0), count)
    bary[kind == 1] = np.array([0.5, 0.5, 0.0])       # an edge midpoint
    bary[kind == 2] = np.array([0.0, 0.0, 1.0])       # a corner
    target = (triangles[pick] * bary[:, :, None]).sum(1)
    origin = rng.uniform((-12, 0.2, -12), (12, 10, 14), (count, 3))
    on_surface = rng.random(count) < 0.25
    other = rng.integers(0, len(triangles), count)
    origin[on_surface] = (triangles[other[on_surface]] * rng.dirichlet((1.0, 1.0, 1.0), int(on_surface.sum()))[:, :, None]).sum(1)
    origin = origin.astype(np.float32)
    direction = (target.astype(np.float32) - origin) + np.float32(0.0)
    rays = np.zeros((count, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origin + np.float32(0.0), 1e-3, direction, 1e5
    shadow = rays.copy()
    shadow[:, 7] = np.where(rng.random(count) < 0.5, 1.0, 0.999).astype(np.float32)   # up to the target, or just short of it
    return rays, shadow


def general_rays(flat, count, seed):
    """Rays towards interior points of the flattened triangles from 2 .. 10 units away (the placements' own scale for the
    large one), t about 1."""
    rng = np.random.default_rng(seed)
    triangles = triangles_of(flat)
    # the world's triangles or one of the placements, equally often, then one of its triangles
    starts = np.concatenate([[0], flat.bases])
    group = rng.integers(0, len(starts) - 1, count)
    pick = (starts[group] + np.floor(rng.random(count) * (starts[group + 1] - starts[group]))).astype(np.int64)
    bary = rng.dirichlet((2.0, 2.0, 2.0), count)
    target = (triangles[pick] * bary[:, :, None]).sum(1)
    size = np.sqrt(np.linalg.norm(np.cross(triangles[pick, 1] - triangles[pick, 0], triangles[pick, 2] - triangles[pick, 0]), axis=1))
    heading = rng.normal(size=(count, 3))
    heading /= np.linalg.norm(heading, axis=1, keepdims=True)
    reach = rng.uniform(2.0, 10.0, count) * np.maximum(1.0, size / 0.3)
    origin = (target + heading * reach[:, None]).astype(np.float32)
    rays = np.zeros((count, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origin, 1e-3, target.astype(np.float32) - origin, 1e5
    return rays


def keep_mask(nearest, prim, margin, second):
    """The filter of the general class, on the float64 data alone: a hit, no barycentric below 0.02, the runner-up further than
    1e-4 relative."""
    return (prim >= 0) & (margin >= 0.02) & ~(second - nearest <= 1e-4 * nearest)


def camera_rays(width, height, origin, target, up=(0, 1, 0), fov_degrees=CAMERA["fov_degrees"]):
    """The pixel-centre camera rays (shading.h: cameraRay), row 0 = bottom: (height * width, 8) float32."""
    origin, target, up = (np.asarray(v, dtype=np.float64) for v in (origin, target, up))
    direction = (origin - target) / np.linalg.norm(origin - target)
    x_axis = np.cross(up / np.linalg.norm(up), direction)
    x_axis /= np.linalg.norm(x_axis)
    y_axis = np.cross(direction, x_axis)
    film_height = 2 * np.tan(np.radians(fov_degrees) / 2) * 0.01
    film_width = film_height * width / height
    rows, cols = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    local = np.stack([film_width * (cols + 0.5) / width - film_width / 2, film_height * (rows + 0.5) / height - film_height / 2,
                      np.full(rows.shape, -0.01)], axis=-1).reshape(-1, 3)
    local /= np.linalg.norm(local, axis=1, keepdims=True)
    world = local[:, 0:1] * x_axis + local[:, 1:2] * y_axis + local[:, 2:3] * direction
    rays = np.zeros((width * height, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origin, 1e-3, world, 1e5
    return rays
