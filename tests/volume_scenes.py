"""Scene constructors for tests/test_gpu_volume_queries.py (a plain module over scene_builder.BuiltScene, no fixtures).

Most scenes sit inside a large emissive room (`enclosure`, +-10) whose six walls emit six different colours: rendered with the
bounce window 0..0 a pixel is the first hit's emission plus, behind a container, emit(what is seen through it) x
rayTransmission -- so it encodes which primitive the volumetric closest-hit query found and which events it kept.

Quad items (pathed_amd/csrc/small_items.h: buildSmallItems) decide between the QUADS instantiations of k_path_volume in a small
scene: two coplanar triangles that share a diagonal pair into one item when they fill a parallelogram (to 5 %) whose
extent stays below about 9.5 units.  The room's walls and anything wider never pair.  Every scene built through `extras`
carries a one-unit patch nobody looks at: two triangles (one quad item) by default, and with `fans=True` a fan of four
around its centre, like every other face of less than room size -- a fan pairs nothing (the fitted parallelogram would
hold half of the second triangle, or is degenerate), so such a scene has no quad item at all.
tests/test_gpu_volume_queries.py checks both statements against buildSmallItems itself.
"""
import numpy as np

from pathed_amd import _capi
from scene_builder import BuiltScene

WALLS = ("-z", "+z", "-y", "+y", "-x", "+x")
WALL_EMIT = {"-z": (4.0, 1.0, 1.0), "+z": (1.0, 4.0, 1.0), "-y": (1.0, 1.0, 4.0), "+y": (4.0, 4.0, 1.0), "-x": (1.0, 4.0, 4.0), "+x": (4.0, 1.0, 4.0)}


def box_faces(lo, hi):
    """corner lists of the six faces in the order of WALLS, counter-clockwise seen from outside (BuiltScene.box's own)"""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]
    return [[v[i] for i in quad] for quad in quads]


def plane(built, corners, material, medium=-1, fans=False):
    """a planar parallelogram: two triangles (one quad item when it is small enough), or a fan of four around its centre"""
    if not fans:
        built.quad(corners, material, medium=medium)
        return
    c = np.asarray(corners, dtype=np.float64)
    built.mesh(list(c) + [c.mean(axis=0)], [(4, 0, 1), (4, 1, 2), (4, 2, 3), (4, 3, 0)], material, medium=medium)


def container_box(built, lo, hi, material, medium, fans=False):
    if not fans:
        built.box(lo, hi, material, medium=medium)
        return
    for corners in box_faces(lo, hi):
        plane(built, corners, material, medium=medium, fans=True)


def enclosure(built, half=10.0):
    """six emissive walls facing inwards, one colour each (WALL_EMIT); two triangles each in every variant: at 20 units they
    are too large to become quad items"""
    for name, corners in zip(WALLS, box_faces((-half, -half, -half), (half, half, half))):
        built.quad(corners[::-1], built.material(diffuse=(0, 0, 0), emit=WALL_EMIT[name]))


def extras(built, fans=False, oren=False, extra_materials=0):
    """the patch nobody looks at (one quad item, or with `fans` none); oren: the patch is Oren-Nayar (the scene leaves the
    Lambertian / glass / container set: TraitsAll); extra_materials: unused materials (more than 96 in all: the material table
    leaves LDS, and nothing pairs)"""
    if oren:
        patch = built.material(_capi.MAT_OREN_NAYAR, diffuse=(0.4, 0.5, 0.6), sigma=0.4)
    else:
        patch = built.material(diffuse=(0.4, 0.5, 0.6))
    plane(built, [(8.0, 9.5, 8.0), (9.0, 9.5, 8.0), (9.0, 9.5, 9.0), (8.0, 9.5, 9.0)], patch, fans=fans)
    for k in range(extra_materials):
        built.material(diffuse=(0.1 + 0.005 * k, 0.2, 0.3))
    return built


def passthrough(built):
    return built.material(type_=_capi.MAT_PASSTHROUGH)


def gas(built, sigma, scatter=None):
    scatter = sigma if scatter is None else scatter
    return built.medium((sigma, sigma, sigma), (scatter, scatter, scatter))


# ------------------------------------------------------------------------------------------------ the analytic cases

def sphere_case(sigma, radius, width=24, height=20, **variant):
    """camera at the centre of a spherical container: ONE event in front of the wall, the segment is o..t0 = radius"""
    built = BuiltScene(width, height, (0, 0, 0), (0, 0, -1), fov_degrees=40)
    enclosure(built)
    built.sphere((0.0, 0.0, 0.0), radius, passthrough(built), medium=gas(built, sigma))
    return extras(built, **variant)


def slab_case(sigma, depth, width=24, height=24, fov=6.0, **variant):
    """camera outside a slab normal to the view axis: TWO events, the segment is t0..t1 = depth / cos(theta)"""
    built = BuiltScene(width, height, (0, 0, 5), (0, 0, 0), fov_degrees=fov)
    fans = variant.get("fans", False)
    enclosure(built)
    container_box(built, (-2, -2, -depth / 2), (2, 2, depth / 2), passthrough(built), gas(built, sigma), fans=fans)
    return extras(built, **variant)


EMITTER_INSIDE = (2.0, 3.0, 5.0)


def emitter_in_slab_case(sigma, depth, front=1.0, width=24, height=24, fov=6.0, **variant):
    """an opaque emitter at depth / 3 inside the slab, the camera `front` before the slab: the slab's far face lies behind the
    final hit and is clipped, ONE event (the near face) remains"""
    built = BuiltScene(width, height, (0, 0, depth / 2 + front), (0, 0, 0), fov_degrees=fov)
    fans = variant.get("fans", False)
    enclosure(built)
    container_box(built, (-2, -2, -depth / 2), (2, 2, depth / 2), passthrough(built), gas(built, sigma), fans=fans)
    z = depth / 2 - depth / 3
    plane(built, [(-1.5, -1.5, z), (1.5, -1.5, z), (1.5, 1.5, z), (-1.5, 1.5, z)], built.material(diffuse=(0, 0, 0), emit=EMITTER_INSIDE), fans=fans)
    return extras(built, **variant)


def two_slabs_case(sigma_near, sigma_far, width=24, height=24, fov=6.0, **variant):
    """two disjoint slabs in a row, the FAR one declared first (lower primitive ids, medium 0): four events, the two nearest
    are the near slab's faces"""
    built = BuiltScene(width, height, (0, 0, 5), (0, 0, 0), fov_degrees=fov)
    fans = variant.get("fans", False)
    enclosure(built)
    far, near = gas(built, sigma_far), gas(built, sigma_near)
    material = passthrough(built)
    container_box(built, (-2, -2, -2), (2, 2, -1), material, far, fans=fans)
    container_box(built, (-2, -2, 1), (2, 2, 2), material, near, fans=fans)
    return extras(built, **variant)


# --------------------------------------------------------------------------------- GPU against oracle, window 0..0

def uv_sphere(centre, radius, stacks=18, scale=1.0):
    """(vertices float32, faces): 2 * stacks slices, 2 * slices * (stacks - 1) triangles (1 224 at 18), outward normals;
    `scale` shrinks the finished float32 vertices about the centre (what a refit of the container is given)"""
    slices = 2 * stacks
    vertices = [(0.0, 1.0, 0.0)]
    for i in range(1, stacks):
        theta = np.pi * i / stacks
        for j in range(slices):
            phi = 2.0 * np.pi * j / slices
            vertices.append((np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)))
    vertices.append((0.0, -1.0, 0.0))
    ring = lambda i, j: 1 + (i - 1) * slices + (j % slices)
    faces = []
    for j in range(slices):
        faces.append((0, ring(1, j + 1), ring(1, j)))
        faces.append((len(vertices) - 1, ring(stacks - 1, j), ring(stacks - 1, j + 1)))
    for i in range(1, stacks - 1):
        for j in range(slices):
            faces.append((ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)))
            faces.append((ring(i, j), ring(i + 1, j + 1), ring(i + 1, j)))
    centre = np.asarray(centre, dtype=np.float32)
    points = (centre + np.float32(radius) * np.asarray(vertices, dtype=np.float32)).astype(np.float32)
    points = (centre + np.float32(scale) * (points - centre)).astype(np.float32)
    return points, faces


def tessellated_scene(width=48, height=40):
    """a 1 224-triangle spherical container around a glass PathedSphere: the queries walk a real tree"""
    built = BuiltScene(width, height, (0.4, 0.3, 5), (0, 0, 0), fov_degrees=40)
    enclosure(built)
    vertices, faces = uv_sphere((0, 0, 0), 1.5)
    built.mesh(vertices, faces, passthrough(built), medium=gas(built, 0.9))
    built.sphere((0.2, 0.1, 0.0), 0.5, built.material(type_=_capi.MAT_GLASS, ior=1.5))
    return built


def nested_scene(camera_inside=False, width=48, height=40):
    """a dense box inside a thin one; camera_inside: the camera sits in the outer medium"""
    origin = (0.9, 0.8, 1.2) if camera_inside else (2.0, 1.5, 5.0)
    built = BuiltScene(width, height, origin, (0, 0, 0), fov_degrees=45)
    enclosure(built)
    material = passthrough(built)
    built.box((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), material, medium=gas(built, 0.5))
    built.box((-0.7, -0.7, -0.7), (0.7, 0.7, 0.7), material, medium=gas(built, 2.0))
    return built


def cut_scene(width=48, height=40):
    """a container cut by an opaque emissive wall that reaches beyond it on every side"""
    built = BuiltScene(width, height, (2.5, 1.0, 5.0), (0, 0, 0), fov_degrees=40)
    enclosure(built)
    built.box((-1, -1, -1), (1, 1, 1), passthrough(built), medium=gas(built, 1.2))
    built.quad([(0.2, -3, -3), (0.6, -3, 3), (0.6, 3, 3), (0.2, 3, -3)], built.material(diffuse=(0.3, 0.3, 0.3), emit=(0.5, 2.0, 3.5)))
    return built


def random_scene(seed, width=48, height=40):
    """2-4 random box or tetrahedron containers over 2 media, random Lambertian emitters; odd seeds add 50 small grey
    triangles, which takes the scene above 64 triangles and onto the tree walk (even seeds: the all-triangles intersector)"""
    rng = np.random.default_rng(seed)
    built = BuiltScene(width, height, (0.0, 0.5, 6.0), (0, 0, 0), fov_degrees=45)
    enclosure(built)
    media = [gas(built, float(rng.uniform(0.3, 3.0))) for _ in range(2)]
    material = passthrough(built)
    for _ in range(int(rng.integers(2, 5))):
        centre = rng.uniform(-2.0, 2.0, 3)
        medium = media[int(rng.integers(0, 2))]
        if rng.random() < 0.5:
            half = rng.uniform(0.3, 1.2, 3)
            built.box(tuple(centre - half), tuple(centre + half), material, medium=medium)
        else:
            points = centre + rng.normal(size=(4, 3)) * 0.9
            faces = []
            for a, b, c, d in ((0, 1, 2, 3), (0, 1, 3, 2), (0, 2, 3, 1), (1, 2, 3, 0)):
                outward = np.dot(np.cross(points[b] - points[a], points[c] - points[a]), points[d] - points[a]) < 0
                faces.append((a, b, c) if outward else (a, c, b))
            built.mesh(points, faces, material, medium=medium)
    for _ in range(int(rng.integers(3, 6))):
        centre = rng.uniform(-2.5, 2.5, 3)
        emitter = built.material(diffuse=rng.uniform(0.1, 0.8, 3), emit=rng.uniform(0.5, 6.0, 3))
        built.mesh(centre + rng.normal(size=(3, 3)) * 0.8, [(0, 1, 2)], emitter)
    if seed % 2:
        grey = built.material(diffuse=(0.5, 0.5, 0.5))
        for _ in range(50):
            built.mesh(rng.uniform(-3.0, 3.0, 3) + rng.normal(size=(3, 3)) * 0.3, [(0, 1, 2)], grey)
    return built


# ------------------------------------------------------------------------------------- full paths on a walked tree

def gas_room(sigma=1.0, scale=1.0, origin=(0, 1.2, 5), width=48, height=40, extra_materials=0):
    """the room of test_gpu_volume.py's _gas_scene with the 1 224-triangle spherical container (vertices shrunk by `scale`
    about its centre) and the glass sphere inside"""
    built = BuiltScene(width, height, origin, (0, 1, 0), fov_degrees=38)
    white = built.material(diffuse=(0.7, 0.7, 0.7))
    red = built.material(diffuse=(0.6, 0.1, 0.1))
    light = built.material(diffuse=(0, 0, 0), emit=(20, 20, 20))
    built.quad([(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)], white)
    built.quad([(-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)], red)
    built.quad([(-0.5, 2.9, -0.5), (0.5, 2.9, -0.5), (0.5, 2.9, 0.5), (-0.5, 2.9, 0.5)], light)
    vertices, faces = uv_sphere((0, 1.2, 0), 1.0, scale=scale)
    built.container_vertices = (len(built.positions), len(vertices))
    built.mesh(vertices, faces, passthrough(built), medium=gas(built, sigma))
    built.sphere((0, 1.0, 0), 0.4, built.material(type_=_capi.MAT_GLASS, ior=1.5))
    for k in range(extra_materials):   # unused: more than 96 in all take the material table out of LDS
        built.material(diffuse=(0.1 + 0.005 * k, 0.2, 0.3))
    return built


# ---------------------------------------------------------------------------------------------------------- ties

TIE_SIGMA = {"A": 0.2, "B": 2.0}


def tie_scene(order="AB", first_medium="A", filler=False, width=32, height=24):
    """two abutting boxes, A (z 0..2, the camera inside) and B (z -1.5..0), whose shared face has the same four corner
    coordinates in both: a ray meets the two containers there at one t.  order: which box is declared first (the lower
    primitive ids); first_medium: whose medium has index 0; filler: 60 further triangles behind the camera, so that the
    scene walks a tree and the three builders apply"""
    built = BuiltScene(width, height, (0.1, 0.05, 1.0), (0.1, 0.05, 0.0), fov_degrees=40)
    enclosure(built)
    media = {}
    for name in (first_medium, "B" if first_medium == "A" else "A"):
        media[name] = gas(built, TIE_SIGMA[name])
    material = passthrough(built)
    boxes = {"A": ((-1, -1, 0), (1, 1, 2)), "B": ((-1, -1, -1.5), (1, 1, 0))}
    for name in order:
        built.box(boxes[name][0], boxes[name][1], material, medium=media[name])
    if filler:
        grey = built.material(diffuse=(0.5, 0.5, 0.5))
        rng = np.random.default_rng(5)
        for _ in range(30):
            centre = rng.uniform(-6.0, 6.0, 3) * (1.0, 1.0, 0.0) + (0.0, 0.0, float(rng.uniform(5.0, 9.0)))
            built.quad([tuple(centre + corner) for corner in ((-0.3, -0.3, 0), (0.3, -0.3, 0), (0.3, 0.3, 0.1), (-0.3, 0.3, 0.1))], grey)
    return built
