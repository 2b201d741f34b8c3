"""Instanced geometry on the Python side: the description HipScene hands pathed_hip_scene_create_instanced, and
`flatten_instances`, the shared definition of "the same scene, flattened".

A scene with instances is a PathedSceneDesc whose last geoms are PROTOTYPES (meshes in their own space, not placed in the
world) plus a list of placements, each one prototype under an affine 3 x 4 transform (include/pathed_hip.h:
PathedInstanceDesc).  Primitive ids are virtual: world triangles [0, T0), then placement k's triangles in placement order.

The flatten routine is the one of the header, operation for operation in float32 (numpy rounds every operation once and
fuses nothing): the device applies the same statements to the prototype's shading record when a ray hits a placement, so
the flattened scene and the instanced scene shade a hit (t, u, v, prim) to the same floats.
"""
import ctypes as C

import numpy as np

from . import _capi


def _f32(value):
    return np.asarray(value, dtype=np.float32)


def instance_inverse(transform):
    """The inverse of a row-major 3 x 4 transform: cofactors in float64 from the float32 entries, rounded once to float32
    (pathed_amd/csrc/instances.h: instanceInverse, the same operations in the same order)."""
    m = _f32(transform).reshape(12).astype(np.float64)
    a, b, c, tx, d, e, f, ty, g, h, k, tz = (m[i] for i in range(12))
    c00, c01, c02 = e * k - f * h, c * h - b * k, b * f - c * e
    c10, c11, c12 = f * g - d * k, a * k - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = (a * c00 + b * c10) + c * c20
    if not (det != 0.0 and np.isfinite(det)):
        raise ValueError("instance transform is not invertible")
    r = [c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det]
    out = np.zeros(12, dtype=np.float32)
    for row in range(3):
        for col in range(3):
            out[4 * row + col] = np.float32(r[3 * row + col])
        out[4 * row + 3] = np.float32(-((r[3 * row] * tx + r[3 * row + 1] * ty) + r[3 * row + 2] * tz))
    return out


def _host_min(a, b):
    """std::min(a, b) as the C++ library states it: b where b < a, else a (a signed zero stays where the host leaves it)"""
    return np.where(b < a, b, a).astype(np.float32)


def _host_max(a, b):
    return np.where(a < b, b, a).astype(np.float32)


def pad_box(lo, hi):
    """bvh_build.h padBox in float32: every child box of a node is its content's box widened by 1e-5 max(1, |lo|, |hi|) per axis."""
    lo, hi = _f32(lo), _f32(hi)
    pad = np.float32(1e-5) * _host_max(np.float32(1.0), _host_max(np.abs(lo), np.abs(hi)))
    return (lo - pad).astype(np.float32), (hi + pad).astype(np.float32)


def prototype_box(positions):
    """The padded box of a prototype's corners ((n, 3) float32, object space): what its root's children span at most."""
    p = _f32(positions).reshape(-1, 3)
    return pad_box(p.min(axis=0), p.max(axis=0))


def placement_box(transform, proto_lo, proto_hi):
    """The world box of a placement as pathed_amd/csrc/instances.h states it (placementBox), float32, one rounding per operation: the
    eight corners of the prototype's padded box (prototype_box) through the flatten routine, min / max, then a pad of
    1e-5 max(1, |lo|, |hi|) + 1e-5 (hi - lo) per axis for the roundings of the object-space ray.  The node that holds the
    placement stores pad_box of this box, as it does of every child."""
    proto_lo, proto_hi = _f32(proto_lo).reshape(3), _f32(proto_hi).reshape(3)
    corners = np.array([[(proto_hi if corner & (1 << axis) else proto_lo)[axis] for axis in range(3)] for corner in range(8)], dtype=np.float32)
    world = flatten_points(transform, corners)
    lo, hi = np.full(3, np.inf, dtype=np.float32), np.full(3, -np.inf, dtype=np.float32)
    for point in world:
        lo, hi = _host_min(lo, point), _host_max(hi, point)
    reach = _host_max(np.float32(1.0), _host_max(np.abs(lo), np.abs(hi)))
    pad = (np.float32(1e-5) * reach + np.float32(1e-5) * (hi - lo)).astype(np.float32)
    return (lo - pad).astype(np.float32), (hi + pad).astype(np.float32)


DIM_TIME = 0xFFFFFFFF   # pathed_amd/csrc/sample_stream.h: kDimTime


def interpolate_transforms(a, b, t):
    """The placements' transforms at shutter time t (pathed_amd/csrc/instances.h: interpolateTransform), float32, one rounding per
    operation: m[i] = ((1 - t) * a[i]) + (t * b[i]).  `a` (time 0) and `b` (time 1) are (n, 12) or (12,) float32; t = 0 and t = 1
    give the bits of a and of b apart from the sign of a zero."""
    a, b, t = _f32(a), _f32(b), np.float32(t)
    s = np.float32(1.0) - t
    return ((s * a).astype(np.float32) + (t * b).astype(np.float32)).astype(np.float32)


def _mix32(x):
    """pathed_amd/csrc/sample_stream.h: mix32, on uint32 (numpy wraps modulo 2^32)"""
    x = np.asarray(x, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846ca68b)
        x = x ^ (x >> np.uint32(16))
    return x


def stream_value(seed, pixel, sample, dimension):
    """u(seed, pixel, sample, dimension) of the counter-based stream (sample_stream.h: makeKey, Rng::next), float32; pixel, sample
    and dimension may be arrays."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    pixel, sample, dimension = (np.asarray(v, dtype=np.uint32) for v in (pixel, sample, dimension))
    with np.errstate(over="ignore"):
        k0 = _mix32(pixel ^ _mix32(np.uint32(seed & 0xFFFFFFFF)))
        k1 = _mix32(sample ^ _mix32(np.uint32(seed >> 32) ^ np.uint32(0x9e3779b9)))
        bits = _mix32(k0 + _mix32(k1 + dimension * np.uint32(0x9e3779b9)))
    return ((bits >> np.uint32(8)).astype(np.float32) * np.float32(5.9604638e-08)).astype(np.float32)


def sample_time(seed, pixel, sample, open, close):
    """The shutter time of a sample (instances.h: sampleTime): t = open + (close - open) * u in float32, u the sample's stream at
    dimension DIM_TIME -- a pure function of (seed, pixel, sample)."""
    open, close = np.float32(open), np.float32(close)
    u = stream_value(seed, pixel, sample, DIM_TIME)
    return (open + ((close - open) * u).astype(np.float32)).astype(np.float32)


def moving_placement_box(a, b, open, close, proto_lo, proto_hi):
    """A moving placement's world box over the shutter (instances.h: movingPlacementBox, where the pad is derived): the union of
    placement_box at `open` and at `close`, widened per axis by the static pad over the union plus 1e-6 of
    sum_j max(|a_ij|, |b_ij|) max(|lo_j|, |hi_j|) + max(|a_i3|, |b_i3|) for the roundings of the interpolated matrix."""
    a, b = _f32(a).reshape(12), _f32(b).reshape(12)
    proto_lo, proto_hi = _f32(proto_lo).reshape(3), _f32(proto_hi).reshape(3)
    lo0, hi0 = placement_box(interpolate_transforms(a, b, open), proto_lo, proto_hi)
    lo1, hi1 = placement_box(interpolate_transforms(a, b, close), proto_lo, proto_hi)
    box_lo, box_hi = _host_min(lo0, lo1), _host_max(hi0, hi1)
    extent = _host_max(np.abs(proto_lo), np.abs(proto_hi))
    lo, hi = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    for i in range(3):
        reach = _host_max(np.abs(a[4 * i + 3]), np.abs(b[4 * i + 3]))
        for j in range(3):
            reach = np.float32(reach + np.float32(_host_max(np.abs(a[4 * i + j]), np.abs(b[4 * i + j])) * extent[j]))
        static = np.float32(np.float32(np.float32(1e-5) * _host_max(np.float32(1.0), _host_max(np.abs(box_lo[i]), np.abs(box_hi[i]))))
                            + np.float32(np.float32(1e-5) * np.float32(box_hi[i] - box_lo[i])))
        pad = np.float32(static + np.float32(np.float32(1e-6) * reach))
        lo[i], hi[i] = np.float32(box_lo[i] - pad), np.float32(box_hi[i] + pad)
    return lo, hi


def flatten_points(transform, points):
    """x' = ((m[0] x + m[1] y) + m[2] z) + m[3], ... in float32, for (n, 3) float32 points."""
    m = _f32(transform).reshape(12)
    p = _f32(points).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3)], axis=1).astype(np.float32)


def flatten_normals(inverse, normals):
    """n' = inverse-transpose times n, x' = ((i[0] x + i[4] y) + i[8] z), ... in float32; not renormalised."""
    i = _f32(inverse).reshape(12)
    n = _f32(normals).reshape(-1, 3)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    return np.stack([(i[c] * x + i[4 + c] * y) + i[8 + c] * z for c in range(3)], axis=1).astype(np.float32)


class InstanceSet:
    """Prototypes [(first_geom, n_geoms), ...] and placements [(prototype, 12 floats row-major 3 x 4), ...] as the
    PathedInstanceDesc of the C ABI; keeps its arrays alive."""

    def __init__(self, prototypes, instances):
        self.prototypes = [(int(first), int(count)) for first, count in prototypes]
        self.instances = [(int(prototype), _f32(transform).reshape(12).copy()) for prototype, transform in instances]
        self._prototype_array = (_capi.PathedPrototype * max(1, len(self.prototypes)))()
        for slot, (first, count) in zip(self._prototype_array, self.prototypes):
            slot.first_geom, slot.n_geoms = first, count
        self._instance_array = (_capi.PathedInstance * max(1, len(self.instances)))()
        for slot, (prototype, transform) in zip(self._instance_array, self.instances):
            slot.prototype = prototype
            slot.transform[:] = transform.tolist()
        self.desc = _capi.PathedInstanceDesc()
        self.desc.struct_size = C.sizeof(_capi.PathedInstanceDesc)
        self.desc.n_prototypes, self.desc.prototypes = len(self.prototypes), self._prototype_array
        self.desc.n_instances, self.desc.instances = len(self.instances), self._instance_array

    def set_transforms(self, transforms):
        """Replace every placement's transform ((n, 12) or (n, 3, 4) float32, instance order); the prototypes stay
        (HipScene.set_instance_transforms keeps the set in step with the device through this)."""
        transforms = _f32(transforms).reshape(-1, 12)
        if len(transforms) != len(self.instances):
            raise ValueError("%d transforms for %d placements" % (len(transforms), len(self.instances)))
        self.instances = [(prototype, row.copy()) for (prototype, _), row in zip(self.instances, transforms)]
        for slot, (_, transform) in zip(self._instance_array, self.instances):
            slot.transform[:] = transform.tolist()


class FlattenedScene:
    """What flatten_instances returns: `.desc` is a pointer to a flat PathedSceneDesc (it shares the camera, materials,
    textures and environment of the description it came from, which must outlive it); `.bases` the virtual-id base of every
    placement and, last, the triangle count."""

    def __init__(self):
        self.desc = None
        self.bases = None
        self._keep = []


def flatten_instances(desc_pointer, prototypes, instances):
    """The flat description of an instanced scene: the world's triangles, then every placement's triangles written out as
    world triangles by the flatten routine, in placement order -- the triangle at index i is the one the instanced scene
    reports as primitive i.  Each placement becomes one mesh geom after the world's geoms."""
    source = desc_pointer.contents
    instance_set = instances if isinstance(instances, InstanceSet) else InstanceSet(prototypes, instances)
    n_vertices, n_triangles = int(source.n_vertices), int(source.n_triangles)
    positions = np.ctypeslib.as_array(source.positions, shape=(n_vertices, 3)) if n_vertices else np.zeros((0, 3), np.float32)
    normals = np.ctypeslib.as_array(source.normals, shape=(n_vertices, 3)) if n_vertices else np.zeros((0, 3), np.float32)
    uvs = np.ctypeslib.as_array(source.uvs, shape=(n_vertices, 2)) if n_vertices else np.zeros((0, 2), np.float32)
    indices = np.ctypeslib.as_array(source.indices, shape=(n_triangles, 3)) if n_triangles else np.zeros((0, 3), np.uint32)
    tri_material = np.ctypeslib.as_array(source.tri_material, shape=(n_triangles,)) if n_triangles else np.zeros(0, np.int32)
    geoms = [source.geoms[g] for g in range(int(source.n_geoms))]

    first_prototype_geom = instance_set.prototypes[0][0] if instance_set.prototypes else len(geoms)
    world_triangles = geoms[first_prototype_geom].first if first_prototype_geom < len(geoms) else n_triangles
    ranges = []
    for first_geom, n_geoms in instance_set.prototypes:
        first = geoms[first_geom].first
        ranges.append((first, sum(geoms[first_geom + g].count for g in range(n_geoms))))

    out_positions, out_normals, out_uvs = [positions.copy()], [normals.copy()], [uvs.copy()]
    out_indices, out_materials = [indices[:world_triangles].copy()], [tri_material[:world_triangles].copy()]
    out_geoms = [_capi.PathedGeom(g.type, g.first, g.count, g.medium) for g in geoms[:first_prototype_geom]]
    vertex_base, triangle_base, bases = n_vertices, world_triangles, []
    for prototype, transform in instance_set.instances:
        first, count = ranges[prototype]
        triangles = indices[first:first + count].astype(np.int64)
        low, high = int(triangles.min()), int(triangles.max()) + 1
        inverse = instance_inverse(transform)
        out_positions.append(flatten_points(transform, positions[low:high]))
        out_normals.append(flatten_normals(inverse, normals[low:high]))
        out_uvs.append(uvs[low:high].copy())
        out_indices.append((triangles - low + vertex_base).astype(np.uint32))
        out_materials.append(tri_material[first:first + count].copy())
        out_geoms.append(_capi.PathedGeom(_capi.GEOM_MESH, triangle_base, count, -1))
        bases.append(triangle_base)
        vertex_base += high - low
        triangle_base += count
    bases.append(triangle_base)

    flat = FlattenedScene()
    flat.bases = np.asarray(bases, dtype=np.int64)
    desc = _capi.PathedSceneDesc()
    C.memmove(C.byref(desc), C.byref(source), C.sizeof(_capi.PathedSceneDesc))   # camera, materials, textures, environment, media
    arrays = {
        "positions": np.ascontiguousarray(np.concatenate(out_positions), dtype=np.float32),
        "normals": np.ascontiguousarray(np.concatenate(out_normals), dtype=np.float32),
        "uvs": np.ascontiguousarray(np.concatenate(out_uvs), dtype=np.float32),
        "indices": np.ascontiguousarray(np.concatenate(out_indices), dtype=np.uint32),
        "tri_material": np.ascontiguousarray(np.concatenate(out_materials), dtype=np.int32),
    }
    flat.positions, flat.indices = arrays["positions"], arrays["indices"]
    desc.n_vertices = len(arrays["positions"])
    desc.positions = arrays["positions"].ctypes.data_as(C.POINTER(C.c_float))
    desc.normals = arrays["normals"].ctypes.data_as(C.POINTER(C.c_float))
    desc.uvs = arrays["uvs"].ctypes.data_as(C.POINTER(C.c_float))
    desc.n_triangles = len(arrays["indices"])
    desc.indices = arrays["indices"].ctypes.data_as(C.POINTER(C.c_uint32))
    desc.tri_material = arrays["tri_material"].ctypes.data_as(C.POINTER(C.c_int32))
    geom_array = (_capi.PathedGeom * max(1, len(out_geoms)))(*out_geoms)
    desc.n_geoms, desc.geoms = len(out_geoms), geom_array
    flat._keep = [arrays, geom_array, desc, desc_pointer, instance_set]
    flat.desc = C.pointer(desc)
    return flat
