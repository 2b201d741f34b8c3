"""Record arrays for the device hook onto the shading functions (pathed_hip_debug_shading_queries) and for the oracle's
function-level interface: the same fp32 arrays feed both (layouts: tests/golden/README.md).  Deterministic, no GPU.

Checked against the oracle alone in tests/test_shading_cases.py (every branch named below is taken); against the device in
tests/test_gpu_shading_queries.py.

material(20) = type, albedo type, diffuse(3), emit(3), checker on(3), off(3), res(2), sigma, alpha, ior, distribution
isect(11)    = geometric normal(3), shading normal(3), wo(3), uv(2)
"""
import functools

import numpy as np

import oracle_lib

F32 = np.float32
LAMBERTIAN, OREN_NAYAR, MICROFACET, PLASTIC, GLASS, MIRROR = range(6)
BECKMANN, GGX = 0, 1
ALPHAS = (1e-3, 0.01, 0.05, 0.3, 1.0, 2.0)
SIGMAS = (0.0, 0.3, 1.5)
IORS = (1.0, 1.0001, 1.4, 2.4)
TINY = float(F32(2.0 ** -24))
ALMOST_ONE = float(F32(1.0 - 2.0 ** -24))


def below(x, steps=1):
    x = F32(x)
    for _ in range(steps):
        x = np.nextafter(x, F32(-np.inf))
    return float(x)


def above(x, steps=1):
    x = F32(x)
    for _ in range(steps):
        x = np.nextafter(x, F32(np.inf))
    return float(x)


def around(x):
    return [below(x), float(F32(x)), above(x)]


U_EDGES = [0.0, TINY, ALMOST_ONE]
U_HALF = around(0.5)

# what each instantiation of the kernels' compile-time scene sets contains (pathed_amd/csrc/shading.h: SceneTraits typedefs)
TRAITS = {
    "All": dict(materials=0x7F, env=True, spheres=True, varying=True, paired=False, dists=3),
    "LambertianTriangles": dict(materials=1, env=False, spheres=False, varying=False, paired=True, dists=3),
    "LambertianPlasticSpheres": dict(materials=1 | 8, env=False, spheres=True, varying=False, paired=True, dists=3),
    "LambertianGlassContainer": dict(materials=1 | 16 | 64, env=False, spheres=True, varying=False, paired=False, dists=3),
    "TriangleLit": dict(materials=0x3F, env=False, spheres=False, varying=False, paired=True, dists=3),
    "EnvironmentOnly": dict(materials=0x3F, env=True, spheres=False, varying=True, paired=False, dists=3),
    "RoughBeckmann": dict(materials=0x0F, env=False, spheres=False, varying=False, paired=True, dists=1),
    "RoughGgx": dict(materials=0x0F, env=False, spheres=False, varying=False, paired=True, dists=2),
    "Smooth": dict(materials=1 | 16 | 32, env=False, spheres=False, varying=False, paired=True, dists=3),
}


def accepts(traits, records):
    """mask over material records: those whose material kind, albedo kind and distribution the set `traits` contains"""
    t = TRAITS[traits]
    records = np.asarray(records)
    kind = records[:, 0].astype(int)
    ok = ((t["materials"] >> kind) & 1) == 1
    ok &= (records[:, 1] == 0) | t["varying"]
    facets = (kind == MICROFACET) | (kind == PLASTIC)
    ok &= ~facets | (((t["dists"] >> records[:, 19].astype(int)) & 1) == 1)
    return ok


# ------------------------------------------------------------------------------------------------------------ materials

def material(kind, albedo=0, diffuse=(0.6, 0.5, 0.4), checker=((0.9, 0.8, 0.1), (0.1, 0.2, 0.3), (4.0, 3.0)), sigma=0.0, alpha=0.1, ior=1.4,
             distribution=BECKMANN):
    return [kind, albedo, *diffuse, 0, 0, 0, *checker[0], *checker[1], *checker[2], sigma, alpha, ior, distribution]


def materials():
    """(label, material(20)) for every parameter the issue lists"""
    out = [("lambertian", material(LAMBERTIAN)), ("checkerboard", material(LAMBERTIAN, albedo=1))]
    out += [("oren-nayar sigma %g" % sigma, material(OREN_NAYAR, sigma=sigma)) for sigma in SIGMAS]
    for kind, name in ((MICROFACET, "microfacet"), (PLASTIC, "plastic")):
        for distribution, dname in ((BECKMANN, "beckmann"), (GGX, "ggx")):
            out += [("%s %s alpha %g" % (name, dname, alpha), material(kind, alpha=alpha, distribution=distribution)) for alpha in ALPHAS]
    out += [("glass ior %g" % ior, material(GLASS, ior=ior)) for ior in IORS]
    out.append(("mirror", material(MIRROR)))
    return out


UP = (0.0, 1.0, 0.0)
_generic = np.array([0.3, 0.8, -0.52], dtype=np.float64)
GENERIC_NORMAL = tuple(float(x) for x in (_generic / np.linalg.norm(_generic)).astype(F32))
_tilted = np.array([0.25, 0.95, 0.1], dtype=np.float64)
TILTED_SHADING = tuple(float(x) for x in (_tilted / np.linalg.norm(_tilted)).astype(F32))


def _with_cosine(cosine):
    """a unit vector in the xy plane at the cosine to UP (fp32; the y component is the cosine exactly)"""
    return (float(F32(np.sqrt(1.0 - float(cosine) ** 2))), float(cosine), 0.0)


def _frame(normal, wo):
    """normalToWorldSpace(normal, wo) in float64: the columns xAxis, normal, zAxis"""
    normal, wo = np.asarray(normal, np.float64), np.asarray(wo, np.float64)
    if np.array_equal(normal, wo):
        if abs(normal[0]) > abs(normal[1]):
            x = np.array([-normal[2], 0.0, normal[0]])
        else:
            x = np.array([0.0, -normal[2], normal[1]])
        x /= np.linalg.norm(x)
        return x, normal, np.cross(normal, x)
    x = np.cross(normal, wo)
    if not np.linalg.norm(x) > 0:
        x = np.array([1.0, 0.0, 0.0])
    x /= np.linalg.norm(x)
    z = np.cross(normal, x)
    return x, normal, z / np.linalg.norm(z)


def to_world(normal, wo, local):
    x, n, z = _frame(normal, wo)
    world = x * local[0] + n * local[1] + z * local[2]
    return tuple(float(v) for v in world.astype(F32))


def to_local(normal, wo, world):
    """normalized(toLocal(frame, world)) in float64 (what the lobes see), for the coverage checks"""
    x, n, z = _frame(normal, wo)
    world = np.asarray(world, np.float64)
    local = np.array([x @ world, n @ world, z @ world])
    length = np.linalg.norm(local)
    return local / length if length > 0 else local


def surfaces():
    """(label, geometric normal, shading normal, wo): the incidences of the issue's list"""
    out = [
        ("wo along the normal", UP, UP, UP),
        ("cos 0.7", UP, UP, _with_cosine(F32(0.7))),
        ("cos 1e-3", UP, UP, _with_cosine(F32(1e-3))),
        ("cos 1e-6", UP, UP, _with_cosine(F32(1e-6))),
        ("cos 0", UP, UP, (1.0, 0.0, 0.0)),
        ("wo below the surface", UP, UP, _with_cosine(F32(-0.8))),
        ("tilted shading normal", UP, TILTED_SHADING, _with_cosine(F32(0.6))),
        ("wo below the tilted shading normal only", UP, TILTED_SHADING, (-0.9987523, 0.049937617, 0.0)),
        ("generic normal", GENERIC_NORMAL, GENERIC_NORMAL, to_world(GENERIC_NORMAL, (0.0, 0.0, 1.0), (0.48, 0.6, 0.64))),
        ("wo along a generic normal", GENERIC_NORMAL, GENERIC_NORMAL, GENERIC_NORMAL),
    ]
    return out


CLAMP = float(F32(0.9999))   # TangentFrame::clamp's threshold


def _unit_with(component, value, azimuth=0.3):
    """a unit vector (float64) whose `component` is `value`, the rest split by `azimuth`"""
    rest = np.sqrt(max(0.0, 1.0 - value * value))
    others = [rest * np.cos(azimuth), rest * np.sin(azimuth)]
    vector = [0.0, 0.0, 0.0]
    vector[component] = value
    for k in range(3):
        if k != component:
            vector[k] = others.pop(0)
    return np.array(vector)


def incident_directions(normal, shading, wo, clamp_edges=True):
    """(label, wi world) at one surface: mirror direction (wh at the pole), -wo (zero half vector), below the horizon, generic
    ones, and directions whose local wi -- or whose half vector with wo -- has one component on either side of 0.9999"""
    wo64 = np.asarray(wo, np.float64)
    local_wo = to_local(shading, wo, wo)
    out = [("mirror", to_world(shading, wo, (-local_wo[0], local_wo[1], -local_wo[2]))),
           ("minus wo", tuple(float(-v) for v in wo)),
           ("below the horizon", to_world(shading, wo, (0.5, -0.3, 0.81))),
           ("generic a", to_world(shading, wo, (0.36, 0.8, 0.48))),
           ("generic b", to_world(shading, wo, (-0.6, 0.35, -0.72))),
           ("grazing", to_world(shading, wo, (0.8, 1e-4, 0.6)))]
    for component, name in enumerate("xyz") if clamp_edges else ():
        for sign in (1.0, -1.0) if name != "y" else (1.0,):
            for value in (below(CLAMP, 3), above(CLAMP, 3)):
                # wi itself across the threshold (beckmannLambda / ggxG1 see wi)
                out.append(("wi.%s %+.8f" % (name, sign * value), to_world(shading, wo, _unit_with(component, sign * value))))
                # the half vector across it: wi = reflect(wo, wh) for that wh
                wh = _unit_with(component, sign * value)
                wi = 2.0 * (local_wo @ wh) * wh - local_wo
                out.append(("wh.%s %+.8f" % (name, sign * value), to_world(shading, wo, wi)))
    return out


UVS = [(0.3, 0.7), (0.25, 1.0 / 3.0), (0.5, 0.5), (-0.1, 0.2), (-0.25, -1.0 / 3.0), (0.0, 0.0), (0.9999999, 2.0)]


@functools.lru_cache(maxsize=None)
def material_f_cases():
    """(records (n, 34) float32, labels): every material x every surface x every incident direction"""
    records, labels = [], []
    for mlabel, m in materials():
        for slabel, normal, shading, wo in surfaces():
            edges = slabel in ("cos 0.7", "tilted shading normal", "generic normal")
            for k, (wlabel, wi) in enumerate(incident_directions(normal, shading, wo, clamp_edges=edges)):
                uv = UVS[k % len(UVS)]
                records.append(m + list(normal) + list(shading) + list(wo) + list(uv) + list(wi))
                labels.append("%s | %s | %s" % (mlabel, slabel, wlabel))
    return np.asarray(records, dtype=F32), labels


def fresnel_of(cosine, eta_i, eta_t):
    return float(oracle_lib.evaluate("fresnel", [cosine, eta_i, eta_t])[0])


def critical_cosines(ior):
    """cosines of wo INSIDE glass at the critical angle: the two largest fp32 values at which the oracle's reflectance is 1
    (total reflection) and the two next floats, which refract -- found by bisection over the floats"""
    ior = float(F32(ior))
    total = lambda bits: fresnel_of(float(np.array(bits, dtype=np.uint32).view(F32)), ior, 1.0) == 1.0
    low, high = int(F32(0).view(np.uint32)), int(F32(1).view(np.uint32))   # positive floats order as their bit patterns
    assert total(low) and not total(high)
    while high - low > 1:
        middle = (low + high) // 2
        low, high = (middle, high) if total(middle) else (low, middle)
    return [float(np.array(bits, dtype=np.uint32).view(F32)) for bits in (low - 1, low, high, high + 1)]


@functools.lru_cache(maxsize=None)
def material_sample_cases():
    """(records (n, 34) float32, labels): materials x surfaces x scripted u"""
    pairs = [(a, b) for a in U_EDGES + [0.37] for b in U_EDGES + [0.61]]
    plastic_pairs = [(0.0, 0.0), (ALMOST_ONE, 0.37), (0.37, ALMOST_ONE), (TINY, 0.0), (0.83, 0.29)]
    records, labels = [], []
    for mlabel, m in materials():
        kind = m[0]
        for slabel, normal, shading, wo in surfaces():
            if slabel in ("wo below the tilted shading normal only", "wo along a generic normal"):
                continue
            if kind == PLASTIC:
                scripts = [(u0, u1, u2) for u0 in U_HALF + [0.0, ALMOST_ONE] for u1, u2 in plastic_pairs]
            elif kind == GLASS:
                local_y = float(F32(F32(F32(F32(shading[0]) * F32(wo[0])) + F32(F32(shading[1]) * F32(wo[1]))) + F32(F32(shading[2]) * F32(wo[2]))))
                eta_i, eta_t = (1.0, m[18]) if not local_y < 0 else (m[18], 1.0)
                reflectance = fresnel_of(abs(local_y), eta_i, eta_t)
                scripts = [(u, 0.5, 0.5) for u in U_EDGES + [0.5] + (around(reflectance) if 0.0 < reflectance < 1.0 else [])]
            elif kind == MIRROR:
                scripts = [(0.5, 0.5, 0.5)]
            else:
                scripts = [(u0, u1, 0.5) for u0, u1 in pairs]
            for k, script in enumerate(scripts):
                uv = UVS[k % len(UVS)]
                records.append(m + list(normal) + list(shading) + list(wo) + list(uv) + list(script))
                labels.append("%s | %s | u %r" % (mlabel, slabel, script))
        if kind == GLASS and m[18] > 1.0:
            # seen from inside, around the critical angle
            for cosine in critical_cosines(m[18]):
                wo = _with_cosine(F32(-cosine))
                reflectance = fresnel_of(cosine, m[18], 1.0)
                for u in [0.0, ALMOST_ONE] + (around(reflectance) if 0.0 < reflectance < 1.0 else []):
                    records.append(m + list(UP) + list(UP) + list(wo) + [0.0, 0.0] + [u, 0.5, 0.5])
                    labels.append("%s | inside, cos %.9g | u %r" % (mlabel, cosine, u))
    return np.asarray(records, dtype=F32), labels


@functools.lru_cache(maxsize=None)
def fresnel_cases():
    records = []
    for ior in IORS:
        for cosine in [0.0, 1e-6, 1e-3, 0.3, 0.7, below(1.0), 1.0]:
            records += [[cosine, 1.0, ior], [cosine, ior, 1.0], [cosine, 1.0, 1.5]]
        if ior > 1.0:
            records += [[cosine, ior, 1.0] for cosine in critical_cosines(ior)]
    return np.asarray(records, dtype=F32)


# -------------------------------------------------------------------------------------------------------------- spheres

SPHERE_CENTRE = (0.5, -1.0, 2.0)
SPHERE_RADIUS = 0.75
SPHERE_DISTANCES = [("inside", 0.3), ("at r", 1.0), ("r (1 + 1e-6)", 1.0 + 1e-6), ("1.15 r", 1.15), ("1e4 r", 1e4)]


@functools.lru_cache(maxsize=None)
def sphere_cases():
    """(sample records (n, 9), pdf records (m, 7), labels of the sample records)"""
    centre = np.asarray(SPHERE_CENTRE, np.float64)
    directions = [np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([0.48, -0.6, 0.64]), np.array([-0.7, 0.1, -0.7071])]
    pairs = [(a, b) for a in U_EDGES + U_HALF + [0.37] for b in U_EDGES + [0.61]]
    samples, pdfs, labels = [], [], []
    for dlabel, factor in SPHERE_DISTANCES:
        for direction in directions:
            reference = centre + direction / np.linalg.norm(direction) * (SPHERE_RADIUS * factor)
            pdfs.append(list(SPHERE_CENTRE) + [SPHERE_RADIUS] + list(reference))
            for pair in pairs:
                samples.append(list(SPHERE_CENTRE) + [SPHERE_RADIUS] + list(reference) + list(pair))
                labels.append("%s | u %r" % (dlabel, pair))
    return np.asarray(samples, dtype=F32), np.asarray(pdfs, dtype=F32), labels


# ---------------------------------------------------------------------------------------------------- environment maps

def _rotation():
    """a rotation that is no axis permutation, rounded to fp32, and its transpose"""
    a, b = 0.7, -0.4
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (ry @ rx).astype(F32)


@functools.lru_cache(maxsize=None)
def environment_maps():
    """{name: (rgba (H, W, 4) float32, scale, map_to_world 3x3 float32 or None)}"""
    rng = np.random.default_rng(20240607)

    def rgba(rgb):
        rgb = np.asarray(rgb, dtype=F32)
        return np.ascontiguousarray(np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), dtype=F32)], axis=2))

    maps = {}
    maps["ones 4x2"] = (rgba(np.ones((2, 4, 3))), 1.0, None)
    bright = np.full((5, 7, 3), 0.01)
    bright[3, 4] = (400.0, 300.0, 500.0)
    maps["one bright texel 7x5"] = (rgba(bright), 1.0, None)
    sparse = rng.uniform(0.05, 4.0, size=(33, 64, 3))
    sparse[rng.uniform(size=(33, 64)) < 0.9] = 0.0
    sparse[0] = 0.0            # a black row 0: an empty phi distribution that xi == 0 reaches
    sparse[17] = 0.0           # ... and one in the middle: a flat stretch of the theta CDF
    sparse[:, :9] = 0.0        # black leading columns
    sparse[5, 9:40] = 0.0      # a long flat stretch inside a row
    sparse[5, 40] = (1.0, 2.0, 0.5)
    maps["sparse 64x33"] = (rgba(sparse), 0.5, None)
    maps["range 16x8"] = (rgba(10.0 ** rng.uniform(-8, 3, size=(8, 16, 3))), 1.0, None)
    maps["single texel"] = (rgba(np.full((1, 1, 3), 0.7)), 2.0, None)
    maps["width one 1x6"] = (rgba(rng.uniform(0.0, 2.0, size=(6, 1, 3))), 1.0, None)
    maps["black 5x3"] = (rgba(np.zeros((3, 5, 3))), 1.0, None)
    maps["rotated 12x6"] = (rgba(rng.uniform(0.0, 3.0, size=(6, 12, 3)) * (rng.uniform(size=(6, 12, 1)) < 0.6)), 1.0, _rotation())
    return maps


def build_environment(built, name):
    """put map `name` on a scene_builder.BuiltScene"""
    rgba, scale, rotation = environment_maps()[name]
    built.environment(rgba, scale=scale)
    if rotation is not None:
        forward, back = np.eye(4, dtype=F32), np.eye(4, dtype=F32)
        forward[:3, :3], back[:3, :3] = rotation, rotation.T
        built.env.map_to_world[:] = forward.reshape(-1).tolist()
        built.env.world_to_map[:] = back.reshape(-1).tolist()


def build_cdf(values):
    """Distribution's constructor (reference src/distribution.cpp:6-33) restated sequentially in fp32: (cdf, empty)"""
    values = np.asarray(values, dtype=F32)
    total = F32(0)
    for v in values:
        total = F32(total + v)
    cdf = np.zeros(len(values), dtype=F32)
    if total == 0:
        return cdf, True
    for i, v in enumerate(values):
        cdf[i] = F32(v / total)
        if i > 0:
            cdf[i] = F32(cdf[i] + cdf[i - 1])
    cdf[-1] = 1.0
    return cdf, False


def environment_cdfs(name):
    """(theta cdf, theta empty, [phi cdf per row], [phi empty per row]) as the environment light's constructor builds them"""
    rgba = environment_maps()[name][0]
    luminance = ((F32(0) + rgba[..., 0]).astype(F32) + rgba[..., 1]).astype(F32)
    luminance = (luminance + rgba[..., 2]).astype(F32)
    rows, theta_data = [], []
    for row in luminance:
        total = F32(0)
        for v in row:
            total = F32(total + v)
        theta_data.append(total)
        rows.append(build_cdf(row))
    theta, theta_empty = build_cdf(theta_data)
    return theta, theta_empty, [r[0] for r in rows], [r[1] for r in rows]


def linear_scan(cdf, empty, xi):
    """Distribution::sample's index and pdf (reference src/distribution.cpp:35-53)"""
    if empty:
        return 0, F32(0)
    for i, c in enumerate(cdf):
        if F32(xi) <= c:
            return i, F32(c - cdf[i - 1]) if i > 0 else c
    return len(cdf) - 1, F32(0)


def _cdf_probes(cdf, grid=True):
    """u values that probe one CDF: its ends, every CDF value and (grid) every k / size, each with both neighbours (in [0, 1))"""
    size = len(cdf)
    values = {0.0, TINY, ALMOST_ONE}
    for x in list(cdf) + ([F32(F32(k) / F32(size)) for k in range(size + 1)] if grid else []):
        values.update(around(x))
    return sorted(v for v in values if 0.0 <= v <= ALMOST_ONE)


@functools.lru_cache(maxsize=None)
def env_sample_cases(name):
    """records (n, 5): point(3) u1 u2.  Every probe of the theta CDF with three u2, and for every row a u1 that selects it
    with every probe of the row's phi CDF (the k / size probes on every sixth row of a tall map)."""
    theta, theta_empty, phis, phi_empty = environment_cdfs(name)
    point = (0.25, -0.5, 1.5)
    records = []
    for u1 in _cdf_probes(theta):
        records += [list(point) + [u1, u2] for u2 in (0.0, 0.43, ALMOST_ONE)]
    for row in range(len(theta)):
        u1 = float(theta[row])   # selects `row` when the row has weight, the first row of the flat stretch otherwise
        if u1 > ALMOST_ONE:
            u1 = ALMOST_ONE
        chosen = linear_scan(theta, theta_empty, u1)[0]
        records += [list(point) + [u1, u2] for u2 in _cdf_probes(phis[chosen], grid=len(theta) <= 8 or row % 6 == 5)]
    records += [list(point) + [0.0, u2] for u2 in _cdf_probes(phis[0])]   # xi == 0: row 0 whatever its weight
    records = np.unique(np.asarray(records, dtype=F32), axis=0)
    return records


@functools.lru_cache(maxsize=None)
def env_direction_cases(name):
    """directions (n, 3), world space, with the texel (row, column) each lies in: at texel centres and at offsets of 2e-3 of a
    texel from the borders (a quarter texel under a rotated map, where the rotation's own rounding moves a direction near the
    pole by more than that).  env_pdf takes them as they are, env_emit their negation (lightWo)."""
    rgba, _, rotation = environment_maps()[name]
    height, width = rgba.shape[:2]
    edge = 0.25 if rotation is not None else 2e-3
    offsets = [(0.5, 0.5), (edge, 0.5), (1 - edge, 0.5), (0.5, edge), (0.5, 1 - edge), (edge, edge), (1 - edge, 1 - edge)]
    directions, texels = [], []
    for row in range(height):
        for column in range(width):
            stride = 1 if height * width <= 128 else 5
            for k, (fx, fy) in enumerate(offsets):
                if k > 0 and (row * width + column) % stride:
                    continue
                theta = (row + fy) / height * np.pi
                phi = (column + fx) / width * 2 * np.pi
                local = np.array([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)])
                world = local if rotation is None else rotation.astype(np.float64) @ local
                directions.append(world)   # unit length: emitPDF does not normalise its argument
                texels.append((row, column))
    return np.asarray(directions, dtype=F32), np.asarray(texels)


# numpy model of the per-cell sampling records the device builds for a CDF (pathed_hip.hip: buildGuide, buildRecords) and of
# the lookup through them (shading.h: cdfSampleRecord).  Returns (index, pdf, which path the lookup took).

def build_guide(cdf):
    size, i, guide = len(cdf), 0, []
    for j in range(size + 1):
        threshold = F32(F32(j) / F32(size))
        while i + 1 < size and not cdf[i] >= threshold:
            i += 1
        guide.append(i)
    return guide


def record_sample(cdf, empty, xi):
    size = len(cdf)
    xi = F32(xi)
    if empty:
        return 0, F32(0), "empty"
    guide = build_guide(cdf)
    bucket = min(max(int(F32(xi * F32(size))), 0), size)
    lo, hi = guide[max(bucket - 1, 0)], guide[min(bucket + 2, size)]
    at = lambda index: cdf[min(max(index, 0), size - 1)]
    if xi <= at(lo):
        return lo, (F32(at(lo) - at(lo - 1)) if lo > 0 else at(lo)), "lo"
    if xi <= at(lo + 1):
        return lo + 1, F32(at(lo + 1) - at(lo)), "lo + 1"
    if xi <= at(lo + 2):
        return lo + 2, F32(at(lo + 2) - at(lo + 1)), "lo + 2"
    first, last = min(lo + 3, hi), hi
    while first < last:
        mid = (first + last) >> 1
        if xi <= cdf[mid]:
            last = mid
        else:
            first = mid + 1
    if not xi <= cdf[first]:
        return size - 1, F32(0), "rare: none"
    return first, (F32(cdf[first] - cdf[first - 1]) if first > 0 else cdf[first]), "rare"


# ------------------------------------------------------------------------------------------------------ through the oracle

def oracle_rows(fn, records, n_out):
    """oracle_eval(fn) on every record: (n, n_out) float32"""
    records = np.asarray(records, dtype=F32)
    return np.stack([oracle_lib.evaluate(fn, record, n_out) for record in records]) if len(records) else np.zeros((0, n_out), F32)


def environment_scene(name):
    """a scene_builder.BuiltScene that holds nothing but map `name` (keep it alive beside what is created from it)"""
    from scene_builder import BuiltScene
    from pathed_amd import _capi
    built = BuiltScene(4, 4, (0, 0, 5), (0, 0, 0), fov_degrees=30)
    built.material(_capi.MAT_LAMBERTIAN)
    build_environment(built, name)
    return built


def oracle_env_rows(name, fn, records, n_out):
    built = environment_scene(name)
    scene = oracle_lib.OracleScene(built.finish())
    try:
        return np.stack([scene.env_eval(fn, record, n_out) for record in np.asarray(records, dtype=F32)])
    finally:
        scene.close()


# ------------------------------------------------------------------------------------------------------------- furnace

FURNACE_ALBEDO = 0.6
FURNACE_ANGLES = (0, 60, 80)


def furnace_cases():
    """(label, case for shading_reference.evaluate, material(20), degrees of wo from the normal): Oren-Nayar (its sigma takes the
    two parameter values), microfacet over Beckmann and over GGX, plastic over GGX; parameter 0.1 and 0.4; 0, 60 and 80 degrees"""
    out = []
    grey = (FURNACE_ALBEDO,) * 3
    for parameter in (0.1, 0.4):
        for angle in FURNACE_ANGLES:
            out.append(("oren-nayar sigma %g at %d" % (parameter, angle), ("oren-nayar", None, parameter, FURNACE_ALBEDO),
                        material(OREN_NAYAR, diffuse=grey, sigma=parameter), angle))
            for kind, name in ((MICROFACET, "microfacet"), (PLASTIC, "plastic")):
                for distribution, dname in ((BECKMANN, "beckmann"), (GGX, "ggx")):
                    if kind == PLASTIC and distribution == BECKMANN:
                        continue
                    out.append(("%s %s alpha %g at %d" % (name, dname, parameter, angle), (name, dname, parameter, FURNACE_ALBEDO),
                                material(kind, diffuse=grey, alpha=parameter, distribution=distribution), angle))
    return out


def furnace_cosine(angle):
    return 1.0 if angle == 0 else float(F32(np.cos(np.radians(angle))))


def furnace_records(entry, side):
    """side^2 material_sample records of one furnace case: the two numbers that pick the direction on a jittered side x side
    grid, the third (plastic: the FIRST, which picks the lobe) a shuffled golden-ratio sequence"""
    label, _, m, angle = entry
    rng = np.random.default_rng(sum(ord(c) for c in label))
    n = side * side
    i, j = np.divmod(np.arange(n), side)
    grid = np.stack([(i + rng.uniform(size=n)) / side, (j + rng.uniform(size=n)) / side], axis=1)
    sequence = np.modf(0.5 + rng.permutation(n) * 0.6180339887498949)[0]
    script = np.column_stack([sequence, grid]) if m[0] == PLASTIC else np.column_stack([grid, sequence])
    script = np.minimum(script.astype(F32), F32(ALMOST_ONE))
    wo = UP if angle == 0 else _with_cosine(F32(furnace_cosine(angle)))
    head = np.asarray(m + list(UP) + list(UP) + list(wo) + [0.0, 0.0], dtype=F32)
    return np.concatenate([np.broadcast_to(head, (n, 31)), script], axis=1).astype(F32)


def furnace_estimate(samples):
    """mean of throughput |cos theta_i| / pdf over material_sample results (n, 7) at the normal UP; a sample without density
    (below the horizon, black) counts zero"""
    samples = np.asarray(samples, dtype=np.float64)
    pdf, throughput, cosine = samples[:, 3], samples[:, 4], np.abs(samples[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        weight = np.where((pdf > 0) & (throughput > 0), throughput * cosine / pdf, 0.0)
    return float(weight.mean())


# what fp32 leaves of one sample's throughput |cos| / pdf: the throughput carries at most three roundings past its exact
# factors, the pdf two, the direction's component three, each of at most 2^-24 relative
FURNACE_ROUNDING = 8 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def furnace_expectation(label):
    """(expected value, standard deviation of one sample, quadrature error) of the case from the float64 reference"""
    import shading_reference
    entry = next(e for e in furnace_cases() if e[0] == label)
    return shading_reference.furnace(entry[1], furnace_cosine(entry[3]))


def furnace_allowance(label, n):
    """five standard errors of n independent samples (the scripted numbers are stratified: their error is smaller), the
    quadrature's own error and the rounding of the fp32 samples"""
    expected, deviation, quadrature = furnace_expectation(label)
    return 5.0 * deviation / np.sqrt(n) + quadrature + FURNACE_ROUNDING * expected
