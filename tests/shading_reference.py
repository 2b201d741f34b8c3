"""A plain float64 numpy restatement of f and pdf of the rough BSDFs -- Lambertian, Oren-Nayar, microfacet and plastic over the
Beckmann and GGX distributions -- in the SHADING FRAME (y up), and the hemisphere quadrature the furnace tests hold sampled
estimates to.  Written from the formulas (reference src/oren_nayar.cpp, src/beckmann.cpp, src/ggx.cpp, src/microfacet.cpp,
src/plastic.cpp, include/tangent_frame.h), not from the oracle: float64 throughout, Oren-Nayar in its trigonometric form,
vectorised over directions; it shares no code and no operation order with oracle/oracle.cpp or the kernels.

Directions are arrays (..., 3); wo is one vector with wo.y >= 0, and the shading normal is the geometric normal.
"""
import numpy as np

CLAMP = float(np.float32(0.9999))


def _sin_theta(v):
    return np.sqrt(np.maximum(0.0, 1.0 - v[..., 1] ** 2))


def _tan2_theta(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 - v[..., 1] ** 2) / v[..., 1] ** 2


def _clamped(v):
    """TangentFrame::clamp (include/tangent_frame.h:79-102): a vector with a component at 0.9999 becomes that axis"""
    out = v.copy()
    done = np.zeros(v.shape[:-1], dtype=bool)
    for sign in (1.0, -1.0):
        for axis in range(3):
            hit = ~done & (sign * v[..., axis] >= CLAMP)
            replacement = np.zeros(3)
            replacement[axis] = sign
            out[hit] = replacement
            done |= hit
    return out


def _cos2_phi(v):
    sin_theta = _sin_theta(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos_phi = np.where(sin_theta == 0, 1.0, np.clip(v[..., 0] / sin_theta, -1.0, 1.0))
    return cos_phi ** 2


def _sin2_phi(v):
    c = _clamped(v)
    sin_theta = _sin_theta(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        sin_phi = np.where(sin_theta == 0, 0.0, np.clip(c[..., 2] / sin_theta, -1.0, 1.0))
    return sin_phi ** 2


def beckmann_d(alpha, wh):
    tan2 = _tan2_theta(wh)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = np.exp(-tan2 * (_cos2_phi(wh) / alpha ** 2 + _sin2_phi(wh) / alpha ** 2)) / (np.pi * alpha ** 2 * wh[..., 1] ** 4)
    return np.where(np.isinf(tan2), 0.0, d)


def _beckmann_lambda(alpha, w):
    with np.errstate(divide="ignore", invalid="ignore"):
        tan = np.abs(_sin_theta(w) / w[..., 1])
        width = np.sqrt(_cos2_phi(w) * alpha ** 2 + _sin2_phi(w) * alpha ** 2)
        a = 1.0 / (width * tan)
        value = (1 - 1.259 * a + 0.396 * a * a) / (3.535 * a + 2.181 * a * a)
    return np.where(np.isinf(tan) | (a >= 1.6), 0.0, value)


def beckmann_g(alpha, wo, wi):
    return 1.0 / (1.0 + _beckmann_lambda(alpha, wo) + _beckmann_lambda(alpha, wi))


def ggx_d(alpha, wh):
    tan2 = _tan2_theta(wh)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = alpha ** 2 / (np.pi * wh[..., 1] ** 4 * (alpha ** 2 + tan2) ** 2)
    return np.where(np.isinf(tan2), 0.0, d)


def _ggx_g1(alpha, v):
    tan2 = _tan2_theta(v)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isinf(tan2), 0.0, 2.0 / (1.0 + np.sqrt(1.0 + alpha ** 2 * tan2)))


def ggx_g(alpha, wo, wi):
    return _ggx_g1(alpha, wo) * _ggx_g1(alpha, wi)


def fresnel(cos_i, eta_i, eta_t):
    sin_t = eta_i / eta_t * np.sqrt(np.maximum(0.0, 1.0 - cos_i ** 2))
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t ** 2))
    parallel = (eta_t * cos_i - eta_i * cos_t) / (eta_t * cos_i + eta_i * cos_t)
    perpendicular = (eta_i * cos_i - eta_t * cos_t) / (eta_i * cos_i + eta_t * cos_t)
    return np.where(sin_t > 1.0, 1.0, 0.5 * (parallel ** 2 + perpendicular ** 2))


def lambertian(albedo, wo, wi):
    up = wi[..., 1] >= 0
    return np.where(up, albedo / np.pi, 0.0), np.where(up, wi[..., 1] / np.pi, 0.0)


def oren_nayar(albedo, sigma, wo, wi):
    """f and the pdf of its cosine-hemisphere sampling"""
    a = 1.0 - sigma ** 2 / (2.0 * (sigma ** 2 + 0.33))
    b = 0.45 * sigma ** 2 / (sigma ** 2 + 0.09)
    theta_i, theta_o = np.arccos(np.clip(wi[..., 1], -1, 1)), np.arccos(np.clip(wo[1], -1, 1))
    phi_i, phi_o = np.arctan2(wi[..., 2], wi[..., 0]), np.arctan2(wo[2], wo[0])
    rough = np.maximum(0.0, np.cos(phi_i - phi_o)) * np.sin(np.maximum(theta_i, theta_o)) * np.tan(np.minimum(theta_i, theta_o))
    up = wi[..., 1] >= 0
    return np.where(up, albedo / np.pi * (a + b * rough), 0.0), np.where(up, wi[..., 1] / np.pi, 0.0)


def microfacet(alpha, distribution, wo, wi):
    d_of, g_of = (ggx_d, ggx_g) if distribution == "ggx" else (beckmann_d, beckmann_g)
    with np.errstate(divide="ignore", invalid="ignore"):
        half = wo + wi
        wh = half / np.linalg.norm(half, axis=-1, keepdims=True)
        d = d_of(alpha, wh)
        pdf = d * np.abs(wh[..., 1]) / (4.0 * (wh @ wo))
        f = d * g_of(alpha, wo, wi) * fresnel(np.clip(np.sum(wi * wh, axis=-1), 0.0, 1.0), 1.0, 1.5) / (4.0 * np.abs(wi[..., 1]) * abs(wo[1]))
    up = wi[..., 1] > 0
    return np.where(up, f, 0.0), np.where(up, pdf, 0.0)


def plastic(albedo, alpha, distribution, wo, wi):
    fd, pd = lambertian(albedo, wo, wi)
    fm, pm = microfacet(alpha, distribution, wo, wi)
    return fd + fm, (pd + pm) / 2.0


def evaluate(case, wo, wi):
    """case = (kind, distribution, parameter, albedo): 'oren-nayar' (parameter sigma), 'microfacet', 'plastic' (parameter alpha)"""
    kind, distribution, parameter, albedo = case
    if kind == "oren-nayar":
        return oren_nayar(albedo, parameter, wo, wi)
    if kind == "microfacet":
        return microfacet(parameter, distribution, wo, wi)
    return plastic(albedo, parameter, distribution, wo, wi)


def _moments(case, wo, rows):
    """midpoint rule over (cos theta, phi), rows x 2 rows cells: (integral of f cos, integral of (f cos)^2 / pdf)"""
    mu = (np.arange(rows) + 0.5) / rows
    phi = (np.arange(2 * rows) + 0.5) / (2 * rows) * 2 * np.pi
    first = second = 0.0
    for block in np.array_split(mu, max(1, rows // 128)):   # (bounded memory)
        m, p = np.meshgrid(block, phi, indexing="ij")
        s = np.sqrt(1.0 - m * m)
        wi = np.stack([s * np.cos(p), m, s * np.sin(p)], axis=-1)
        f, pdf = evaluate(case, wo, wi)
        value = f * m
        with np.errstate(divide="ignore", invalid="ignore"):
            squared = np.where(pdf > 0, value * value / pdf, 0.0)
        first += value.sum()
        second += squared.sum()
    cell = (1.0 / rows) * (2 * np.pi / (2 * rows))
    return first * cell, second * cell


def furnace(case, cos_o, rows=768):
    """(expected value of throughput |cos| / pdf under the BSDF's own sampling, its standard deviation, the quadrature's error:
    the difference between two resolutions)"""
    wo = np.array([0.0, cos_o, -np.sqrt(max(0.0, 1.0 - cos_o * cos_o))])
    coarse, _ = _moments(case, wo, rows // 2)
    fine, second = _moments(case, wo, rows)
    return fine, np.sqrt(max(0.0, second - fine * fine)), abs(fine - coarse)
