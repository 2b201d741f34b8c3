"""The numpy float32 restatement of the second-moment sums and of the noise figure (include/pathed_hip.h:
pathed_hip_render_moments_device, pathed_hip_noise_estimate_device), operation for operation, and a float64 evaluation of
the same formulas to check it against.  numpy's float32 multiply, add, divide and square root are the correctly rounded
IEEE ones and numpy never contracts a multiply and an add, which is what the device build (-ffp-contract=off) computes."""
import numpy as np

F = np.float32


def square_sums(samples, start=None):
    """q = q + (x * x) over the samples in order: samples (n, ..., 3) float32 -> (..., 3) float32, continued from `start`"""
    samples = np.asarray(samples, dtype=F)
    q = np.zeros(samples.shape[1:], dtype=F) if start is None else np.array(start, dtype=F)
    for x in samples:
        q = (q + (x * x).astype(F)).astype(F)
    return q


def sums(samples, start=None):
    """s = s + x over the samples in order (what k_resolve adds)"""
    samples = np.asarray(samples, dtype=F)
    s = np.zeros(samples.shape[1:], dtype=F) if start is None else np.array(start, dtype=F)
    for x in samples:
        s = (s + x).astype(F)
    return s


def moments(rgb_sum, rgb_sq_sum, n):
    """(m_c, v_c): m = S / n, d = Q / n - m * m, v = max(d, 0) * (n / (n - 1)), all float32, n and n / (n - 1) computed once"""
    S = np.asarray(rgb_sum, dtype=F)
    Q = np.asarray(rgb_sq_sum, dtype=F)
    nf = F(n)
    bessel = F(nf / F(nf - F(1.0)))
    with np.errstate(all="ignore"):
        m = (S / nf).astype(F)
        d = ((Q / nf).astype(F) - (m * m).astype(F)).astype(F)
        v = (np.where(d > F(0.0), d, F(0.0)).astype(F) * bessel).astype(F)
    return m, v


def noise(rgb_sum, rgb_sq_sum, n, floor):
    """e = sqrt(((v_r + v_g) + v_b) / n) / (((m_r + m_g) + m_b) + floor) per pixel, float32; a non-finite e counts as 0:
    (e, mask of the pixels where it was not finite)"""
    m, v = moments(rgb_sum, rgb_sq_sum, n)
    nf = F(n)
    with np.errstate(all="ignore"):
        spread = ((v[..., 0] + v[..., 1]).astype(F) + v[..., 2]).astype(F)
        brightness = (((m[..., 0] + m[..., 1]).astype(F) + m[..., 2]).astype(F) + F(floor)).astype(F)
        e = (np.sqrt((spread / nf).astype(F)).astype(F) / brightness).astype(F)
    invalid = ~np.isfinite(e)
    return np.where(invalid, F(0.0), e).astype(F), invalid


def standard_error(rgb_sum, rgb_sq_sum, n):
    """sqrt(v_c / n) per channel, float32: what auto-stderr.exr holds"""
    _, v = moments(rgb_sum, rgb_sq_sum, n)
    return np.sqrt((v / F(n)).astype(F)).astype(F)


def noise_float64(rgb_sum, rgb_sq_sum, n, floor):
    """the same formula in float64 on the same inputs: (e, d_c / (Q_c / n), the share of Q / n that survives the subtraction)"""
    S = np.asarray(rgb_sum, dtype=np.float64)
    Q = np.asarray(rgb_sq_sum, dtype=np.float64)
    n = float(n)
    m = S / n
    d = Q / n - m * m
    v = np.maximum(d, 0.0) * (n / (n - 1.0))
    e = np.sqrt(v.sum(axis=-1) / n) / (m.sum(axis=-1) + float(np.float32(floor)))
    with np.errstate(all="ignore"):
        survives = np.where(Q > 0.0, d / (Q / n), 1.0)
    return e, survives
