"""The numpy restatement of adaptive sampling (include/pathed_hip.h: pathed_hip_select_pixels_device and the schedule of
pathed_amd/host/job.h, key "adaptive"): the noise formula of tests/noise_reference.py with a sample count per pixel, the
list of the pixels still to render, the mean in the device's order of additions, and a replay of the rounds."""
import numpy as np

import noise_reference

F = np.float32
BLOCK = 256


def errors(rgb_sum, rgb_sq_sum, counts, floor):
    """e per pixel with n = counts[pixel] (n and n / (n - 1) in float32, per pixel): sums (P, 3), counts (P,) -> (e (P,)
    float32, invalid (P,)).  A pixel with fewer than 2 samples has e = 0 and is invalid; a non-finite e counts as 0 and invalid."""
    S = np.asarray(rgb_sum, dtype=F).reshape(-1, 3)
    Q = np.asarray(rgb_sq_sum, dtype=F).reshape(-1, 3)
    counts = np.asarray(counts, dtype=np.uint32).reshape(-1)
    e = np.zeros(counts.shape, dtype=F)
    invalid = counts < 2
    for n in np.unique(counts):
        if n < 2:
            continue
        where = counts == n
        e[where], invalid[where] = noise_reference.noise(S[where], Q[where], int(n), floor)
    return e, invalid


def select(rgb_sum, rgb_sq_sum, counts, floor, threshold):
    """(e, invalid, list): the list holds, ascending, the pixels with e > threshold (compared in float32) or fewer than 2 samples"""
    e, invalid = errors(rgb_sum, rgb_sq_sum, counts, floor)
    counts = np.asarray(counts, dtype=np.uint32).reshape(-1)
    chosen = (e > F(threshold)) | (counts < 2)
    return e, invalid, np.flatnonzero(chosen).astype(np.uint32)


def mean_error(e):
    """the device's mean: per block of 256 pixels the errors added in double in pixel order, the blocks' sums added in
    block order, over the number of pixels.  np.cumsum adds one element after the other, each partial sum rounded to a
    double: the same additions in the same order as a loop over Python floats, for all full blocks at once (row by row of
    a (blocks, 256) array), then for the ragged last block, then over the blocks' sums."""
    e = np.asarray(e, dtype=F).reshape(-1).astype(np.float64)
    full = e.size // BLOCK
    partials = []
    if full:
        partials.append(np.cumsum(e[:full * BLOCK].reshape(full, BLOCK), axis=1)[:, -1])
    if e.size > full * BLOCK:
        partials.append(np.cumsum(e[full * BLOCK:])[-1:])
    partials = np.concatenate(partials)
    # (0.0 + x is x: starting the chain at the first element is starting it at zero)
    return float(np.cumsum(partials)[-1]) / e.size


def replay(uniform, min_spp, cap, target, floor):
    """The schedule replayed on uniform renders: uniform[c] = (sums, squares) of the c-sample render of every pixel, for every
    count the schedule reaches.  min(min_spp, cap) samples of every pixel; then rounds: among the pixels still active those
    with e > target stay active and go to min(2 n, cap) samples; the run ends when none is left or n == cap.
    Returns (counts (P,) uint32, rounds, samples rendered)."""
    n = min(min_spp, cap)
    pixels = np.asarray(uniform[n][0]).reshape(-1, 3).shape[0]
    counts = np.full(pixels, n, dtype=np.uint32)
    active = np.ones(pixels, dtype=bool)
    rounds = 0
    rendered = n * pixels
    while n < cap:
        e, _, _ = select(uniform[n][0], uniform[n][1], np.full(pixels, n, dtype=np.uint32), floor, target)
        active &= e > F(target)
        if not active.any():
            break
        following = min(2 * n, cap)
        counts[active] = following
        rendered += (following - n) * int(active.sum())
        rounds += 1
        n = following
    return counts, rounds, rendered
