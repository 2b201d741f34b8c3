"""The moving scene of the shutter tests (test_shutter_host.py, test_gpu_shutter.py): instances_scene's general placements are
the placements at shutter time 0, CLOSE_PLACEMENTS the same placements at time 1 -- each rotated, scaled non-uniformly and
translated differently, one left exactly where it is.  No test lives here."""
import numpy as np

from pathed_amd import flatten_instances
from pathed_amd import instances as I

import instances_scene as S

OPEN_PLACEMENTS = S.GENERAL_PLACEMENTS
STILL = 1   # the placement whose two transforms are bit-equal

CLOSE_PLACEMENTS = [
    (S.P, S.placed(np.diag([2.2, 1.2, 1.7]) @ S.rotation((0.2, 1.0, 0.4), 95.0), (-2.6, 4.4, 3.5), S.P_CENTRE)),
    OPEN_PLACEMENTS[1],
    (S.Q, S.placed(np.diag([1.5, 3.4, 2.1]) @ S.rotation((1.0, 0.3, 0.2), -50.0), (2.8, 3.3, 1.0), S.Q_CENTRE)),
    (S.P, S.placed(np.diag([-1.1, 2.3, 1.4]) @ S.rotation((0.1, 0.4, 1.0), 75.0), (3.2, 1.9, 4.0), S.P_CENTRE)),
    (S.P, S.placed(np.diag([130.0, 170.0, 150.0]) @ S.rotation((1.0, 0.2, 0.5), 110.0), (-120.0, 210.0, -940.0), S.P_CENTRE)),
]


def transforms(placements):
    return np.stack([t for _, t in placements]).astype(np.float32)


def placements_at(t):
    """The static placements of shutter time t by the rule of include/pathed_hip.h: interpolate_transforms of the two sets, entry
    by entry in float32, and a placement whose two transforms are bit-equal keeps its transform (0.7 a + 0.3 a need not be a in
    float32; at t = 0, 0.25 and 1 it is, which test_shutter_host.py asserts for this set)."""
    a, b = transforms(OPEN_PLACEMENTS), transforms(CLOSE_PLACEMENTS)
    at = I.interpolate_transforms(a, b, t)
    still = (a.view(np.uint32) == b.view(np.uint32)).all(axis=1)
    at[still] = a[still]
    return [(prototype, row) for (prototype, _), row in zip(OPEN_PLACEMENTS, at)]


def first_hit_change(width, height):
    """The share of pixels whose pixel-centre camera ray changes its first-hit primitive between the flattened scenes of t = 0
    and t = 1, by the CPU oracle alone: were it small, a render that ignored the time could pass the per-sample test."""
    import oracle_lib
    built, pointer, prototypes, _ = S.build(OPEN_PLACEMENTS, width, height)
    rays = S.camera_rays(width, height, S.CAMERA["origin"], S.CAMERA["target"])
    prims = []
    for t in (0.0, 1.0):
        flat = flatten_instances(pointer, prototypes, placements_at(t))
        hits = oracle_lib.OracleScene(flat.desc).trace(rays)
        prims.append(np.ascontiguousarray(hits[:, 3]).view(np.int32).copy())
    return float((prims[0] != prims[1]).mean())
