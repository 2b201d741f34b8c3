#!/usr/bin/env python3
"""Moving placements (pathed_hip_scene_set_instance_transforms, pathed_hip_scene_rebuild_top), two
measurements in one process, three arms each -- move (refit), move + rebuild (per device builder), destroy + create:

  (1) update time: set_instance_transforms (wall time of the call, which returns synchronised, and the device time of its
      kernels), the same followed by rebuild_top, and destroying the scene and creating it again with the same placements
      (wall time) -- at the 400 placements of jobs/instances-field.json, at 4 096 and at 262 144 placements of a
      5 120-triangle stand-in on a grid
  (2) render rate on the REFITTED tree, on the REBUILT trees and on a FRESH build of the same placements, the scenes
      alternating: a small rigid motion (every placement turned a few degrees and shifted by a tenth of the spacing) and a
      full shuffle of the positions, on the field scene and on the 4 096-placement grid; the image sums must agree

The lines of a run are appended to the log.

    tools/instances_motion.py [--spp 64] [--repeats 3] [--counts 4096,262144] [--log profiles/instances_motion.log]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pathed_amd.integrator import HipScene  # noqa: E402
from pathed_amd.instances import InstanceSet  # noqa: E402
from pathed_amd.scene import LoadedScene  # noqa: E402

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def rigid(transforms, shift, rng):
    """every placement turned about its own position's vertical by up to 10 degrees and shifted by up to `shift` in x and z"""
    out = np.asarray(transforms, dtype=np.float64).reshape(-1, 3, 4).copy()
    angle = np.radians(rng.uniform(-10.0, 10.0, len(out)))
    turn = np.zeros((len(out), 3, 3))
    turn[:, 0, 0], turn[:, 0, 2], turn[:, 1, 1], turn[:, 2, 0], turn[:, 2, 2] = np.cos(angle), np.sin(angle), 1.0, -np.sin(angle), np.cos(angle)
    out[:, :, :3] = turn @ out[:, :, :3]
    out[:, 0, 3] += rng.uniform(-shift, shift, len(out))
    out[:, 2, 3] += rng.uniform(-shift, shift, len(out))
    return out.astype(np.float32).reshape(-1, 12)


def shuffled(transforms, rng):
    """the placements keep their linear parts and exchange their positions by a random permutation"""
    out = np.asarray(transforms, dtype=np.float32).reshape(-1, 3, 4).copy()
    out[:, :, 3] = out[rng.permutation(len(out)), :, 3]
    return out.reshape(-1, 12)


def grid_scene(count, width, height):
    """`count` placements of a 5 120-triangle stand-in on a square grid over a floor under an emitter"""
    from instances_scene import icosphere
    from scene_builder import BuiltScene
    side = int(np.ceil(np.sqrt(count)))
    spacing = 3.0
    half = spacing * side / 2
    scene = BuiltScene(width, height, origin=(0.0, 0.55 * half + 6.0, 1.3 * half + 10.0), target=(0.0, 0.5, 0.0), fov_degrees=40.0)
    floor = scene.material(diffuse=(0.6, 0.6, 0.55))
    light = scene.material(diffuse=(0.0, 0.0, 0.0), emit=(20.0, 19.0, 17.0))
    skin = scene.material(diffuse=(0.7, 0.35, 0.25))
    scene.quad([(-half - 4, 0, -half - 4), (-half - 4, 0, half + 4), (half + 4, 0, half + 4), (half + 4, 0, -half - 4)], floor)
    scene.quad([(-half / 3, half + 8, -half / 3), (half / 3, half + 8, -half / 3), (half / 3, half + 8, half / 3), (-half / 3, half + 8, half / 3)], light)
    positions, faces, normals, uvs = icosphere((0.0, 1.2, 0.0), 1.0, 4)
    scene.mesh(positions, faces, skin, normals=normals, uvs=uvs)
    pointer = scene.finish()
    k = np.arange(count)
    angle = np.radians(23.0 * k)
    scale = 0.8 + 0.05 * (k % 5)
    transforms = np.zeros((count, 3, 4))
    transforms[:, 0, 0], transforms[:, 0, 2] = scale * np.cos(angle), scale * np.sin(angle)
    transforms[:, 1, 1] = scale
    transforms[:, 2, 0], transforms[:, 2, 2] = -scale * np.sin(angle), scale * np.cos(angle)
    transforms[:, 0, 3] = ((k % side) - (side - 1) / 2) * spacing
    transforms[:, 2, 3] = ((k // side) - (side - 1) / 2) * spacing
    return scene, pointer, [(2, 1)], np.zeros(count, dtype=np.int64), transforms.astype(np.float32).reshape(count, 12), spacing


def instance_set(prototypes, which, transforms):
    """an InstanceSet without a Python object per placement (262 144 of them): the C array is filled from numpy"""
    from pathed_amd import _capi
    import ctypes as C
    placements = InstanceSet(prototypes, [(int(which[0]), transforms[0])] if len(which) else [])
    record = np.zeros(len(which), dtype=np.dtype([("prototype", np.int32), ("transform", np.float32, 12)]))
    record["prototype"], record["transform"] = which, transforms
    placements._records = record
    placements._instance_array = C.cast(record.ctypes.data, C.POINTER(_capi.PathedInstance))
    placements.desc.n_instances, placements.desc.instances = len(which), placements._instance_array
    return placements


def create(pointer, prototypes, which, transforms):
    return HipScene(pointer, device=0, instances=instance_set(prototypes, which, transforms))


def move(gpu, transforms):
    """(wall ms, device ms) of one call of the host entry (the call returns synchronised); the Python-side set is left alone"""
    import ctypes as C
    transforms = np.ascontiguousarray(transforms, dtype=np.float32)
    ms = C.c_float(0.0)
    start = time.perf_counter()
    code = gpu._lib.pathed_hip_scene_set_instance_transforms(gpu._handle, transforms.ctypes.data_as(C.POINTER(C.c_float)), len(transforms), C.byref(ms))
    wall = (time.perf_counter() - start) * 1e3
    assert code == 0, gpu._lib.pathed_hip_last_error()
    return wall, float(ms.value)


BUILDERS = ("lbvh", "ploc")


def rebuild(gpu, builder):
    """(wall ms, device ms) of one rebuild_top (the call returns synchronised)"""
    start = time.perf_counter()
    device = gpu.rebuild_top(builder)
    return (time.perf_counter() - start) * 1e3, device


def update_times(name, pointer, prototypes, which, transforms, shift, repeats):
    rng = np.random.default_rng(5)
    gpu = create(pointer, prototypes, which, transforms)
    gpu.trace(np.array([[0, 50, 0, 1e-3, 0, -1, 0, 1e5]], dtype=np.float32))
    walls, devices = [], []
    for k in range(repeats + 1):   # (the first call allocates the second record buffer and the refit's working memory)
        moved = rigid(transforms, shift, rng)
        wall, device = move(gpu, moved)
        if k > 0:
            walls.append(wall)
            devices.append(device)
    stats = gpu.stats()
    rebuilt = {}
    for builder in BUILDERS:   # move + rebuild: both calls' wall time, both calls' device time
        pairs = []
        for k in range(repeats + 1):   # (the first rebuild after a refit frees the refit's side arrays; the move allocates them again)
            moved = rigid(transforms, shift, rng)
            wall, device = move(gpu, moved)
            more_wall, more_device = rebuild(gpu, builder)
            if k > 0:
                pairs.append((wall + more_wall, device + more_device))
        rebuilt[builder] = (pairs, gpu.stats())
    recreates = []
    for _ in range(max(2, repeats // 3)):
        placements = instance_set(prototypes, which, moved)   # (made outside the timed stretch: the caller has it anyway)
        start = time.perf_counter()
        gpu.close()
        gpu = HipScene(pointer, device=0, instances=placements)
        recreates.append((time.perf_counter() - start) * 1e3)
    gpu.close()
    say("update %-8s %7d placements, %d nodes, depth %d: set_instance_transforms wall median %.3f ms (%s), device %.3f ms; destroy + create_instanced %.1f ms (%s): x%.0f"
        % (name, len(which), stats["bvh_nodes"], stats["bvh_max_depth"], float(np.median(walls)), " ".join("%.3f" % v for v in walls), float(np.median(devices)),
           float(np.median(recreates)), " ".join("%.1f" % v for v in recreates), float(np.median(recreates)) / float(np.median(walls))))
    for builder in BUILDERS:
        pairs, after = rebuilt[builder]
        wall = float(np.median([w for w, _ in pairs]))
        say("update %-8s %7d placements, move + rebuild_top(%s): %d nodes, depth %d; wall median %.3f ms (%s), device %.3f ms; destroy + create is x%.2f of it"
            % (name, len(which), builder, after["bvh_nodes"], after["bvh_max_depth"], wall, " ".join("%.3f" % w for w, _ in pairs),
               float(np.median([d for _, d in pairs])), float(np.median(recreates)) / wall))


def rate(gpu, spp, last_bounce, accum):
    accum[:] = 0
    start = time.perf_counter()
    gpu.render(1, 0, spp, 0, last_bounce, accum)
    seconds = time.perf_counter() - start
    return gpu.width * gpu.height * spp / seconds / 1e6, float(accum.astype(np.float64).sum())


def render_rates(name, pointer, prototypes, which, transforms, moved, spp, bounces, repeats, shape):
    arms = {"refitted": create(pointer, prototypes, which, transforms)}
    move(arms["refitted"], moved)
    for builder in BUILDERS:
        arms["rebuilt " + builder] = create(pointer, prototypes, which, transforms)
        move(arms["rebuilt " + builder], moved)
        rebuild(arms["rebuilt " + builder], builder)
    arms["fresh"] = create(pointer, prototypes, which, moved)
    accum = np.zeros(shape + (3,), dtype=np.float32)
    for gpu in arms.values():
        gpu.render(1, 0, 1, 0, 2, accum)
    rates, sums = {label: [] for label in arms}, {}
    for _ in range(repeats):
        for label, gpu in arms.items():
            value, sums[label] = rate(gpu, spp, bounces, accum)
            rates[label].append(value)
    medians = {label: float(np.median(values)) for label, values in rates.items()}
    equal = all(value == sums["fresh"] for value in sums.values())
    say("render %-22s %s; image sums %s" % (name, "; ".join(
        "%s %.1f Msamples/s (%s: spread %.1f %%, %.3f of fresh)" % (label, medians[label], " ".join("%.1f" % v for v in rates[label]),
                                                                  100.0 * (max(rates[label]) - min(rates[label])) / medians[label], medians[label] / medians["fresh"])
        for label in arms), "equal" if equal else "DIFFER %r" % sums))
    for gpu in arms.values():
        gpu.close()
    return equal


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--spp", type=int, default=64)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--counts", default="4096,262144")
    parser.add_argument("--log", default=os.path.join(ROOT, "profiles", "instances_motion.log"))
    args = parser.parse_args()
    counts = [int(value) for value in args.counts.split(",") if value]

    job = json.load(open(os.path.join(ROOT, "jobs", "instances-field.json")))
    field = LoadedScene(job["scene"], job["width"], job["height"])
    field_which = np.array([p for p, _ in field.instances], dtype=np.int64)
    field_transforms = np.array([t for _, t in field.instances], dtype=np.float32).reshape(-1, 12)
    say("# tools/instances_motion.py --spp %d --repeats %d --counts %s" % (args.spp, args.repeats, args.counts))
    update_times("field", field.desc, field.prototypes, field_which, field_transforms, 0.34, 3 * args.repeats)
    grids = {}
    for count in counts:
        grids[count] = grid_scene(count, 1024, 768)
        built, pointer, prototypes, which, transforms, spacing = grids[count]
        update_times("grid", pointer, prototypes, which, transforms, 0.1 * spacing, 3 * args.repeats)

    shape = (job["height"], job["width"])
    rng = np.random.default_rng(9)
    same = []
    same.append(render_rates("field, rigid motion", field.desc, field.prototypes, field_which, field_transforms, rigid(field_transforms, 0.34, rng),
                 args.spp, job["lastBounce"], args.repeats, shape))
    same.append(render_rates("field, shuffle", field.desc, field.prototypes, field_which, field_transforms, shuffled(field_transforms, rng),
                 args.spp, job["lastBounce"], args.repeats, shape))
    if counts:
        built, pointer, prototypes, which, transforms, spacing = grids[counts[0]]
        same.append(render_rates("grid %d, rigid motion" % counts[0], pointer, prototypes, which, transforms, rigid(transforms, 0.1 * spacing, rng), args.spp, 4, args.repeats, (768, 1024)))
        same.append(render_rates("grid %d, shuffle" % counts[0], pointer, prototypes, which, transforms, shuffled(transforms, rng), args.spp, 4, args.repeats, (768, 1024)))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as handle:
        handle.write("\n".join(LINES) + "\n")
    assert all(same), "the arms' image sums differ"


if __name__ == "__main__":
    main()
